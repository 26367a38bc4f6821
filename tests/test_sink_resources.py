"""Register remarks of the region-delete kernels (salva_amd/csrc/sink.hip), checked without a GPU in the manner of
tests/test_compound_sampling_resources.py.  The predicates walk a mesh hierarchy or a parts table without a stack, the compaction
keeps its four array pointers in a by-value struct indexed by an unrolled loop: none may use scratch or spill a register.  The remarks
report, in VGPRs: k_sink_plane_box 10, k_sink_shape 15, k_sink_mesh 46, k_sink_compound 51, k_sink_block_counts 5,
k_sink_scan_counts 16, k_sink_scan_totals 22, k_sink_scatter 10 - all at 8 waves per SIMD; what is asserted is the occupancy step those
counts fall in (at most 64 VGPRs, 8 waves)."""
import pytest

from test_kernel_resources import one, pytestmark, resources  # noqa: F401

KERNELS = ("k_sink_plane_box", "k_sink_shape", "k_sink_mesh", "k_sink_compound", "k_sink_block_counts", "k_sink_scan_counts",
           "k_sink_scan_totals", "k_sink_scatter")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return resources("sink.hip", tmp_path_factory.mktemp("sink_resources"))


@pytest.mark.parametrize("kernel", KERNELS)
def test_sink_kernel_has_no_scratch_and_eight_waves(table, kernel):
    r = one(table, kernel)
    print(kernel, r)
    assert r["scratch"] == 0 and r["spilled"] == 0, r
    assert r["vgprs"] <= 64 and r["waves"] >= 8, r


def test_every_kernel_of_the_file_is_listed(table):
    assert sorted(k for k in table) and len(table) == len(KERNELS), sorted(table)

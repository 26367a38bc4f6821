"""Register remarks of the field evaluator's kernels (salva_amd/csrc/field.hip), checked without a GPU in the manner
of tests/test_sink_resources.py.  The file carries the reference's other kernels as wave-uniform branches of kernel_eval, and the two
summing kernels keep nine accumulators per lane: none may use scratch or spill a vector register.  The remarks report, in VGPRs:
k_field_bbox 10, k_field_keys 20, k_field_scatter 8, k_field_order 14, k_field_points 49 - all at 8 waves per SIMD - and
k_field_lattice 74 at 6 waves per SIMD with 20 512 bytes of static LDS (two 8 KiB record chunks, the run table of a group and the
scan's wave totals): a workgroup is 8 waves, two per SIMD, so three bricks share a CU by registers and seven by LDS.  What is asserted
is the occupancy step those counts fall in."""
import pytest

from test_kernel_resources import one, pytestmark, resources  # noqa: F401

EIGHT_WAVES = ("k_field_bbox", "k_field_keys", "k_field_scatter", "k_field_order", "k_field_points")
SIX_WAVES = ("k_field_lattice",)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return resources("field.hip", tmp_path_factory.mktemp("field_resources"))


@pytest.mark.parametrize("kernel", EIGHT_WAVES)
def test_field_kernel_has_no_scratch_and_eight_waves(table, kernel):
    r = one(table, kernel)
    print(kernel, r)
    assert r["scratch"] == 0 and r["spilled"] == 0, r
    assert r["vgprs"] <= 64 and r["waves"] >= 8, r


@pytest.mark.parametrize("kernel", SIX_WAVES)
def test_brick_kernel_has_no_scratch_and_six_waves(table, kernel):
    r = one(table, kernel)
    print(kernel, r)
    assert r["scratch"] == 0 and r["spilled"] == 0, r
    assert r["vgprs"] <= 80 and r["waves"] >= 6, r


def test_every_kernel_of_the_file_is_listed(table):
    assert sorted(k for k in table) and len(table) == len(EIGHT_WAVES) + len(SIX_WAVES), sorted(table)

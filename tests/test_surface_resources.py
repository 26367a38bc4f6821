"""Register remarks of the surface extractor's kernels (salva_amd/csrc/surface.hip), checked without a GPU in the
manner of tests/test_field_resources.py.  The passes stream over the nodes with a few words of state per lane; none may use scratch or
spill a vector register - the case of a tetrahedron is one 64-bit load from the constant table and is taken apart by shifts, never
indexed as an array in registers.  The remarks report, in VGPRs: k_surface_classify 12, k_surface_emit 27, k_surface_normals 11,
k_surface_bounds 11 - all at 8 waves per SIMD, no LDS.  What is asserted is the occupancy step those counts fall in.  The file also
instantiates the library scans and the reduction it calls (hipcub); those are held to "no scratch, no spill" with the rest."""
import pytest

from test_kernel_resources import one, pytestmark, resources  # noqa: F401

EIGHT_WAVES = ("k_surface_classify", "k_surface_emit", "k_surface_normals", "k_surface_bounds")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return resources("surface.hip", tmp_path_factory.mktemp("surface_resources"))


@pytest.mark.parametrize("kernel", EIGHT_WAVES)
def test_surface_kernel_has_no_scratch_and_eight_waves(table, kernel):
    r = one(table, kernel)
    print(kernel, r)
    assert r["scratch"] == 0 and r["spilled"] == 0, r
    assert r["vgprs"] <= 64 and r["waves"] >= 8, r


def test_no_kernel_of_the_file_uses_scratch(table):
    for name, r in table.items():
        assert r["scratch"] == 0 and r["spilled"] == 0, (name, r)


def test_every_kernel_of_the_file_is_listed(table):
    own = sorted(k for k in table if "k_surface" in k)
    assert len(own) == len(EIGHT_WAVES), own
    assert all(k.startswith("_ZN5salva") or "rocprim" in k or "hipcub" in k for k in table), sorted(table)

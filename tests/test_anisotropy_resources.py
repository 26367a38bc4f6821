"""Register remarks of the anisotropic kernels (salva_amd/csrc/anisotropy.hip), checked without a GPU in the manner of
tests/test_surface_resources.py.  k_aniso_moments keeps ten sums, the symmetric 3 x 3 matrix, the accumulated rotation and the six
entries of the metric in named scalars - indexed as arrays they would live in scratch - and k_aniso_points three float4 records per
candidate and five sums.  The remarks report, in VGPRs: k_aniso_moments 56, k_aniso_points 48, k_aniso_gather 14, k_aniso_pack 18 - all
at 8 waves per SIMD, no LDS, no scratch.  What is asserted is the occupancy step those counts fall in: the one the build reports
(DESIGN.md §23), not a target."""
import pytest

from test_kernel_resources import one, pytestmark, resources  # noqa: F401

EIGHT_WAVES = ("k_aniso_moments", "k_aniso_points", "k_aniso_gather", "k_aniso_pack")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return resources("anisotropy.hip", tmp_path_factory.mktemp("anisotropy_resources"))


@pytest.mark.parametrize("kernel", EIGHT_WAVES)
def test_anisotropy_kernel_has_no_scratch_and_eight_waves(table, kernel):
    r = one(table, kernel)
    print(kernel, r)
    assert r["scratch"] == 0 and r["spilled"] == 0, r
    assert r["vgprs"] <= 64 and r["waves"] >= 8, r


def test_no_kernel_of_the_file_uses_scratch(table):
    for name, r in table.items():
        assert r["scratch"] == 0 and r["spilled"] == 0, (name, r)


def test_every_kernel_of_the_file_is_listed(table):
    own = sorted(k for k in table if "k_aniso" in k)
    assert len(own) == len(EIGHT_WAVES), own
    assert all(k.startswith("_ZN5salva") for k in table), sorted(table)

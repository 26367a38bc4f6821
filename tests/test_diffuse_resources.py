"""Register remarks of the diffuse kernels (salva_amd/csrc/diffuse.hip), checked without a GPU in the manner of
tests/test_anisotropy_resources.py.  The two potential kernels keep their sums in named scalars - no LDS, no scratch.  The remarks
report, in VGPRs: k_diffuse_sums 44, k_diffuse_crest 32, k_diffuse_pack 12, and for the set k_diffuse_add 18, k_diffuse_get 24,
k_diffuse_advect 26, k_diffuse_compact 20, k_diffuse_rate 14, k_diffuse_emit 54 - all at 8 waves per SIMD.  What is asserted is the occupancy
step those counts fall in: the one the build reports, not a target."""
import pytest

from test_kernel_resources import one, pytestmark, resources  # noqa: F401

EIGHT_WAVES = ("k_diffuse_sums", "k_diffuse_crest", "k_diffuse_pack", "k_diffuse_add", "k_diffuse_get", "k_diffuse_advect", "k_diffuse_compact",
               "k_diffuse_rate", "k_diffuse_emit")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return resources("diffuse.hip", tmp_path_factory.mktemp("diffuse_resources"))


@pytest.mark.parametrize("kernel", EIGHT_WAVES)
def test_diffuse_kernel_has_no_scratch_and_eight_waves(table, kernel):
    r = one(table, kernel)
    print(kernel, r)
    assert r["scratch"] == 0 and r["spilled"] == 0, r
    assert r["vgprs"] <= 64 and r["waves"] >= 8, r


def test_no_kernel_of_the_file_uses_scratch(table):
    for name, r in table.items():
        assert r["scratch"] == 0 and r["spilled"] == 0, (name, r)


def test_every_kernel_of_the_file_is_listed(table):
    own = sorted(k for k in table if "k_diffuse" in k)
    assert len(own) == len(EIGHT_WAVES), own
    assert all(k.startswith("_ZN5salva") for k in table), sorted(table)

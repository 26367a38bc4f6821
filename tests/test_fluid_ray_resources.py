"""Register remarks of the ray caster's kernels (salva_amd/csrc/fluidcast.hip), checked without a GPU in the manner of
tests/test_field_resources.py.  The walk keeps a ray, its advanced origin, the slice's planes and cell ranges and the best hit per
lane and needs no LDS: none of its instances may use scratch or spill a register.  The remarks report, in VGPRs: k_fluid_cast
first hit 64, first hit + thickness 64, thickness only 60, k_fluid_cast_miss 7 - all at 8 waves per SIMD, no LDS - and for the two
counting instances behind salva_hip_count_ray_candidates, a measuring aid that carries one counter more, 66 (first-hit walk, 7 waves)
and 61 (thickness walk, 8 waves).  What is asserted is the occupancy step those counts fall in."""
import pytest

from test_kernel_resources import one, pytestmark, resources  # noqa: F401

# (template arguments <HIT, THICK, COUNT> as the mangled names spell them; COUNT: the instances of salva_hip_count_ray_candidates)
EIGHT_WAVES = ("k_fluid_castILb1ELb0ELb0EE", "k_fluid_castILb1ELb1ELb0EE", "k_fluid_castILb0ELb1ELb0EE", "k_fluid_castILb0ELb1ELb1EE",
               "k_fluid_cast_miss")
SEVEN_WAVES = ("k_fluid_castILb1ELb0ELb1EE",)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return resources("fluidcast.hip", tmp_path_factory.mktemp("fluidcast_resources"))


@pytest.mark.parametrize("kernel", EIGHT_WAVES)
def test_cast_kernel_has_no_scratch_and_eight_waves(table, kernel):
    r = one(table, kernel)
    print(kernel, r)
    assert r["scratch"] == 0 and r["spilled"] == 0, r
    assert r["vgprs"] <= 64 and r["waves"] >= 8, r


@pytest.mark.parametrize("kernel", SEVEN_WAVES)
def test_counting_first_hit_walk_has_no_scratch_and_seven_waves(table, kernel):
    r = one(table, kernel)
    print(kernel, r)
    assert r["scratch"] == 0 and r["spilled"] == 0, r
    assert r["vgprs"] <= 72 and r["waves"] >= 7, r


def test_every_kernel_of_the_file_is_listed(table):
    EVERY = EIGHT_WAVES + SEVEN_WAVES
    listed = {name: [f for f in EVERY if f in name] for name in table}
    assert all(len(f) == 1 for f in listed.values()), listed
    assert {f[0] for f in listed.values()} == set(EVERY) and len(table) == len(EVERY), sorted(table)

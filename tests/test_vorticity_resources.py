"""Register remarks of the vorticity confinement kernels (salva_amd/csrc/vorticity.hip), checked without a GPU in the
manner of tests/test_diffuse_resources.py.  Both kernels keep their sums in named scalars: no LDS beyond what Tile stages (the remarks'
static LDS is 0), no scratch.  The remarks report, in VGPRs: k_vorticity_curl 56, k_vorticity_confine 58 - both at 8 waves per SIMD.
What is asserted is the occupancy step those counts fall in: the one the build reports, not a target.  The second compilation
(-DSALVA_OTHER_KERNELS, namespace salva_ok: 63 and 61) is held to the same step."""
import pytest

from test_kernel_resources import CSRC, FLAGS, HIPCC, one, pytestmark, resources  # noqa: F401

EIGHT_WAVES = ("k_vorticity_curl", "k_vorticity_confine")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return resources("vorticity.hip", tmp_path_factory.mktemp("vorticity_resources"))


@pytest.fixture(scope="module")
def table_ok(tmp_path_factory):
    """the same source as the Makefile's OKSRCS rule compiles it"""
    import re
    import subprocess

    out = subprocess.run([HIPCC] + FLAGS + ["-DSALVA_OTHER_KERNELS", "vorticity.hip", "-o", str(tmp_path_factory.mktemp("vorticity_ok") / "v.o")],
                         cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    table = {}
    for block in re.split(r"remark: Function Name: ", out.stderr)[1:]:
        field = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
        table[block.split(" ")[0]] = {"vgprs": field("VGPRs"), "waves": field(r"Occupancy \[waves/SIMD\]"),
                                      "scratch": field(r"ScratchSize \[bytes/lane\]"), "spilled": field("VGPRs Spill"),
                                      "lds": field(r"LDS Size \[bytes/block\]")}
    return table


@pytest.mark.parametrize("kernel", EIGHT_WAVES)
def test_vorticity_kernel_has_no_scratch_and_eight_waves(table, kernel):
    r = one(table, kernel)
    print(kernel, r)
    assert r["scratch"] == 0 and r["spilled"] == 0, r
    assert r["vgprs"] <= 64 and r["waves"] >= 8, r


@pytest.mark.parametrize("kernel", EIGHT_WAVES)
def test_other_kernels_build_keeps_the_step_and_has_no_static_lds(table_ok, kernel):
    r = one(table_ok, kernel)
    print(kernel, r)
    assert r["scratch"] == 0 and r["spilled"] == 0 and r["lds"] == 0, r
    assert r["vgprs"] <= 64 and r["waves"] >= 8, r


def test_no_kernel_of_the_file_uses_scratch(table):
    for name, r in table.items():
        assert r["scratch"] == 0 and r["spilled"] == 0, (name, r)


def test_every_kernel_of_the_file_is_listed(table, table_ok):
    own = sorted(k for k in table if "k_vorticity" in k)
    assert len(own) == len(EIGHT_WAVES) == len(table), own
    assert all(k.startswith("_ZN5salva") for k in table), sorted(table)
    assert len(table_ok) == len(EIGHT_WAVES) and all(k.startswith("_ZN8salva_ok") for k in table_ok), sorted(table_ok)

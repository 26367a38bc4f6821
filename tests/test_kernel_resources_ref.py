"""Register budget of the list builder that keeps the referenced halo slots only (grid.hip k_nbr_tile_ref), checked without a GPU like
the kernels of test_kernel_resources.py.  It replaces k_nbr_tile<1, MM> in the steps whose halos are beyond a three-per-CU layout and
must keep that kernel's residency: four tiles per CU need 64 VGPRs (8 waves per SIMD).  The scratch budgets are the ones the project
already accepts for k_nbr_tile (16 bytes per lane and three spilled registers for one or two masses, 32 and six for three or four);
at the time of writing the builder uses 12 / 2, 12 / 2 and 24 / 6."""
import pytest

from test_kernel_resources import HIPCC, one, resources  # noqa: F401

pytestmark = __import__("test_kernel_resources").pytestmark


def test_the_referenced_halo_builder_keeps_four_tiles_per_cu(tmp_path):
    t = resources("grid.hip", tmp_path)
    for mm, scratch, spilled in ((0, 16, 3), (1, 16, 3), (2, 32, 6)):
        r = one(t, "k_nbr_tile_refILi%dE" % mm)
        assert r["vgprs"] <= 64 and r["waves"] >= 8 and r["scratch"] <= scratch and r["spilled"] <= spilled, (mm, r)

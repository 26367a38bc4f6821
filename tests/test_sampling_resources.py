"""Register budgets of the shape sampler's kernels (salva_amd/csrc/sample.hip), checked without a GPU in the manner of
tests/test_kernel_resources.py: the same flags, the same remark parsing.  The three kernels are short and stream through memory:
none may use scratch or spill a register.  The remarks report 14 (k_sample_mark), 4 (k_sample_count) and 20 (k_sample_emit) VGPRs,
all at 8 waves per SIMD; the ceiling is the next occupancy step, 64 VGPRs."""
from test_kernel_resources import one, pytestmark, resources  # noqa: F401


def test_sampler_kernels_have_no_scratch(tmp_path):
    t = resources("sample.hip", tmp_path)
    for fragment in ("k_sample_mark", "k_sample_count", "k_sample_emit"):
        r = one(t, fragment)
        assert r["scratch"] == 0 and r["spilled"] == 0, (fragment, r)
        assert r["vgprs"] <= 64 and r["waves"] >= 8, (fragment, r)

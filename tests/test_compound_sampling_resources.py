"""Register remarks of the compound's mark kernel (salva_amd/csrc/sample.hip k_compound_mark; DESIGN.md §17 "Ray sampling"), checked
without a GPU in the manner of tests/test_mesh_resources.py.  The kernel walks a parts table and, for mesh parts, a hierarchy, both
without a stack and without an indexed array of its own: it may not use scratch or spill a register.  The remarks report 52 VGPRs
and 8 waves per SIMD; what is asserted is the occupancy step that count falls in (at most 64 VGPRs, 8 waves), which is also its
siblings' (k_sample_mesh_mark: 44)."""
from test_kernel_resources import one, pytestmark, resources  # noqa: F401


def test_compound_mark_kernel_has_no_scratch(tmp_path):
    t = resources("sample.hip", tmp_path)
    r = one(t, "k_compound_mark")
    print("k_compound_mark", r)
    assert r["scratch"] == 0 and r["spilled"] == 0, r
    assert r["vgprs"] <= 64 and r["waves"] >= 8, r
    # the loop the two cast kernels share left the mesh kernel where it was
    m = one(t, "k_sample_mesh_mark")
    assert m["scratch"] == 0 and m["spilled"] == 0 and m["waves"] >= 8, m

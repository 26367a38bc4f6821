"""Register remarks of the compound kernels (salva_amd/csrc/dcs.hip k_dcs_compound_project and the two k_dcsb_segment kernels a batched
run with compounds goes through; world_query.hip k_compound_query, k_mesh_query), checked without a GPU in the manner of
tests/test_mesh_resources.py.  All of them walk a parts table and, for mesh parts, a hierarchy without a stack: none may use scratch or
spill a vector register.  The counts are printed; DESIGN.md §17 records them."""
from test_kernel_resources import one, pytestmark, resources  # noqa: F401


def test_compound_sampling_kernels_have_no_scratch(tmp_path):
    t = resources("dcs.hip", tmp_path)
    for fragment in ("k_dcs_compound_project", "k_dcsb_segmentILb0E", "k_dcsb_segmentILb1E"):
        r = one(t, fragment)
        print(fragment, r)
        assert r["scratch"] == 0 and r["spilled"] == 0, (fragment, r)
    # the compounds' own launch is where the walk's registers go: the batch's kernel keeps its five waves
    assert one(t, "k_dcsb_project")["waves"] >= 5 and one(t, "k_dcsb_segmentILb0E")["waves"] >= 5


def test_query_kernels_have_no_scratch(tmp_path):
    t = resources("world_query.hip", tmp_path)
    for fragment in ("k_compound_query", "k_mesh_query", "k_shape_query"):
        r = one(t, fragment)
        print(fragment, r)
        assert r["scratch"] == 0 and r["spilled"] == 0, (fragment, r)

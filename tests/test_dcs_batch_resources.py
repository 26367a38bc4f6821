"""Register budgets of the batched DynamicContactSampling kernels (salva_amd/csrc/dcs.hip k_dcsb_project / _push / _emit) and of the
batched pose and wrench kernels (world_coupling.hip), checked without a GPU in the manner of tests/test_mesh_resources.py.  k_dcsb_project
holds the mesh walk and the four analytic projections in one loop over the colliders: it may not use scratch or spill a vector
register.  The remarks report 85 VGPRs for it, 5 waves per SIMD; no ceiling beyond "no scratch" is set.  The kernels
the batch shares its device functions with must keep theirs: k_dcs_project 31, k_dcs_project_mesh 46."""
from test_kernel_resources import one, pytestmark, resources  # noqa: F401


def test_batched_kernels_have_no_scratch(tmp_path):
    t = resources("dcs.hip", tmp_path)
    for fragment in ("k_dcsb_project", "k_dcsb_push", "k_dcsb_emit"):
        r = one(t, fragment)
        print(fragment, r)
        assert r["scratch"] == 0 and r["spilled"] == 0, (fragment, r)
    # `k_dcs_project` is still the name of exactly one kernel, and neither it nor the mesh projection grew by the factoring
    r = one(t, "13k_dcs_projectE")
    assert r["vgprs"] <= 31 and r["scratch"] == 0 and r["spilled"] == 0, r
    r = one(t, "k_dcs_project_mesh")
    assert r["vgprs"] <= 46 and r["scratch"] == 0 and r["spilled"] == 0, r


def test_batched_pose_and_wrench_kernels_have_no_scratch(tmp_path):
    t = resources("world_coupling.hip", tmp_path)
    for fragment in ("k_boundary_posesE", "k_boundary_wrenchesE"):
        r = one(t, fragment)
        print(fragment, r)
        assert r["scratch"] == 0 and r["spilled"] == 0, (fragment, r)

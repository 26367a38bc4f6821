"""Register budgets of the two mesh kernels (salva_amd/csrc/sample.hip k_sample_mesh_mark, dcs.hip k_dcs_project_mesh), checked
without a GPU in the manner of tests/test_kernel_resources.py.  Both walk the hierarchy without a stack: neither may use scratch or
spill a register.  The remarks report 44 and 46 VGPRs; no ceiling beyond "no scratch" is set."""
from test_kernel_resources import one, pytestmark, resources  # noqa: F401


def test_mesh_kernels_have_no_scratch(tmp_path):
    for source, fragment in (("sample.hip", "k_sample_mesh_mark"), ("dcs.hip", "k_dcs_project_mesh")):
        r = one(resources(source, tmp_path), fragment)
        print(fragment, r)
        assert r["scratch"] == 0 and r["spilled"] == 0, (fragment, r)

"""Register budget of the contact-table kernel of device forces (salva_amd/csrc/userforce.hip k_contact_tables), checked without a
GPU in the manner of tests/test_dcs_batch_resources.py: neither instantiation (indices only / indices + kernel values) may use scratch
or spill a vector register.  DESIGN.md §16 quotes the counts the remarks report; no ceiling beyond "no scratch" is set here."""
from test_kernel_resources import one, pytestmark, resources  # noqa: F401


def test_contact_table_kernels_have_no_scratch(tmp_path):
    t = resources("userforce.hip", tmp_path)
    for fragment in ("k_contact_tablesILb0E", "k_contact_tablesILb1E", "k_widen_counts"):
        r = one(t, fragment)
        print(fragment, r)
        assert r["scratch"] == 0 and r["spilled"] == 0, (fragment, r)

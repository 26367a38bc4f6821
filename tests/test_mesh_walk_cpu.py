"""The stackless hierarchy walks of salva_amd/csrc/mesh.h give what a pass over all triangles gives, bit for bit —
checked without a GPU: the walks are `__host__ __device__`, tests/mesh_walk_check.hip is a stand-alone host program around them and
around the library's own hierarchy builder."""
import os
import re
import subprocess

from test_kernel_resources import CSRC, HIPCC, pytestmark  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))


def test_hierarchy_walks_equal_brute_force(hip_lib, tmp_path):
    exe = str(tmp_path / "mesh_walk_check")
    build = subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "mesh_walk_check.hip"),
                            "-o", exe, "-L" + CSRC, "-lsalva_hip", "-Wl,-rpath," + CSRC], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    m = re.search(r"deepest hierarchy: (\d+) levels; differences: (\d+)", run.stdout)
    assert run.returncode == 0 and m and int(m.group(2)) == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert int(m.group(1)) >= 10

"""The device queries share one staging buffer for the results of host buffers: every family's query made back to
back on one world, all into host memory and in sizes that go up and down, returns bit for bit what the same call returns as the
first query of a freshly built twin world.  Only the public Python interface is used."""
import numpy as np
import pytest

import diffuse_reading as dr
import field_child as fc
from salva_amd import Anisotropy

pytestmark = pytest.mark.gpu
ALL = dict(density=True, fraction=True, velocity=True, gradient=True, count=True)


@pytest.fixture(scope="module")
def case():
    """the families' standard cloud (1 386 particles in two fluids, with a flow) and the places of the queries"""
    c = dict(dr.standard_cloud())
    h = c["h"]
    lo, hi = c["x"].min(axis=0), c["x"].max(axis=0)
    u, v = np.meshgrid(np.linspace(lo[0], hi[0], 6), np.linspace(lo[1], hi[1], 6), indexing="ij")
    c["ray_origins"] = np.stack([u.ravel(), v.ravel(), np.full(36, lo[2] - 2.0 * h)], axis=1).astype(np.float32)
    c["ray_directions"] = np.tile(np.array([0.05, -0.03, 1.0], np.float32), (36, 1))
    c["few"] = c["points"][:1000]
    c["coarse"] = (c["origin"], 2.0 * float(c["spacing"]), tuple((int(d) + 1) // 2 for d in c["dims"]))
    c["seeds"] = c["x"][:10] + np.float32(0.3 * c["r"])
    return c


def diffuse_get(w, c):
    s = w.create_diffuse(64)
    s.add(c["seeds"], c["v"][:10], lifetimes=1.5)
    return s.get()


# the calls, in the order the one world makes them: a large staging size, a small one, the four outputs of a mesh, ...
CALLS = [
    ("evaluate_fields", lambda w, c: w.evaluate_fields(c["few"], **ALL)),
    ("cast_rays", lambda w, c: w.cast_rays(c["ray_origins"], c["ray_directions"], normals=True, thickness=True)),
    ("extract_surface", lambda w, c: w.extract_surface(*c["coarse"], normals=True, velocities=True)),
    ("extract_surface_anisotropic", lambda w, c: w.extract_surface(*c["coarse"], normals=True, velocities=True, anisotropy=Anisotropy())),
    ("anisotropy", lambda w, c: w.anisotropy()),
    ("diffuse_potentials", lambda w, c: w.diffuse_potentials()),
    ("diffuse_get", diffuse_get),
    ("evaluate_lattice_anisotropic", lambda w, c: w.evaluate_lattice(*c["coarse"], gradient=True, fraction=True, anisotropy=Anisotropy())),
    ("evaluate_fields_again", lambda w, c: w.evaluate_fields(c["few"], **ALL)),
]


def same(a, b):
    """array for array and bit for bit (NaN payloads and the sign of zero included)"""
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)), k


def test_back_to_back_queries_equal_the_first_query_of_a_twin_world(hip_lib, case):
    w, _ = fc.standard_world(case)
    got = [(name, call(w, case)) for name, call in CALLS]
    for name, result in got:
        assert all(a.size for a in result.values()), name  # (every call has something to stage)
    assert np.isfinite(got[1][1]["t"]).sum() > 18  # (the rays do meet the fluid)
    same(got[0][1], got[-1][1])
    for (name, result), (_, call) in zip(got, CALLS):
        twin, _ = fc.standard_world(case)
        print(name, {k: a.shape for k, a in result.items()})
        same(result, call(twin, case))

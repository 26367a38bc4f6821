"""What the five operations on a geometry refuse, for each of the three forms a geometry takes: the code, the whole
message and — where a call is wrong in two ways — which refusal wins.  The operations are sampling to the host, adding sampled
particles to a fluid, sampling a static boundary, registering a dynamically sampled boundary and the shape query; the forms are a
built-in SalvaHipShape, a mesh handle and a compound handle.  Every message below was read from the source of the library as it
was before the fifteen methods behind these entries became five; the rows that no other test makes are here, with the whole text
(the other tests look at codes and at words of a message).

One world of one fluid of 4^3 particles and one boundary of a 4 x 4 plate.  No case steps it and no case changes it: every call is
refused.  The calls from inside a force callback need a step, of a second world of the same size."""
import ctypes as C

import numpy as np
import pytest

import mesh_fixtures as X
from salva_amd import Boundary, DFSPHSolver, Fluid, LiquidWorld, NonPressureForce, _lib, sampling, scenes

pytestmark = pytest.mark.gpu

F = np.float32
RAD = 0.025
NAN = float("nan")
OPS = ("sample", "add_sampled", "boundary_from", "dynamic", "query")
FORMS = ("shape", "mesh", "compound")
ENTRY = {
    "sample": ("salva_hip_sample_shape", "salva_hip_sample_mesh", "salva_hip_sample_compound"),
    "add_sampled": ("salva_hip_add_particles_sampled", "salva_hip_add_particles_sampled_mesh", "salva_hip_add_particles_sampled_compound"),
    "boundary_from": ("salva_hip_set_boundary_sampling_from_shape", "salva_hip_set_boundary_sampling_from_mesh",
                      "salva_hip_set_boundary_sampling_from_compound"),
    "dynamic": ("salva_hip_set_boundary_dynamic_sampling", "salva_hip_set_boundary_dynamic_sampling_mesh",
                "salva_hip_set_boundary_dynamic_sampling_compound"),
    "query": ("salva_hip_particles_intersecting_shape", "salva_hip_particles_intersecting_mesh", "salva_hip_particles_intersecting_compound"),
}

UNKNOWN_KIND = ("unknown shape kind (ball, cuboid, capsule (y) and cylinder (y) are built in; other parry shapes belong to the host)")
NO_SUCH = {"mesh": "no such mesh", "compound": "no such compound"}
BAD_MODE = "unknown sampling mode (SALVA_HIP_SAMPLE_SURFACE / SALVA_HIP_SAMPLE_VOLUME)"
BAD_RADIUS = "the particle radius must be positive"
BAD_PARAMS = {op: "shape parameters must be positive" for op in OPS}
BAD_PARAMS["query"] = "shape query: radius / half extents must be positive and finite"
FLUID_SLOT = "fluid slot out of range"
BOUNDARY_SLOT = "boundary slot out of range (slots are dense)"
NOT_SOLID = {
    "mesh": "shape query: a mesh without SALVA_HIP_MESH_ORIENTED has no solid distance (use salva_hip_particles_intersecting_host_shape)",
    "compound": "shape query: a mesh part of the compound lacks SALVA_HIP_MESH_ORIENTED and has no solid distance "
                "(use salva_hip_particles_intersecting_host_shape)",
}
IN_FORCE_CALLBACK = "this entry point is not available inside a force callback"


def shape_of(kind=_lib.SHAPE_BALL, params=(0.1, 0.1, 0.1)):
    s = _lib.Shape()
    s.kind = kind
    s.params[:] = params
    return s


def compound_of(w, mesh=None):
    part = _lib.CompoundPart()
    part.kind, part.mesh = (_lib.SHAPE_BALL, 0) if mesh is None else (_lib.SHAPE_MESH, mesh)
    part.params[:] = (0.1, 0.1, 0.1)
    part.rotation_ijkw[:] = (0, 0, 0, 1)
    h = C.c_uint32()
    _lib.check(w._L.salva_hip_create_compound(w._h, (_lib.CompoundPart * 1)(part), 1, C.byref(h)))
    return h.value


def small_world():
    w = LiquidWorld(DFSPHSolver(), RAD, 2.0)
    f = Fluid(scenes.cube_fluid_positions(4, 4, 4, RAD), RAD, 1000.0)
    w.add_fluid(f)
    plate = np.array([[2 * RAD * i, -4 * RAD, 2 * RAD * k] for i in range(4) for k in range(4)], F)
    w.add_boundary(Boundary(plate))
    return w, f


class Geometries:
    """The good and the bad geometries of one world, by form."""

    def __init__(self, w):
        v, t, _ = X.tetrahedron()
        oriented, surface, gone = (sampling.Mesh(v, t, oriented=o).handle(w) for o in (True, False, True))
        self.good = {"shape": shape_of(), "mesh": oriented, "compound": compound_of(w)}
        self.unknown = {"mesh": 9999, "compound": 9999}
        self.not_solid = {"mesh": surface, "compound": compound_of(w, surface)}
        self.destroyed = {"mesh": gone, "compound": compound_of(w)}  # (destroyed last: a free entry of the table may be handed out again)
        _lib.check(w._L.salva_hip_destroy_mesh(w._h, gone))
        _lib.check(w._L.salva_hip_destroy_compound(w._h, self.destroyed["compound"]))


@pytest.fixture(scope="module")
def world(hip_lib):
    w, _ = small_world()
    w.sync_to_device()
    return w, Geometries(w)


def call(w, op, form, geom, t=(0, 0, 0), q=(0, 0, 0, 1), fluid=0, boundary=1, rad=RAD, mode=0):
    """One entry of the family on `geom` (a Shape, or a handle) -> (code, message); a count >= 0 comes back as it is."""
    entry = getattr(w._L, ENTRY[op][FORMS.index(form)])
    g = C.byref(geom) if form == "shape" else geom
    t, q = (C.c_float * 3)(*t), (C.c_float * 4)(*q)
    if op == "sample":
        rc = entry(w._h, g, rad, mode, 0, None)
    elif op == "add_sampled":
        rc = entry(w._h, fluid, g, t, q, mode, None)
    elif op == "query":
        rc = entry(w._h, t, q, g, 0, None, None, None)
    else:
        rc = entry(w._h, boundary, g, 1, 0xFFFFFFFF)
    return int(rc), w._L.salva_hip_last_error().decode()


def refused(w, message, *args, **kwargs):
    assert call(w, *args, **kwargs) == (_lib.E_INVALID, message)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("op", OPS)
def test_refusals(world, op, form):
    w, G = world
    good = G.good[form]
    handle = form != "shape"
    unchanged = (w._L.salva_hip_fluid_len(w._h, 0), w._L.salva_hip_num_boundaries(w._h))

    # ---- the pose, where the operation takes one
    if op == "query":
        refused(w, "shape query: non-finite translation", op, form, good, t=(0, NAN, 0))
        refused(w, "shape query: non-finite translation", op, form, good, t=(float("inf"), 0, 0))
        refused(w, "shape query: non-finite rotation", op, form, good, q=(0, NAN, 0, 1))
        refused(w, "shape query: the rotation must be a unit quaternion (x, y, z, w)", op, form, good, q=(0, 0, 0, 1.01))
        refused(w, "shape query: the rotation must be a unit quaternion (x, y, z, w)", op, form, good, q=(0, 0, 0, 0))
    if op == "add_sampled":  # (any finite quaternion is taken as it is)
        refused(w, "non-finite pose", op, form, good, t=(0, NAN, 0))
        refused(w, "non-finite pose", op, form, good, q=(0, NAN, 0, 1))

    # ---- the geometry itself
    if handle:
        refused(w, NO_SUCH[form], op, form, G.unknown[form])
        refused(w, NO_SUCH[form], op, form, G.destroyed[form])
        if op == "query":
            refused(w, NOT_SOLID[form], op, form, G.not_solid[form])
            refused(w, NOT_SOLID[form], op, form, G.not_solid[form], t=(0, NAN, 0))  # (before the pose)
    else:
        for kind in (0, 99, _lib.SHAPE_MESH, _lib.SHAPE_COMPOUND, 100):  # (a handle's kind in a SalvaHipShape is no shape)
            refused(w, UNKNOWN_KIND, op, form, shape_of(kind=kind))
        for params in ((0.0, 0.1, 0.1), (-1.0, 0.1, 0.1), (NAN, 0.1, 0.1)):
            refused(w, BAD_PARAMS[op], op, form, shape_of(params=params))
        refused(w, BAD_PARAMS[op], op, form, shape_of(_lib.SHAPE_CUBOID, (0.1, 0.1, 0.0)))
        refused(w, BAD_PARAMS[op], op, form, shape_of(_lib.SHAPE_CAPSULE, (0.1, float("inf"), 0.0)))

    # ---- the slot
    if op == "add_sampled":
        refused(w, FLUID_SLOT, op, form, good, fluid=1)
        refused(w, FLUID_SLOT, op, form, good, fluid=0xFFFFFFFF)
    if op in ("boundary_from", "dynamic"):
        refused(w, BOUNDARY_SLOT, op, form, good, boundary=3)

    # ---- the sampler's own arguments
    if op == "sample":
        for rad in (0.0, -RAD, NAN, float("inf")):
            refused(w, BAD_RADIUS, op, form, good, rad=rad)
    if op in ("sample", "add_sampled"):
        for mode in (2, -1):
            refused(w, BAD_MODE, op, form, good, mode=mode)

    # ---- two things wrong at once: which refusal wins
    bad = G.unknown[form] if handle else shape_of(kind=99)
    bad_message = NO_SUCH[form] if handle else UNKNOWN_KIND
    if op == "query":  # an unknown kind, or an unknown handle, before a bad pose; a shape's parameters after it
        refused(w, bad_message, op, form, bad, t=(0, NAN, 0))
        refused(w, bad_message, op, form, bad, q=(0, 0, 0, 2))
        if not handle:
            refused(w, "shape query: non-finite translation", op, form, shape_of(params=(0.0, 0.1, 0.1)), t=(0, NAN, 0))
    if op == "sample":  # a handle is looked up before the sampler's arguments are checked, a shape after
        refused(w, NO_SUCH[form] if handle else BAD_MODE, op, form, bad, mode=2)
        refused(w, NO_SUCH[form] if handle else BAD_RADIUS, op, form, bad, rad=0.0)
        refused(w, BAD_RADIUS, op, form, good, rad=0.0, mode=2)
    if op == "add_sampled":  # the slot, the pose, then the handle; the mode before a shape, after a handle
        refused(w, FLUID_SLOT, op, form, bad, fluid=1, t=(0, NAN, 0))
        refused(w, "non-finite pose", op, form, bad, t=(0, NAN, 0))
        refused(w, NO_SUCH[form] if handle else BAD_MODE, op, form, bad, mode=2)
    if op == "boundary_from":  # the slot before the geometry
        refused(w, BOUNDARY_SLOT, op, form, bad, boundary=3)
    if op == "dynamic":  # the geometry before the slot
        refused(w, bad_message, op, form, bad, boundary=3)

    assert (w._L.salva_hip_fluid_len(w._h, 0), w._L.salva_hip_num_boundaries(w._h)) == unchanged


# ---------------------------------------------------------------------------------------------- regions share the two checks
def region_of(kind, handle=0, shape=None, t=(0, 0, 0), q=(0, 0, 0, 1)):
    r = _lib.Region()
    r.struct_size, r.version, r.kind, r.handle = _lib.REGION_BYTES, _lib.REGION_VERSION, kind, handle
    if shape is not None:
        r.shape = shape
    r.translation[:] = t
    r.rotation_ijkw[:] = q
    return r


REGION_KIND = {"shape": _lib.REGION_SHAPE, "mesh": _lib.REGION_MESH, "compound": _lib.REGION_COMPOUND}


@pytest.mark.parametrize("form", FORMS)
def test_region_refusals(world, form):
    """A region resolves its geometry like the shape query: the same order, `region:` in front, no hint behind."""
    w, G = world
    handle = form != "shape"

    def refused_region(message, geom, **pose):
        r = region_of(REGION_KIND[form], handle=geom if handle else 0, shape=None if handle else geom, **pose)
        sink = C.c_uint32()
        for rc in (w._L.salva_hip_delete_particles_in_region(w._h, C.byref(r), 0, None), w._L.salva_hip_add_sink(w._h, C.byref(r), 0, C.byref(sink))):
            assert (int(rc), w._L.salva_hip_last_error().decode()) == (_lib.E_INVALID, message)

    good = G.good[form]
    refused_region("region: non-finite translation", good, t=(0, NAN, 0))
    refused_region("region: non-finite rotation", good, q=(0, NAN, 0, 1))
    refused_region("region: the rotation must be a unit quaternion (x, y, z, w)", good, q=(0, 0, 0, 2))
    if handle:
        refused_region(NO_SUCH[form], G.unknown[form])
        refused_region(NO_SUCH[form], G.destroyed[form], t=(0, NAN, 0))
        not_solid = NOT_SOLID[form].replace("shape query:", "region:").replace(" (use salva_hip_particles_intersecting_host_shape)", "")
        refused_region(not_solid, G.not_solid[form])
        refused_region(not_solid, G.not_solid[form], q=(0, 0, 0, 2))
    else:
        refused_region(UNKNOWN_KIND, shape_of(kind=99), t=(0, NAN, 0))
        refused_region("region: non-finite translation", shape_of(params=(0.0, 0.1, 0.1)), t=(0, NAN, 0))
        refused_region("region: radius / half extents must be positive and finite", shape_of(params=(0.0, 0.1, 0.1)))
    assert w._L.salva_hip_fluid_len(w._h, 0) == 64


# ---------------------------------------------------------------------------------------------- inside a force callback
class CallsEveryEntry(NonPressureForce):
    """Every entry of the family with an unknown kind / an unknown handle: an entry that is refused inside a force callback says so,
    one that is not gets as far as looking at its geometry."""

    def solve(self, timestep, kernel_radius, ff, fb, fluid, boundaries, densities):
        bad = {"shape": shape_of(kind=99), "mesh": 9999, "compound": 9999}
        self.seen = {(op, form): call(self.world, op, form, bad[form]) for op in OPS for form in FORMS}


def test_inside_a_force_callback(hip_lib):
    """All fifteen entries are refused inside a force callback but one: salva_hip_particles_intersecting_shape is not."""
    w, f = small_world()
    force = CallsEveryEntry()
    force.world = w
    f.nonpressure_forces.append(force)
    w.step(1.0 / 240.0, (0.0, -9.81, 0.0))
    want = {(op, form): (_lib.E_INVALID, IN_FORCE_CALLBACK) for op in OPS for form in FORMS}
    want[("query", "shape")] = (_lib.E_INVALID, UNKNOWN_KIND)
    assert force.seen == want
    assert f.num_particles() == 64 and w._L.salva_hip_num_boundaries(w._h) == 1

"""Shared by test_dcs_cloud_cpu.py and test_dcs_cloud_gpu.py: clouds of fluid particles that fill EVERY projection branch of the
four shapes of ColliderSampling::DynamicContactSampling (fluids_pipeline.rs:193-259; dcs.hip / the oracle's update_boundaries_dynamic).

* `Collider` / `COLLIDERS`: the five posed shapes (ball, cuboid, capsule, a tall and a flat cylinder) on moving bodies.
* `cloud(colliders)`: a jittered lattice at spacing 2 R around them, with velocities of up to 4 m/s per axis, so that with a previous
  substep of DT_PREV the prediction x + v dt carries points across the borders between the regions.
* `classify(collider, points)`: an f64 numpy reading of the geometry that names the branch every point falls in and gives its
  nearest surface point.  It is written from the shapes themselves (distances to faces, caps, axis) and shares no text with
  dcs.hip or the oracle; it is the arbiter when two f32 readings disagree.
* `capsule_callbacks` / `cylinder_callbacks`: f32 numpy `aabb` / `project` callbacks for HostShapeSampling, operation by operation
  after the parry description quoted at the top of dcs.hip — a third reading of the two shapes next to the device's and the oracle's.
* `run_oracle` / `HipWorld`: one world per side with a probe force as its only force, and everything the arm produces.
* `DEGENERATE`: exact points on the borders between branches (dyadic coordinates, identity rotation).
"""
from dataclasses import dataclass, field

import numpy as np

from salva_amd import scenes
from salva_amd.coupling import RigidBody
from test_host_shape_gpu import ball_callbacks, cuboid_callbacks, to_local, to_world

F = np.float32
R = 0.025
H = 4 * R            # particle radius * smoothing factor 2 * 2 (liquid_world.rs:44)
REACH = 1.5 * H      # h + prediction
DT_PREV = 0.004
VMAX = 4.0
EPS = float(np.finfo(np.float32).eps)
KIND = {"ball": 1, "cuboid": 2, "capsule": 3, "cylinder": 4}


@dataclass
class Collider:
    name: str
    shape: tuple            # what salva_amd.coupling.make_shape takes
    body: RigidBody = field(default=None)

    @property
    def kind(self):
        return self.shape[0]

    @property
    def params(self):
        return [float(x) for x in (self.shape[1] if self.kind == "cuboid" else self.shape[1:])]


def _body(t, axis, linvel, angvel, com):
    # kinematic: the wrench on a dynamic body is an atomically accumulated sum whose last bit varies from run to run
    return RigidBody(translation=F(t), rotation=scenes.quat_from_scaled_axis(axis), linvel=F(linvel), angvel=F(angvel), local_com=F(com),
                     dynamic=False)


def collider(name):
    """A fresh copy (the bodies are integrated by some tests)."""
    return {
        "ball": lambda: Collider(name, ("ball", 0.17), _body([0.05, -0.02, 0.03], (0.3, -0.2, 0.5), [0.2, -0.1, 0.3], [1.0, 2.0, -0.5], [0.06, -0.02, 0.02])),
        # three clearly different half extents; the thinnest still holds two lattice layers per side
        "cuboid": lambda: Collider(name, ("cuboid", (0.22, 0.12, 0.17)), _body([-0.03, 0.04, 0.02], (0.3, -0.2, 0.5), [0.3, 0.2, -0.1], [-0.5, 1.0, 2.0], [0.02, 0.01, -0.03])),
        # half height > radius: barrel and hemispheres are both populated
        "capsule": lambda: Collider(name, ("capsule", 0.16, 0.11), _body([0.02, 0.03, -0.04], (-0.4, 0.3, 0.25), [-0.2, 0.3, 0.1], [2.0, -1.0, 0.5], [0.0, 0.03, 0.01])),
        # tall: the inner side region dominates; flat: the caps do
        "tall_cylinder": lambda: Collider(name, ("cylinder", 0.22, 0.12), _body([0.04, -0.03, 0.01], (0.3, -0.2, 0.5), [0.1, 0.3, -0.2], [1.0, -0.5, 2.0], [0.01, -0.04, 0.0])),
        "flat_cylinder": lambda: Collider(name, ("cylinder", 0.09, 0.21), _body([-0.02, 0.01, 0.05], (0.25, 0.4, -0.3), [-0.3, 0.1, 0.2], [0.5, 2.0, 1.0], [0.03, 0.0, -0.02])),
    }[name]()


COLLIDERS = ("ball", "cuboid", "capsule", "tall_cylinder", "flat_cylinder")


def overlapping_pair():
    """The cuboid and a capsule that sticks out of it: a particle the first collider of a pass pushes out may land inside the second."""
    a, b = collider("cuboid"), collider("capsule")
    b.body.translation = (a.body.translation + F([0.16, 0.10, 0.06])).astype(F)
    return [a, b]


# ------------------------------------------------------------------------------------------------ f64 geometry
def rotation_matrix(q):
    """The rotation of the unit quaternion (i, j, k, w) as a matrix, from Rodrigues' formula on its axis and angle."""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q)
    s = np.linalg.norm(q[:3])
    if s < 1e-300:
        return np.eye(3)
    n = q[:3] / s
    ang = 2.0 * np.arctan2(s, q[3])
    K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1.0 - np.cos(ang)) * (K @ K)


def half_extent(c):
    """Half extents of the posed shape's axis-aligned box about the body's translation."""
    M = np.abs(rotation_matrix(c.body.rotation))
    p = c.params
    if c.kind == "ball":
        return np.full(3, p[0])
    if c.kind == "cuboid":
        return M @ np.array(p)
    if c.kind == "capsule":   # a segment of half length hh along the local y axis, fattened by the radius
        return M[:, 1] * p[0] + p[1]
    return M @ np.array([p[1], p[0], p[1]])


def local_points(c, pts):
    return (np.asarray(pts, np.float64) - c.body.translation.astype(np.float64)) @ rotation_matrix(c.body.rotation)


def world_points(c, loc):
    return loc @ rotation_matrix(c.body.rotation).T + c.body.translation.astype(np.float64)


BRANCHES = {
    "ball": ["inside", "outside"],
    "cuboid": [f"inside, nearest face {s}{a}" for a in "xyz" for s in "-+"] + [f"outside, beyond face {s}{a}" for a in "xyz" for s in "-+"]
              + ["outside, edge region", "outside, corner region"],
    "capsule": [f"{w}, closest segment point {e}" for w in ("inside", "outside") for e in ("end a", "end b", "interior")],
    "cylinder": ["inside, nearest top", "inside, nearest bottom", "inside, nearest side", "outside, above within the radius",
                 "outside, above beyond the radius", "outside, below within the radius", "outside, below beyond the radius", "outside, beside"],
}


def classify(c, pts):
    """(labels, inside, nearest surface point in world space) of world points, in f64."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return _classify(c, local_points(c, pts))


def _classify(c, l):
    n = len(l)
    p = c.params
    labels = np.empty(n, dtype=object)
    if c.kind == "ball":
        d = np.linalg.norm(l, axis=1)
        inside = d <= p[0]
        near = l * (p[0] / d)[:, None]
        labels[:] = np.where(inside, "inside", "outside")
    elif c.kind == "cuboid":
        he = np.array(p)
        over = np.abs(l) - he            # signed distance to each pair of faces, positive beyond them
        inside = (over <= 0).all(1)
        near = np.clip(l, -he, he)
        ax = over.argmax(1)              # inside: the face whose plane is closest
        sign = np.where(l >= 0, 1.0, -1.0)
        for k in range(n):
            if inside[k]:
                a = ax[k]
                near[k, a] = sign[k, a] * he[a]
                labels[k] = f"inside, nearest face {'+' if sign[k, a] > 0 else '-'}{'xyz'[a]}"
            else:
                beyond = np.nonzero(over[k] > 0)[0]
                if len(beyond) == 1:
                    a = beyond[0]
                    labels[k] = f"outside, beyond face {'+' if sign[k, a] > 0 else '-'}{'xyz'[a]}"
                else:
                    labels[k] = "outside, edge region" if len(beyond) == 2 else "outside, corner region"
    elif c.kind == "capsule":
        hh, r = p
        seg = np.zeros_like(l)
        seg[:, 1] = np.clip(l[:, 1], -hh, hh)
        d = np.linalg.norm(l - seg, axis=1)
        inside = d <= r
        near = seg + (l - seg) * (r / d)[:, None]
        end = np.where(l[:, 1] <= -hh, "end a", np.where(l[:, 1] >= hh, "end b", "interior"))
        for k in range(n):
            labels[k] = f"{'inside' if inside[k] else 'outside'}, closest segment point {end[k]}"
    else:
        hh, r = p
        y, rho = l[:, 1], np.hypot(l[:, 0], l[:, 2])
        inside = (np.abs(y) <= hh) & (rho <= r)
        rim = l[:, [0, 2]] * (r / rho)[:, None]   # the point of the circle of radius r under (or over) the point
        near = l.copy()
        for k in range(n):
            if inside[k]:
                dist = {"side": r - rho[k], "top": hh - y[k], "bottom": y[k] + hh}
                which = min(dist, key=dist.get)   # (ties: the first listed, the side)
                labels[k] = f"inside, nearest {which}"
                if which == "side":
                    near[k, 0], near[k, 2] = rim[k]
                else:
                    near[k, 1] = hh if which == "top" else -hh
            else:
                near[k, 1] = min(max(y[k], -hh), hh)
                if rho[k] > r:
                    near[k, 0], near[k, 2] = rim[k]
                if abs(y[k]) > hh:
                    labels[k] = f"outside, {'above' if y[k] > 0 else 'below'} {'within' if rho[k] <= r else 'beyond'} the radius"
                else:
                    labels[k] = "outside, beside"
    return labels, inside, world_points(c, near)


# ------------------------------------------------------------------------------------------------ the cloud
def cloud(colliders, seed=11):
    """(positions, velocities): a jittered 2 R lattice over the box that holds every posed shape and 1.5 h + 0.05 beyond it."""
    lo = np.min([c.body.translation - half_extent(c) for c in colliders], axis=0) - (REACH + 0.05)
    hi = np.max([c.body.translation + half_extent(c) for c in colliders], axis=0) + (REACH + 0.05)
    amp = 0.2 * R
    # cube_fluid_positions puts the outermost centres at -+(n - 1) R about its centre
    n = [int(np.ceil((hi[a] - lo[a] + 2 * amp) / (2 * R))) + 1 for a in range(3)]
    pos = scenes.jitter(scenes.cube_fluid_positions(n[0], n[1], n[2], R), amp, seed=seed) + F((lo + hi) / 2)
    assert (pos.min(0) <= lo).all() and (pos.max(0) >= hi).all()
    return pos.astype(F), scenes.random_velocities(len(pos), VMAX, seed=seed + 1)


def slab_cloud(colliders, half_width=0.3):
    """(positions, velocities, long axis): the cloud cut down to a bar — its full length along the axis on which the first shape's box
    is widest, `half_width` about the shapes' centre on the two others.  Wrapped onto a torus of 8 cells the full cloud piles onto itself
    along all three axes (a tile's halo then holds more than twice the particles of the lattice at rest, beyond what a tile kernel
    stages); the bar overlaps itself along its length only, by a cell or two."""
    pos, vel = cloud(colliders)
    long_axis = int(np.argmax(half_extent(colliders[0])))
    centre = np.mean([c.body.translation for c in colliders], axis=0)
    half = np.full(3, half_width)
    half[long_axis] = np.inf
    keep = (np.abs(pos - centre) <= half).all(1)
    return pos[keep], vel[keep], long_axis


def fold_periods(err):
    """The fold periods (cells per axis, 0 = not folded) of every pass in the SALVA_HIP_TILE_TRACE lines of a captured stderr."""
    import re

    return [tuple(int(x) for x in m.groups()) for m in re.finditer(r"\| fold (\d+) (\d+) (\d+)", err)]


def predicted(pos, vel, dt=DT_PREV):
    """x + v dt as both sides compute it (fluids_pipeline.rs:206-207): f32, the product rounded before the sum."""
    return (pos + (vel * F(dt)).astype(F)).astype(F)


def box_tests(c, pos, pred):
    """f64: which particles' grid cell lies in the cell range of the loosened box, and which predictions lie in that box."""
    t, ext = c.body.translation.astype(np.float64), half_extent(c)
    lo, hi = t - ext - REACH, t + ext + REACH
    cell = np.floor(pos.astype(np.float64) / np.float64(F(H)))
    in_cells = ((cell >= np.floor(lo / H)) & (cell <= np.floor(hi / H))).all(1)
    p = pred.astype(np.float64)
    return in_cells, ((p >= lo) & (p <= hi)).all(1)


# ------------------------------------------------------------------------------------------------ the third reading
def capsule_callbacks(body, hh, r):
    """parry Capsule::new_y(hh, r): the segment a = (0, -hh, 0), b = (0, hh, 0) and a radius."""
    hh, r = F(hh), F(r)
    a, b = np.array([[F(0), -hh, F(0)]], F), np.array([[F(0), hh, F(0)]], F)

    def aabb():
        # Capsule::aabb(pos) = [inf(A, B) - r, sup(A, B) + r] with A, B the posed segment ends
        A, B = to_world(body, a)[0], to_world(body, b)[0]
        return (np.minimum(A, B) - r).astype(F), (np.maximum(A, B) + r).astype(F)

    def project(pts):
        l = to_local(body, pts)
        ab = (b - a)[0]
        ap = (l - a).astype(F)
        ab_ap = ((ab[0] * ap[:, 0] + ab[1] * ap[:, 1]) + ab[2] * ap[:, 2]).astype(F)
        sqn = F((ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2])
        s = (a + ab[None, :] * (ab_ap / sqn)[:, None]).astype(F)
        s[ab_ap <= 0] = a[0]
        s[ab_ap >= sqn] = b[0]
        d = (l - s).astype(F)
        sq = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)
        dist = np.sqrt(sq)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = (s + (d / dist[:, None]).astype(F) * r).astype(F)
        inside = dist <= r
        on = ~(sq > F(EPS) * F(EPS))   # try_new_and_get(p - s, eps) fails: the point is on the segment
        out[on] = (s[on] + np.array([F(1), F(0), F(0)], F) * r).astype(F)
        inside[on] = True
        return to_world(body, out), inside

    return aabb, project


def cylinder_callbacks(body, hh, r):
    """parry Cylinder(hh, r), axis = local y."""
    hh, r = F(hh), F(r)

    # Cylinder::aabb(pos) = t -+ |R| (r, hh, r): the cuboid's box with the half extents of the cylinder's local box
    aabb = cuboid_callbacks(body, (r, hh, r))[0]

    def project(pts):
        l = to_local(body, pts)
        x, y, z = l[:, 0], l[:, 1], l[:, 2]
        planar = np.sqrt(x * x + z * z).astype(F)
        with np.errstate(divide="ignore", invalid="ignore"):
            ux, uz = (x / planar).astype(F), (z / planar).astype(F)
        ux[planar <= F(EPS)], uz[planar <= F(EPS)] = F(1), F(0)
        cx, cz = (ux * r).astype(F), (uz * r).astype(F)       # the plane point carried to the circle
        inside = (y >= -hh) & (y <= hh) & (planar <= r)
        top, bottom, side = (hh - y).astype(F), (y + hh).astype(F), (r - planar).astype(F)
        to_top, to_bottom = inside & (top < bottom) & (top < side), inside & (bottom < top) & (bottom < side)
        to_side = inside & ~to_top & ~to_bottom
        # outside: the height clamped to the caps, the plane point to the circle
        oy = np.where(y > hh, hh, np.where(y < -hh, -hh, y)).astype(F)
        beside = ~inside & (oy == y)
        on_circle = to_side | beside | (~inside & (planar > r))
        out = np.stack([np.where(on_circle, cx, x), np.where(to_top, hh, np.where(to_bottom, -hh, oy)), np.where(on_circle, cz, z)], axis=1).astype(F)
        return to_world(body, out), inside

    return aabb, project


def callbacks(c):
    p = c.params
    if c.kind == "ball":
        return ball_callbacks(c.body, p[0])
    if c.kind == "cuboid":
        return cuboid_callbacks(c.body, p)
    if c.kind == "capsule":
        return capsule_callbacks(c.body, p[0], p[1])
    return cylinder_callbacks(c.body, p[0], p[1])


# ------------------------------------------------------------------------------------------------ the two sides
@dataclass
class Arm:
    """What one step of the arm produced: per collider the emitting particles (ascending) with their projections and velocities at
    the point; the fluid as the first force of the step saw it; the contact search's result; the fluid after the step."""
    sources: list
    points: list
    velocities: list
    pushed_positions: np.ndarray
    probe_velocities: np.ndarray
    ncontacts: int
    counts: np.ndarray
    boundary_counts: np.ndarray
    positions_after: np.ndarray
    velocities_after: np.ndarray


def _sorted(fluids, particles, *arrays):
    assert not np.asarray(fluids).any()
    order = np.argsort(particles, kind="stable")
    return [np.asarray(particles)[order]] + [np.asarray(a, F)[order] for a in arrays]


def run_oracle(colliders, pos, vel, solver="dfsph", dt_prev=DT_PREV, dt=1.0 / 200.0):
    """One step of the f32 oracle: zero gravity, a probe force as the only force."""
    from oracle import oracle as O

    w = O.OracleWorld(R, 2.0, O.DFSPH if solver == "dfsph" else O.IISPH)
    f = w.add_fluid(pos, 1000.0, vel)
    seen = []
    w.add_custom_force(f, lambda world, fl, p, v, dens, acc: seen.append((p.astype(F), v.astype(F))))
    for k, c in enumerate(colliders):
        b = w.add_boundary(np.zeros((0, 3), F))
        assert b == k
        w.set_boundary_dynamic_sampling(b, KIND[c.kind], c.params)
        w.update_boundary_pose(b, c.body.translation, c.body.rotation, c.body.linvel, c.body.angvel, c.body.center_of_mass(), True, False)
    w.set_timestep(dt_prev, 1.0 / dt_prev)
    st = w.step(dt, (0.0, 0.0, 0.0))
    assert len(seen) == 1
    rows = [_sorted(*w.boundary_sources(k), w.boundary_vec(k, "positions"), w.boundary_vec(k, "velocities")) for k in range(len(colliders))]
    return Arm([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], seen[0][0], seen[0][1], int(st.ncontacts),
               w.contact_counts(f), w.contact_counts(f, True), w.fluid_vec(f, "positions"), w.fluid_vec(f, "velocities"))


class HipWorld:
    """The same world on the device.  `host=True`: every collider as a HostShapeSampling over `callbacks` instead of a built-in shape."""

    def __init__(self, colliders, pos, vel, solver="dfsph", host=False, dt_prev=DT_PREV):
        from salva_amd import Boundary, DFSPHSolver, Fluid, IISPHSolver, LiquidWorld, NonPressureForce, _lib
        from salva_amd.coupling import ColliderCouplingSet, DynamicContactSampling, HostShapeSampling

        class Probe(NonPressureForce):
            def __init__(self):
                self.seen = []

            def solve(self, timestep, kernel_radius, ff, fb, fluid, boundaries, densities):
                self.seen.append((fluid.positions.copy(), fluid.velocities.copy()))

        self.colliders, self.probe = colliders, Probe()
        self.world = LiquidWorld(DFSPHSolver() if solver == "dfsph" else IISPHSolver(), R, 2.0)
        fl = Fluid(pos, R, 1000.0)
        fl.velocities = vel
        fl.nonpressure_forces.append(self.probe)
        self.fluid = self.world.add_fluid(fl)
        self.coupling = ColliderCouplingSet()
        self.bounds = []
        for c in colliders:
            b = self.world.add_boundary(Boundary(np.zeros((0, 3), F)))
            self.bounds.append(b)
            self.coupling.register_coupling(b, c.name, c.body, HostShapeSampling(*callbacks(c)) if host else DynamicContactSampling(c.shape))
        self.world.sync_to_device()
        _lib.check(self.world._L.salva_hip_set_timestep(self.world._h, dt_prev, 1.0 / dt_prev))

    def step(self, dt=1.0 / 200.0):
        """One step (zero gravity); the kinematic bodies then move on."""
        self.probe.seen.clear()
        st = self.world.step_with_coupling(dt, (0.0, 0.0, 0.0), self.coupling)
        for c in self.colliders:
            c.body.integrate(dt, (0.0, 0.0, 0.0))
        assert len(self.probe.seen) == 1
        rows = [_sorted(*b.sources(), b.positions, b.velocities) if b.num_particles() else [np.zeros(0, np.uint32), np.zeros((0, 3), F), np.zeros((0, 3), F)]
                for b in self.bounds]
        w, h = self.world, self.fluid
        return Arm([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], self.probe.seen[0][0], self.probe.seen[0][1], int(st.ncontacts),
                   w.contact_counts(h), w.contact_counts(h, True), np.array(h.positions, F).copy(), np.array(h.velocities, F).copy())


def first_difference(c, pred, ids, a, b, what):
    """A message for two readings' rows that differ: the worst particle, its branch by the classifier, and which reading lies nearer
    to the classifier's nearest surface point."""
    bad = np.nonzero((a != b).reshape(len(ids), -1).any(1))[0]
    k = bad[np.argmax(np.abs(a[bad].astype(np.float64) - b[bad]).reshape(len(bad), -1).max(1))]
    labels, _, near = classify(c, pred[ids[k]][None])
    msg = f"{c.name}: {what} differ for {len(bad)} of {len(ids)} particles; particle {ids[k]} in branch '{labels[0]}': {a[k]} vs {b[k]}"
    if np.ndim(a) == 2:
        msg += f"; distances to the nearest surface point {np.linalg.norm(a[k] - near[0]):.3e} vs {np.linalg.norm(b[k] - near[0]):.3e}"
    return msg


# ------------------------------------------------------------------------------------------------ degenerate points
# Exact points on the borders between branches: identity rotation, dyadic sizes and translation, zero velocity — the local coordinates
# are exact, so the comparisons inside the projections see true equalities.  (name, shape, [(what, local point, expected local
# projection)]).  No particle sits at a ball's exact centre: the reference computes r / 0 * 0 = NaN there, and a NaN boundary point
# entering the grid is not something to feed a device for the sake of a test.
DEGENERATE_T = F([0.5, -0.25, 0.125])
DEGENERATE = [
    ("capsule", ("capsule", 0.25, 0.125), [
        ("on the segment's interior", (0.0, 0.0625, 0.0), (0.125, 0.0625, 0.0)),
        ("on the axis beyond end b, inside", (0.0, 0.3125, 0.0), (0.0, 0.375, 0.0)),
        ("on the axis beyond end a, outside", (0.0, -0.4375, 0.0), (0.0, -0.375, 0.0)),
        ("exactly at end b", (0.0, 0.25, 0.0), (0.125, 0.25, 0.0)),
        ("exactly at end a", (0.0, -0.25, 0.0), (0.125, -0.25, 0.0)),
    ]),
    ("tall cylinder", ("cylinder", 0.25, 0.125), [
        ("on the axis inside: side, through the planar <= eps fallback", (0.0, 0.0625, 0.0), (0.125, 0.0625, 0.0)),
        ("on the axis above the cap", (0.0, 0.3125, 0.0), (0.0, 0.25, 0.0)),
        ("y = 0: top equals bottom, side wins", (0.0625, 0.0, 0.0), (0.125, 0.0, 0.0)),
        ("top equals side: side wins", (0.0625, 0.1875, 0.0), (0.125, 0.1875, 0.0)),
    ]),
    ("flat cylinder", ("cylinder", 0.125, 0.25), [
        ("on the axis inside: the nearer cap", (0.0, 0.0625, 0.0), (0.0, 0.125, 0.0)),
        ("on the axis below the cap", (0.0, -0.1875, 0.0), (0.0, -0.125, 0.0)),
        ("y = 0: top equals bottom, side wins although it is farther", (0.0625, 0.0, 0.0), (0.25, 0.0, 0.0)),
        ("top equals side: side wins", (0.1875, 0.0625, 0.0), (0.25, 0.0625, 0.0)),
    ]),
    ("cuboid", ("cuboid", (0.25, 0.125, 0.1875)), [
        ("the centre: mins - p == p - maxs on every axis, the mins side of the thinnest axis", (0.0, 0.0, 0.0), (0.0, -0.125, 0.0)),
        ("exactly on a face", (0.25, 0.03125, 0.0625), (0.25, 0.03125, 0.0625)),
        ("exactly on an edge", (0.25, 0.125, -0.0625), (0.25, 0.125, -0.0625)),
        ("exactly on a corner", (-0.25, -0.125, 0.1875), (-0.25, -0.125, 0.1875)),
    ]),
    ("cube", ("cuboid", (0.125, 0.125, 0.125)), [
        ("the centre of a cube: the first axis wins", (0.0, 0.0, 0.0), (-0.125, 0.0, 0.0)),
    ]),
    ("ball", ("ball", 0.25), [
        ("exactly on the surface: inside, dpt = 0, emits without a push", (0.25, 0.0, 0.0), (0.25, 0.0, 0.0)),
        ("inside on an axis", (0.0, -0.125, 0.0), (0.0, -0.25, 0.0)),
    ]),
]


def degenerate_world(case):
    """(collider, positions, velocities, expected world projections or None) of one DEGENERATE entry."""
    name, shape, points = case
    body = RigidBody(translation=DEGENERATE_T.copy(), linvel=F([0.25, 0.0, -0.5]), angvel=F([0.0, 1.0, 0.5]), local_com=F([0.0, 0.0625, 0.0]), dynamic=False)
    c = Collider(name, shape, body)
    pos = (np.array([p[1] for p in points], F) + DEGENERATE_T).astype(F)
    assert len(pos) <= 16
    want = [None if p[2] is None else (F(p[2]) + DEGENERATE_T).astype(F) for p in points]
    return c, pos, np.zeros_like(pos), want

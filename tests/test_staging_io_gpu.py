"""The host-order ("staging") arrays and the host <-> device transfers behind the C API: every edit of the fluid and boundary
sets (salva_hip_set_fluid, _add_particles, _delete_particles, _remove_fluid, _set_boundary, _remove_boundary) followed by every
read-back (salva_hip_get_fluid, _get_fluid_async, _get_fluid_field, _get_boundary, _get_boundary_particles, _get_local,
_get_fluid_contacts, _get_local_contacts), next to a NumPy model of those arrays.  These paths only move data: every comparison
is bitwise, and every array holds distinct values so that a row in the wrong place shows.

The solver's per-slot buffers (velocity changes, IISPH pressures) are positional in the reference and outlive a removed fluid
(test_oracle.py::test_add_delete_remove_follow_the_reference_bookkeeping): the fluid that moves into, or is created in, a slot
inherits the buffer that is there, truncated or zero-extended, and particles added before the next step get its tail.  The model
keeps such a buffer in `Sim.left` and applies exactly that rule."""
import ctypes as C

import numpy as np
import pytest

from salva_amd import _lib

pytestmark = pytest.mark.gpu
R = 0.025
DT = 1.0 / 200.0
FP, U8P, U32P, U64P = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
VEC_FIELDS = (_lib.FIELD_VELOCITY_CHANGE, _lib.FIELD_ACCELERATION)
SOLVERS = {"dfsph": _lib.SOLVER_DFSPH, "iisph": _lib.SOLVER_IISPH}


def fp(a):
    return None if a is None else a.ctypes.data_as(FP)


def same(got, want, what=""):
    """Bit for bit."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {g.size} words differ, first at {np.argwhere(g != w)[0].tolist()}"


def resized(buf, n):
    """Vec::resize(n, zero) of a positional solver buffer."""
    out = np.zeros((n, 4), np.float32)
    m = min(n, len(buf))
    out[:m] = buf[:m]
    return out


def lattice(nx, ny, nz, origin):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3)
    p = np.float32(origin) + g.astype(np.float32) * np.float32(2 * R)
    return (p + np.arange(p.size, dtype=np.float32).reshape(p.shape) * np.float32(2.0 ** -20)).astype(np.float32)


class Sim:
    """A device world driven through the C API, and the NumPy model of its host-order arrays."""

    def __init__(self, solver):
        self.L = _lib.lib()
        p = _lib.Params()
        self.L.salva_hip_default_params(C.byref(p))
        p.particle_radius, p.smoothing_factor, p.solver = R, 2.0, SOLVERS[solver]
        self.h = C.c_void_p()
        _lib.check(self.L.salva_hip_create(C.byref(p), C.byref(self.h)))
        self.fluids, self.bounds = [], []   # fluids: pos, vel, vol, acc, dv (x, y, z = velocity change, w = pressure), rho0
        self.left = {}                      # slot -> the positional solver buffer a removed / moved fluid left there
        self.acc_user = False
        self.counter = 1
        r = np.float32(R)
        self.default_volume = r * r * r * np.float32(6.4)
        self.pin_cap = 4096
        self.pin_ptr = self.L.salva_hip_host_alloc(self.h, 4 * self.pin_cap)
        assert self.pin_ptr
        self.pinned = np.ctypeslib.as_array((C.c_float * self.pin_cap).from_address(self.pin_ptr))

    def close(self):
        _lib.check(self.L.salva_hip_wait_download(self.h))
        _lib.check(self.L.salva_hip_host_free(self.pin_ptr))
        self.L.salva_hip_destroy(self.h)

    def fresh(self, *shape):
        """Values no other array of the test holds (exact in float32)."""
        k = int(np.prod(shape))
        a = (np.arange(self.counter, self.counter + k, dtype=np.float32) * np.float32(2.0 ** -8)).reshape(shape)
        self.counter += k
        assert self.counter < 2 ** 24
        return a

    # ---- edits: the device call, then the model
    def set_fluid(self, slot, pos, vel=None, vol=None, acc=None, dvs=None, rho0=1000.0, dirty=_lib.DIRTY_ALL):
        nn = len(pos)
        _lib.check(self.L.salva_hip_set_fluid(self.h, slot, nn, fp(pos), fp(vel), fp(vol), fp(acc), fp(dvs), rho0, 1, 0xffffffff, dirty))
        is_new = slot == len(self.fluids)
        if is_new or len(self.fluids[slot]["pos"]) != nn:
            dirty = _lib.DIRTY_ALL
            f = dict(pos=np.zeros((nn, 3), np.float32), vel=np.zeros((nn, 3), np.float32), vol=np.full(nn, self.default_volume, np.float32),
                     acc=np.zeros((nn, 3), np.float32), dv=np.zeros((nn, 4), np.float32))
            if is_new:
                self.fluids.append(f)
                if dvs is None and slot in self.left:
                    f["dv"] = resized(self.left[slot], nn)
                    if len(self.left[slot]) <= nn:
                        del self.left[slot]
            else:
                self.fluids[slot] = f
        f = self.fluids[slot]
        f["rho0"] = rho0
        if dirty & _lib.DIRTY_POSITIONS:
            f["pos"] = pos.copy()
        if dirty & _lib.DIRTY_VELOCITIES and vel is not None:
            f["vel"] = vel.copy()
        if dirty & _lib.DIRTY_VOLUMES and vol is not None:
            f["vol"] = vol.copy()
        if dirty & _lib.DIRTY_ACCELERATIONS and acc is not None:
            f["acc"] = acc.copy()
            self.acc_user = True
        if dvs is not None:
            f["dv"][:, :3] = dvs

    def set_field(self, slot, field, data):
        _lib.check(self.L.salva_hip_set_fluid_field(self.h, slot, field, fp(data)))
        if field == _lib.FIELD_VELOCITY_CHANGE:
            self.fluids[slot]["dv"][:, :3] = data
        else:
            self.fluids[slot]["dv"][:, 3] = data

    def add_particles(self, slot, pos, vel=None):
        _lib.check(self.L.salva_hip_add_particles(self.h, slot, len(pos), fp(pos), fp(vel)))
        f, k = self.fluids[slot], len(pos)
        old_n = len(f["pos"])
        f["pos"] = np.concatenate([f["pos"], pos])
        f["vel"] = np.concatenate([f["vel"], np.zeros((k, 3), np.float32) if vel is None else vel])
        f["vol"] = np.concatenate([f["vol"], np.full(k, self.default_volume, np.float32)])
        f["acc"] = np.concatenate([f["acc"], np.zeros((k, 3), np.float32)])
        tail = resized(self.left[slot][old_n:], k) if slot in self.left else np.zeros((k, 4), np.float32)
        f["dv"] = np.concatenate([f["dv"], tail])

    def delete_particles(self, slot, mask):
        m = np.ascontiguousarray(mask, np.uint8)
        kept = self.L.salva_hip_delete_particles(self.h, slot, m.ctypes.data_as(U8P))
        f = self.fluids[slot]
        keep = m == 0
        assert kept == int(keep.sum())
        for k in ("pos", "vel", "vol", "acc", "dv"):
            f[k] = f[k][keep]
        if slot in self.left:  # filtered with the same mask; what lies beyond the fluid's particles moves down
            b = self.left[slot]
            k2 = np.ones(len(b), bool)
            k2[:min(len(b), len(keep))] = keep[:len(b)]
            self.left[slot] = b[k2]

    def remove_fluid(self, slot):
        _lib.check(self.L.salva_hip_remove_fluid(self.h, slot))
        last = len(self.fluids) - 1
        a = self.left.pop(slot, self.fluids[slot]["dv"])
        b = self.left.pop(last, self.fluids[last]["dv"]) if slot != last else None
        if slot != last:
            self.fluids[slot] = self.fluids[last]
            moved = self.fluids[slot]
            moved["dv"] = resized(a, len(moved["pos"]))
            if len(a) > len(moved["pos"]):
                self.left[slot] = a
            self.left[last] = b
        else:
            self.left[last] = a
        self.fluids.pop()

    def set_boundary(self, slot, pos, vel=None, wants_forces=True):
        _lib.check(self.L.salva_hip_set_boundary(self.h, slot, len(pos), fp(pos), fp(vel), 1, 0xffffffff, 1 if wants_forces else 0))
        b = dict(pos=pos.copy(), vel=np.zeros_like(pos) if vel is None else vel.copy())
        if slot == len(self.bounds):
            self.bounds.append(b)
        else:
            self.bounds[slot] = b

    def remove_boundary(self, slot):
        _lib.check(self.L.salva_hip_remove_boundary(self.h, slot))
        self.bounds[slot] = self.bounds[-1]
        self.bounds.pop()

    def step(self):
        g = (C.c_float * 3)(0.0, -9.81, 0.0)
        st = _lib.StepStats()
        _lib.check(self.L.salva_hip_step(self.h, DT, g, C.byref(st)))
        return st

    # ---- reads
    def get_fluid(self, slot, n):
        p, v = np.full((n, 3), np.nan, np.float32), np.full((n, 3), np.nan, np.float32)
        _lib.check(self.L.salva_hip_get_fluid(self.h, slot, fp(p), fp(v)))
        return p, v

    def get_fluid_async(self, slot, n, pinned):
        if pinned:
            assert 6 * n <= self.pin_cap
            self.pinned[:] = np.nan
            p, v = self.pinned[:3 * n].reshape(n, 3), self.pinned[3 * n:6 * n].reshape(n, 3)
        else:
            p, v = np.full((n, 3), np.nan, np.float32), np.full((n, 3), np.nan, np.float32)
        _lib.check(self.L.salva_hip_get_fluid_async(self.h, slot, fp(p), fp(v)))
        _lib.check(self.L.salva_hip_wait_download(self.h))
        return p.copy(), v.copy()

    def field(self, slot, field, n):
        out = np.full((n, 3) if field in VEC_FIELDS else n, np.nan, np.float32)
        _lib.check(self.L.salva_hip_get_fluid_field(self.h, slot, field, fp(out)))
        return out

    def check_fluids(self, what, asynchronous=True):
        assert self.L.salva_hip_num_fluids(self.h) == len(self.fluids)
        for s, f in enumerate(self.fluids):
            n = len(f["pos"])
            assert self.L.salva_hip_fluid_len(self.h, s) == n
            tag = f"{what}, fluid {s}"
            p, v = self.get_fluid(s, n)
            same(p, f["pos"], tag + " positions")
            same(v, f["vel"], tag + " velocities")
            if asynchronous:
                for pinned in (False, True):
                    p, v = self.get_fluid_async(s, n, pinned)
                    same(p, f["pos"], tag + f" positions (async, pinned={pinned})")
                    same(v, f["vel"], tag + f" velocities (async, pinned={pinned})")
            same(self.field(s, _lib.FIELD_VELOCITY_CHANGE, n), f["dv"][:, :3], tag + " velocity changes")
            same(self.field(s, _lib.FIELD_PRESSURE, n), f["dv"][:, 3], tag + " pressures")
            same(self.field(s, _lib.FIELD_VOLUME, n), f["vol"], tag + " volumes")
            same(self.field(s, _lib.FIELD_ACCELERATION, n), f["acc"] if self.acc_user else np.zeros((n, 3), np.float32), tag + " accelerations")

    def check_boundaries(self, what):
        assert self.L.salva_hip_num_boundaries(self.h) == len(self.bounds)
        for s, b in enumerate(self.bounds):
            n = len(b["pos"])
            assert self.L.salva_hip_boundary_len(self.h, s) == n
            p, v, f = (np.full((n, 3), np.nan, np.float32) for _ in range(3))
            _lib.check(self.L.salva_hip_get_boundary_particles(self.h, s, fp(p), fp(v)))
            _lib.check(self.L.salva_hip_get_boundary(self.h, s, None, fp(f)))
            same(p, b["pos"], f"{what}, boundary {s} positions")
            same(v, b["vel"], f"{what}, boundary {s} velocities")
            same(f, b.get("force", np.zeros((n, 3), np.float32)), f"{what}, boundary {s} forces")


def make_scene(solver, with_velocities=False):
    s = Sim(solver)
    a, b = lattice(3, 3, 3, (0.0, 0.0, 0.0)), lattice(4, 4, 4, (6 * R, 0.0, 0.0))
    floor = lattice(10, 1, 10, (-4 * R, -2 * R, -2 * R))
    va = s.fresh(27, 3) * np.float32(2.0 ** -6) if with_velocities else s.fresh(27, 3)
    vb = s.fresh(64, 3) * np.float32(2.0 ** -6) if with_velocities else s.fresh(64, 3)
    s.set_fluid(0, a, va, None if with_velocities else s.fresh(27), rho0=1000.0)
    s.set_fluid(1, b, vb, None if with_velocities else s.fresh(64), rho0=800.0)
    s.set_boundary(0, floor, None, wants_forces=True)
    return s


@pytest.fixture(params=sorted(SOLVERS))
def solver(request):
    return request.param


def test_round_trip_before_any_step(solver):
    s = make_scene(solver)
    try:
        s.check_fluids("as created")  # (no acceleration was uploaded: the field reads zeros)
        s.check_boundaries("as created")
        for dvs in (False, True):
            for dirty in range(16):
                for slot in (0, 1):
                    n = len(s.fluids[slot]["pos"])
                    pos = s.fluids[slot]["pos"] + s.fresh(n, 3) * np.float32(2.0 ** -12)
                    s.set_fluid(slot, pos, s.fresh(n, 3), s.fresh(n), s.fresh(n, 3), s.fresh(n, 3) if dvs else None,
                                rho0=s.fluids[slot]["rho0"], dirty=dirty)
                s.check_fluids(f"set_fluid dirty={dirty} dvs={dvs}", asynchronous=dirty in (0, 5, 15))
        assert s.acc_user
        for slot in (1, 0):
            n = len(s.fluids[slot]["pos"])
            s.set_field(slot, _lib.FIELD_VELOCITY_CHANGE, s.fresh(n, 3))
            s.check_fluids(f"set_fluid_field(VELOCITY_CHANGE, {slot})", asynchronous=False)
            s.set_field(slot, _lib.FIELD_PRESSURE, s.fresh(n))
            s.check_fluids(f"set_fluid_field(PRESSURE, {slot})")
    finally:
        s.close()


def test_edits_without_a_step_in_between(solver):
    """dfsph: fluid A ends longer than B, so B inherits a truncated buffer and A's tail stays behind; iisph: shorter, so B's is
    zero-extended."""
    a_final = 70 if solver == "dfsph" else 40
    s = make_scene(solver)
    try:
        for slot in (0, 1):  # the solver state that the edits below have to carry along
            n = len(s.fluids[slot]["pos"])
            s.set_field(slot, _lib.FIELD_VELOCITY_CHANGE, s.fresh(n, 3))
            s.set_field(slot, _lib.FIELD_PRESSURE, s.fresh(n))
        s.add_particles(0, s.fresh(5, 3), s.fresh(5, 3))
        s.check_fluids("add_particles with velocities")
        s.add_particles(0, s.fresh(5, 3), None)
        s.check_fluids("add_particles without velocities")
        mask = np.zeros(64, np.uint8)
        mask[[0, 37, 63]] = 1
        s.delete_particles(1, mask)
        s.check_fluids("delete_particles")
        # the first user accelerations of the world: every other fluid's stay zero
        s.set_fluid(1, s.fluids[1]["pos"], None, None, s.fresh(61, 3), None, rho0=800.0, dirty=_lib.DIRTY_ACCELERATIONS)
        s.check_fluids("first acceleration upload", asynchronous=False)
        s.set_fluid(0, s.fresh(20, 3), s.fresh(20, 3), None, None, None, rho0=1000.0)
        s.check_fluids("set_fluid resizing down")
        s.set_fluid(0, s.fresh(a_final, 3), None, s.fresh(a_final), s.fresh(a_final, 3), s.fresh(a_final, 3), rho0=1000.0)
        s.set_field(0, _lib.FIELD_PRESSURE, s.fresh(a_final))
        s.check_fluids("set_fluid resizing up")
        # boundaries: a second one, so that a resize of the first moves rows
        s.set_boundary(1, s.fresh(7, 3), s.fresh(7, 3), wants_forces=False)
        s.check_boundaries("second boundary")
        for n in (64, 121):
            s.set_boundary(0, s.fresh(n, 3), s.fresh(n, 3) if n == 64 else None, wants_forces=True)
            s.check_boundaries(f"set_boundary resizing to {n}")
        s.check_fluids("after the boundary edits", asynchronous=False)
        # remove_fluid(0): B moves into slot 0 and inherits A's velocity changes and pressures, truncated or zero-extended
        a_dv, b_dv = s.fluids[0]["dv"].copy(), s.fluids[1]["dv"].copy()
        s.remove_fluid(0)
        assert len(s.fluids) == 1 and len(s.fluids[0]["pos"]) == 61
        same(s.fluids[0]["dv"], resized(a_dv, 61), "the model's own inheritance rule")
        s.check_fluids("remove_fluid(0)")
        s.add_particles(0, s.fresh(3, 3), s.fresh(3, 3))  # ... and A's tail, if there is one, goes to particles added before the next step
        same(s.fluids[0]["dv"][61:], resized(a_dv[61:], 3), "the model's own tail rule")
        s.check_fluids("add_particles after remove_fluid")
        mask = np.zeros(64, np.uint8)  # the buffer left behind is compacted with the fluid: its tail moves down
        mask[[0, 62]] = 1
        s.delete_particles(0, mask)
        s.add_particles(0, s.fresh(3, 3), None)
        same(s.fluids[0]["dv"][62:], resized(np.delete(resized(a_dv, max(len(a_dv), 64)), [0, 62], axis=0)[62:], 3),
             "the model's own tail rule after a deletion")
        s.check_fluids("delete_particles and add_particles after remove_fluid")
        # a fluid created in the freed last slot finds B's old buffer there
        s.set_fluid(1, s.fresh(30, 3), s.fresh(30, 3), None, None, None, rho0=900.0)
        same(s.fluids[1]["dv"], b_dv[:30], "the model's own inheritance rule (new fluid)")
        s.check_fluids("a fluid in the freed slot")
        s.add_particles(1, s.fresh(4, 3), None)
        same(s.fluids[1]["dv"][30:], b_dv[30:34], "the model's own tail rule (new fluid)")
        s.check_fluids("add_particles to the fluid in the freed slot")
        s.remove_boundary(0)
        s.check_boundaries("remove_boundary(0)")
        s.remove_boundary(0)
        s.check_boundaries("remove_boundary of the last one")
        s.check_fluids("at the end", asynchronous=False)
    finally:
        s.close()


def _contacts(s, slot, boundary, n):
    off = np.zeros(n + 1, np.uint64)
    total = s.L.salva_hip_get_fluid_contacts(s.h, slot, boundary, off.ctypes.data_as(U64P), None, None, 0)  # the sizing call
    assert total >= 0 and int(off[n]) == total
    jm, j = np.full(max(total, 1), 0xffffffff, np.uint32), np.full(max(total, 1), 0xffffffff, np.uint32)
    off2 = np.zeros(n + 1, np.uint64)
    assert s.L.salva_hip_get_fluid_contacts(s.h, slot, boundary, off2.ctypes.data_as(U64P), jm.ctypes.data_as(U32P), j.ctypes.data_as(U32P), total) == total
    assert np.array_equal(off, off2)
    return off.astype(np.int64), jm[:total], j[:total]


def test_after_one_step(solver):
    s = make_scene(solver, with_velocities=True)
    try:
        s.step()
        counts = [27, 64]
        first = [0, 27]
        # the asynchronous read-back first: it reads the sorted working set, the synchronous one un-sorts into the staging arrays
        got_async = [s.get_fluid_async(k, counts[k], pinned=False) for k in (0, 1)]
        got = [s.get_fluid(k, counts[k]) for k in (0, 1)]
        vols = [s.field(k, _lib.FIELD_VOLUME, counts[k]) for k in (0, 1)]
        for k in (0, 1):
            assert not np.array_equal(got[k][0], s.fluids[k]["pos"]), "the step moved nothing"
            same(got_async[k][0], got[k][0], f"fluid {k} positions, async from the sorted set")
            same(got_async[k][1], got[k][1], f"fluid {k} velocities, async from the sorted set")
            p, v = s.get_fluid_async(k, counts[k], pinned=True)  # (the staging arrays are current now)
            same(p, got[k][0], f"fluid {k} positions, async from the staging arrays")
            same(v, got[k][1], f"fluid {k} velocities, async from the staging arrays")
            same(vols[k], s.fluids[k]["vol"], f"fluid {k} volumes")
        # the local view, gathered by its ids
        n = int(s.L.salva_hip_local_len(s.h))
        assert n == 91
        ids, slots, ghost = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.ones(n, np.uint8)
        lp, lv, lrho, lvol = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        _lib.check(s.L.salva_hip_get_local(s.h, ids.ctypes.data_as(U32P), slots.ctypes.data_as(U32P), ghost.ctypes.data_as(U8P), fp(lp), fp(lv),
                                           fp(lrho), fp(lvol)))
        assert sorted(ids.tolist()) == list(range(n)) and not ghost.any()
        assert np.array_equal(slots, (ids >= 27).astype(np.uint32))
        same(lp, np.concatenate([got[0][0], got[1][0]])[ids], "local positions")
        same(lv, np.concatenate([got[0][1], got[1][1]])[ids], "local velocities")
        same(lvol, np.concatenate(vols)[ids], "local volumes")
        rho_host = np.zeros(n, np.float32)
        rho_host[ids] = lrho
        local_of = np.zeros(n, np.int64)
        local_of[ids] = np.arange(n)
        for boundary in (0, 1):
            loff = np.zeros(n + 1, np.uint64)
            total = s.L.salva_hip_get_local_contacts(s.h, boundary, loff.ctypes.data_as(U64P), None, None, 0)
            assert total >= 0 and int(loff[n]) == total and (boundary or total >= n)  # (the self contact is included)
            ljm, lj = np.zeros(max(total, 1), np.uint32), np.zeros(max(total, 1), np.uint32)
            assert s.L.salva_hip_get_local_contacts(s.h, boundary, loff.ctypes.data_as(U64P), ljm.ctypes.data_as(U32P), lj.ctypes.data_as(U32P), total) == total
            loff = loff.astype(np.int64)
            for k in (0, 1):
                off, jm, j = _contacts(s, k, boundary, counts[k])
                for i in range(counts[k]):
                    mine = sorted(zip(jm[off[i]:off[i + 1]].tolist(), j[off[i]:off[i + 1]].tolist()))
                    li = local_of[first[k] + i]
                    m, jj = ljm[loff[li]:loff[li + 1]], lj[loff[li]:loff[li + 1]]
                    if not boundary:  # a local index -> the fluid and the index inside its host arrays
                        g = ids[jj].astype(np.int64)
                        assert np.array_equal(m, slots[jj])
                        jj = g - np.asarray(first)[m]
                    assert mine == sorted(zip(m.tolist(), np.asarray(jj).tolist())), (boundary, k, i)
                num = s.field(k, _lib.FIELD_NUM_BOUNDARY_CONTACTS if boundary else _lib.FIELD_NUM_FLUID_CONTACTS, counts[k])
                same(num, np.diff(off).astype(np.float32), f"fluid {k} contact counts (boundary={boundary})")
        for k in (0, 1):
            same(s.field(k, _lib.FIELD_DENSITY, counts[k]), rho_host[first[k]:first[k] + counts[k]], f"fluid {k} densities")
            alpha = s.field(k, _lib.FIELD_ALPHA, counts[k])
            assert not np.isnan(alpha).any()
            same(s.field(k, _lib.FIELD_ALPHA, counts[k]), alpha, f"fluid {k} alpha, read twice")
        # the reaction forces of the step ride along when another boundary is added and the first one leaves
        force = np.full((100, 3), np.nan, np.float32)
        _lib.check(s.L.salva_hip_get_boundary(s.h, 0, None, fp(force)))
        assert not np.isnan(force).any()
        s.bounds[0]["force"] = force
        s.set_boundary(1, s.fresh(4, 3), s.fresh(4, 3), wants_forces=True)
        s.check_boundaries("a second boundary after the step")
        s.remove_boundary(0)
        s.check_boundaries("remove_boundary(0) after the step")
    finally:
        s.close()


def test_error_paths_keep_their_codes_and_messages():
    s = make_scene("dfsph")
    L, h = s.L, s.h
    buf, u = np.zeros(3 * 128, np.float32), np.zeros(256, np.uint32)
    o64, m8 = np.zeros(128, np.uint64), np.zeros(128, np.uint8)
    B, U, O = fp(buf), u.ctypes.data_as(U32P), o64.ctypes.data_as(U64P)
    slot = "fluid slot out of range"
    bslot = "boundary slot out of range"
    cb = "only available inside a force callback"
    nostep = "no completed step: there are no contact lists yet"
    cases = [
        (lambda: L.salva_hip_set_fluid(h, 3, 4, B, None, None, None, None, 1000.0, 1, 1, 15), "fluid slot out of range (slots are dense)"),
        (lambda: L.salva_hip_set_fluid(h, 2, 4, None, None, None, None, None, 1000.0, 1, 1, 15), "positions are required when a fluid is created or resized"),
        (lambda: L.salva_hip_set_fluid(h, 0, 4, None, None, None, None, None, 1000.0, 1, 1, 15), "positions are required when a fluid is created or resized"),
        (lambda: L.salva_hip_add_particles(h, 2, 1, B, None), slot),
        (lambda: L.salva_hip_add_particles(h, 2, 1, None, None), slot),
        (lambda: L.salva_hip_add_particles(h, 0, 1, None, None), "positions are required"),
        (lambda: L.salva_hip_delete_particles(h, 2, m8.ctypes.data_as(U8P)), slot),
        (lambda: L.salva_hip_set_fluid_forces(h, 2, None, 0), slot),
        (lambda: L.salva_hip_remove_fluid(h, 2), slot),
        (lambda: L.salva_hip_set_boundary(h, 2, 1, B, None, 1, 1, 0), "boundary slot out of range (slots are dense)"),
        (lambda: L.salva_hip_set_boundary(h, 1, 1, None, None, 1, 1, 0), "boundary positions are required"),
        (lambda: L.salva_hip_remove_boundary(h, 1), bslot),
        (lambda: L.salva_hip_get_boundary(h, 1, None, B), bslot),
        (lambda: L.salva_hip_get_boundary_particles(h, 1, B, None), bslot),
        (lambda: L.salva_hip_get_fluid(h, 2, B, None), slot),
        (lambda: L.salva_hip_get_fluid_async(h, 2, B, None), slot),
        (lambda: L.salva_hip_get_fluid_field(h, 2, _lib.FIELD_VOLUME, B), slot),
        (lambda: L.salva_hip_get_fluid_field(h, 2, _lib.FIELD_VOLUME, None), slot),
        (lambda: L.salva_hip_get_fluid_field(h, 0, _lib.FIELD_VOLUME, None), "null output"),
        (lambda: L.salva_hip_get_fluid_field(h, 0, _lib.FIELD_DENSITY, B), "solver scratch fields are only available right after a step"),
        (lambda: L.salva_hip_get_fluid_field(h, 0, 99, B), "solver scratch fields are only available right after a step"),
        (lambda: L.salva_hip_set_fluid_field(h, 2, _lib.FIELD_PRESSURE, B), slot),
        (lambda: L.salva_hip_set_fluid_field(h, 2, _lib.FIELD_DENSITY, None), slot),
        (lambda: L.salva_hip_set_fluid_field(h, 0, _lib.FIELD_DENSITY, None), "null data"),
        (lambda: L.salva_hip_set_fluid_field(h, 0, _lib.FIELD_DENSITY, B), "only velocity_changes and pressures can be set"),
        (lambda: L.salva_hip_set_fluid_field(h, 0, _lib.FIELD_VOLUME, B), "only velocity_changes and pressures can be set"),
        (lambda: L.salva_hip_get_fluid_contacts(h, 2, 0, O, U, U, 128), slot),
        (lambda: L.salva_hip_get_fluid_contacts(h, 0, 0, O, U, U, 128), nostep),
        (lambda: L.salva_hip_get_local_contacts(h, 0, O, U, U, 128), nostep),
        (lambda: L.salva_hip_get_local(h, U, None, None, None, None, None, None), "no completed step: the working set has no order yet"),
        (lambda: L.salva_hip_force_get_state(h, 0, B, None, None), cb),
        (lambda: L.salva_hip_force_get_state(h, 2, B, None, None), cb),
        (lambda: L.salva_hip_force_add_accelerations(h, 0, B), cb),
        (lambda: L.salva_hip_force_add_accelerations(h, 2, None), cb),
        (lambda: L.salva_hip_force_add_local_accelerations(h, B), cb),
        (lambda: L.salva_hip_force_add_local_accelerations(h, None), cb),
        (lambda: L.salva_hip_get_force_stats(h, 2, 0, None, None), "fluid slot / force index out of range"),
        (lambda: L.salva_hip_get_force_stats(h, 0, 0, None, None), "fluid slot / force index out of range"),
    ]
    try:
        for k, (call, message) in enumerate(cases):
            assert call() == _lib.E_INVALID, (k, message)
            assert L.salva_hip_last_error().decode() == message, k
        s.check_fluids("after the refused calls")  # none of them changed anything
        s.check_boundaries("after the refused calls")
        s.step()
        assert L.salva_hip_get_fluid_field(h, 0, 99, B) == _lib.E_INVALID
        assert L.salva_hip_last_error().decode() == "unknown field"
        assert L.salva_hip_get_fluid_contacts(h, 2, 1, O, U, U, 128) == _lib.E_INVALID
        assert L.salva_hip_last_error().decode() == slot
        # an edit ends what the step left: the solver's scratch and the contact lists are gone again
        s.set_field(0, _lib.FIELD_PRESSURE, s.fresh(27))
        assert L.salva_hip_get_fluid_field(h, 0, _lib.FIELD_DENSITY, B) == _lib.E_INVALID
        assert L.salva_hip_last_error().decode() == "solver scratch fields are only available right after a step"
        assert L.salva_hip_get_local_contacts(h, 0, O, U, U, 128) == _lib.E_INVALID
        assert L.salva_hip_last_error().decode() == nostep
    finally:
        s.close()

"""The scenes and the case matrix in which every built-in NonPressureForce is looked at by itself: shared by
tests/test_force_reading_cpu.py (the CPU oracle with a recording custom force on either side of the built-in one) and
tests/test_forces_isolated_gpu.py (the device with a DeviceForce reader on either side).

A force is described in the numpy reading's terms (numpy_reading.DenseWorld.add_force): ("xsph", c_f, c_b),
("artificial", c_f, c_b, alpha, beta, speed_of_sound), ("akinci2013", tension, adhesion), ("he2014", c_f, c_b), ("wcsph", c_f),
("dfsph_viscosity", coefficient, min_iter, max_iter, max_error).

Test infrastructure only."""
from collections import namedtuple

import numpy as np

from salva_amd import scenes

R = 0.025
DT = 1.0 / 200.0
GRAVITY = (0.0, -9.81, 0.0)
NSTEPS = 3
COMPARED = (1, 2)  # steps 2 and 3 (0-based): at step 1 the timestep's inv_dt is still 0, XSPH and DFSPHViscosity add nothing

F = np.float32
# Added to every fluid particle's vertical velocity in scenes A and B.  A block let go above a floor falls onto it, and by step 3
# four boundary contacts in five are approaching; with this drift upwards about half of them are, at steps 2 and 3 alike.
LIFT = 0.2


def _volumes(n, seed):
    """0.8 (2r)^3 (1 + 0.2 u): particle masses that differ, so that m_i for m_j shows"""
    return (F(0.8) * F(2 * R) ** 3 * (F(1.0) + F(0.2) * scenes.lcg_uniform(n, seed))).astype(F)


def _floor(nx, nz):
    """one layer at y = 0, moving at 0.5 m/s along x; it reaches h = 4 r beyond the fluid on every side"""
    pos = scenes.plane_lattice(nx, nz, 0.0, R, -(nx - 1) * R, -(nz - 1) * R, layers=1)
    vel = np.zeros_like(pos)
    vel[:, 0] = 0.5
    return pos, vel


def scene_a(coincident=False):
    """One fluid: a 9 x 9 x 9 block jittered by 0.1 r (4.5 cells of h = 4 r per axis: more than one 4-cell tile, the outer tiles
    partly filled), velocities of 0.3 m/s at random, its lowest layer 3 r above the floor, and one stray particle further than h
    from everything.  `coincident`: one more particle at the position, and with the velocity, of a particle inside the block."""
    pos = scenes.jitter(scenes.cube_fluid_positions(9, 9, 9, R), 0.1 * R, seed=21)
    pos[:, 1] += F(11 * R)
    vel = scenes.random_velocities(len(pos), 0.3, seed=22)
    vel[:, 1] += F(LIFT)
    extra_p, extra_v = [[0.0, 19 * R + 3 * 4 * R, 0.0]], [[0.0, 0.0, 0.0]]
    if coincident:
        k = (4 * 9 + 4) * 9 + 4  # the block's central particle
        extra_p.append(pos[k]); extra_v.append(vel[k])
    pos = np.concatenate([pos, np.asarray(extra_p, F)]).astype(F)
    vel = np.concatenate([vel, np.asarray(extra_v, F)]).astype(F)
    vol = _volumes(len(pos), 23)
    if coincident:
        vol[-1] = vol[k]
    return dict(fluids=[dict(pos=pos, vel=vel, vol=vol, density0=1000.0)], floor=_floor(13, 13))


def scene_b():
    """Two fluids of density0 1000 and 500, 5 x 9 x 9 particles each, side by side along x over the same floor: they share an
    interface of 9 x 9 particles (4.5 cells on either axis), and both touch the floor."""
    fluids = []
    for k, (sx, rho0) in enumerate(((-1, 1000.0), (1, 500.0))):
        pos = scenes.jitter(scenes.cube_fluid_positions(5, 9, 9, R), 0.1 * R, seed=31 + k)
        pos[:, 0] += F(sx * 5 * R)
        pos[:, 1] += F(11 * R)
        vel = scenes.random_velocities(len(pos), 0.4, seed=33 + k)  # (0.4: the beta share of ArtificialViscosity stays above 1 % at step 3)
        vel[:, 1] += F(LIFT)
        fluids.append(dict(pos=pos, vel=vel, vol=_volumes(len(pos), 35 + k), density0=rho0))
    return dict(fluids=fluids, floor=_floor(14, 13))


def scene_v():
    """The mildly perturbed sheared block of golden_scenes.scene_dfsph_viscous (jitter 0.02 r; DFSPHViscosity's loop diverges on
    rougher input in the reference too), 8^3 particles, no boundary."""
    pos = scenes.jitter(scenes.cube_fluid_positions(8, 8, 8, R), 0.02 * R, seed=42)
    vel = scenes.random_velocities(len(pos), 0.01, seed=12345)
    vel[:, 0] += F(2.0) * pos[:, 1]
    return dict(fluids=[dict(pos=pos, vel=vel, vol=None, density0=1000.0)], floor=None)


SCENES = {"A": scene_a, "A2": lambda: scene_a(coincident=True), "B": scene_b, "V": scene_v}

# name -> the description with both arms on; arms(desc) switches them
FORCES = {
    "xsph": ("xsph", 0.5, 0.3),
    "artificial": ("artificial", 0.8, 0.4, 1.5, 0.5, 8.0),
    "akinci": ("akinci2013", 1.0, 10.0),
    "he2014": ("he2014", 1.0, 0.5),
    "wcsph": ("wcsph", 0.3),
}
TWO_ARMS = ("xsph", "artificial", "akinci2013", "he2014")


def arms(desc):
    """[(suffix, description)]: (c_f, c_b), (c_f, 0), (0, c_b) where the force has two arms"""
    if desc[0] not in TWO_ARMS:
        return [("", desc)]
    return [("", desc), ("-fluid", desc[:2] + (0.0,) + desc[3:]), ("-boundary", desc[:1] + (0.0,) + desc[2:])]


# `forces`: the built-in forces of fluid `target`, in list order, each between two probes
Case = namedtuple("Case", "id scene kernels target forces")


def _cases():
    out = []
    for name, desc in FORCES.items():  # scene A: Akinci's one-fluid fast path, the <DS> kernels
        for sfx, d in arms(desc):
            out.append(Case(f"A-{name}{sfx}", "A", ("cubic", "cubic"), 0, (d,)))
    for target in (1, 0):              # scene B: the general kernels and the i_model == j_model filter
        for name, desc in FORCES.items():
            for sfx, d in arms(desc):
                out.append(Case(f"B{target}-{name}{sfx}", "B", ("cubic", "cubic"), target, (d,)))
    for target in (1, 0):              # scene B with <poly6, spiky>: weights and gradients from the world's kernel pair
        for name in ("akinci", "he2014", "artificial"):
            for sfx, d in arms(FORCES[name]):
                out.append(Case(f"B{target}p-{name}{sfx}", "B", ("poly6", "spiky"), target, (d,)))
    out.append(Case("A2-xsph+akinci", "A2", ("cubic", "cubic"), 0, (FORCES["xsph"], FORCES["akinci"])))
    for iters in (1, 3):
        out.append(Case(f"V-visc{iters}", "V", ("cubic", "cubic"), 0, (("dfsph_viscosity", 0.6, iters, iters, 0.01),)))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
KERNEL_KINDS = {"cubic": 0, "poly6": 1, "spiky": 2, "viscosity": 3}


# ---------------------------------------------------------------------------------------------------- the CPU oracle
def run_oracle(case, f64, shuffle_seed=0, nsteps=NSTEPS):
    """The scene in the oracle, a recording custom force in front of and behind every built-in force of the target fluid.
    Returns, per step, the list of records the probes made (len(case.forces) + 1 of them): dict(acc, pos, vel, rho of the target
    fluid, others = [(pos, vel, rho)] of every fluid, vol of every fluid, bvol, bforce, dt, inv_dt)."""
    from oracle import oracle as O

    sc = SCENES[case.scene]()
    o = O.OracleWorld(R, 2.0, O.DFSPH, f64=f64)
    if shuffle_seed:
        o.set_shuffle_seed(shuffle_seed)
    o.set_kernels(KERNEL_KINDS[case.kernels[0]], KERNEL_KINDS[case.kernels[1]])
    nf = len(sc["fluids"])
    steps, current = [], []

    def probe(world, f, pos, vel, dens, acc):
        rec = dict(acc=acc.copy(), dt=world.timestep()[0], inv_dt=world.timestep()[1], fluids=[])
        for g in range(nf):
            if g == f:
                rec["fluids"].append((pos.copy(), vel.copy(), dens.copy()))
            else:
                rec["fluids"].append((world.fluid_vec(g, "positions"), world.fluid_vec(g, "velocities"), world.fluid_scalar(g, "densities")))
        rec["vol"] = [world.fluid_scalar(g, "volumes") for g in range(nf)]
        if sc["floor"] is not None:
            rec["bvol"], rec["bforce"] = world.boundary_volumes(0), world.boundary_vec(0, "forces")
        current.append(rec)

    for g, fl in enumerate(sc["fluids"]):
        fid = o.add_fluid(fl["pos"], fl["density0"], fl["vel"])
        assert fid == g
        if fl["vol"] is not None:
            o.set_fluid_volumes(fid, fl["vol"])
        if g != case.target:
            continue
        o.add_custom_force(fid, probe)
        for d in case.forces:
            {"xsph": o.add_xsph, "artificial": o.add_artificial_viscosity, "akinci2013": o.add_akinci2013, "he2014": o.add_he2014,
             "wcsph": lambda f, t: o.add_wcsph_tension(f, t, 0.0), "dfsph_viscosity": o.add_dfsph_viscosity}[d[0]](fid, *d[1:])
            o.add_custom_force(fid, probe)
    if sc["floor"] is not None:
        o.add_boundary(sc["floor"][0], sc["floor"][1], 1, 0xFFFFFFFF, True)
    for _ in range(nsteps):
        current = []
        o.step(DT, GRAVITY)
        assert len(current) == len(case.forces) + 1
        steps.append(current)
    visc = [o.viscosity_stats(case.target, 1 + 2 * k)[0] if d[0] == "dfsph_viscosity" else None for k, d in enumerate(case.forces)]
    return sc, steps, visc


def oracle_snapshot(case, sc, rec):
    """force_reading.Snapshot from a probe's record (all fluids' particles, fluid 0's first)"""
    from force_reading import Snapshot

    rho0 = [fl["density0"] for fl in sc["fluids"]]
    x = np.concatenate([p for p, _, _ in rec["fluids"]])
    v = np.concatenate([q for _, q, _ in rec["fluids"]])
    rho = np.concatenate([d for _, _, d in rec["fluids"]])
    m = np.concatenate([vol * r0 for vol, r0 in zip(rec["vol"], rho0)])
    model = np.concatenate([np.full(len(p), g) for g, (p, _, _) in enumerate(rec["fluids"])])
    acc = np.zeros_like(x)
    acc[model == case.target] = rec["acc"]
    if sc["floor"] is not None:
        xb, vb = sc["floor"][0].astype(np.float64), sc["floor"][1].astype(np.float64)
        volb = rec["bvol"]
    else:
        xb, vb, volb = np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0)
    h = float(F(R)) * 4.0  # the f64 build takes the radius as the f32 the C ABI hands over, widened
    return Snapshot(x, v, m, rho, model, rho0, acc, xb, vb, volb, np.zeros(len(xb), np.int64), h, case.kernels, rec["dt"], rec["inv_dt"])

//! Diffuse particles: spray, foam and bubbles after Ihmsen et al. 2012 (include/salva_hip.h "Diffuse particles").
//! `LiquidWorld::diffuse_potentials` reads out, per particle of the selected fluids and on the device, what whitewater is made from:
//! trapped air, wave crest, kinetic energy, the surface normal and the number of neighbours within h.  `LiquidWorld::create_diffuse`
//! makes a set of diffuse particles that lives on the device; `update_diffuse` advects, removes and emits after a step.
use crate::ffi;
use crate::liquid_world::{check, Error};
use nalgebra::{Point3, Vector3};
use salva3d::math::Real;

/// `SalvaHipDiffuse`.  `Default` is `salva_hip_default_diffuse`.
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct Diffuse {
    /// a particle has a normal when h |g| reaches this
    pub surface_min: Real,
    /// a crest moves along its normal at least this much: [-1, 1]
    pub crest_cos: Real,
    /// the clamp ranges (lo, hi) of the three potentials
    pub trapped_air: (Real, Real),
    pub wave_crest: (Real, Real),
    pub energy: (Real, Real),
    /// particles per unit of time at full potential
    pub k_ta: Real,
    pub k_wc: Real,
    pub max_per_particle: u32,
    /// spray below `n_spray` fluid neighbours, bubble above `n_bubble`, foam between
    pub n_spray: u32,
    pub n_bubble: u32,
    /// buoyancy and drag
    pub k_b: Real,
    pub k_d: Real,
    pub lifetime: (Real, Real),
    pub seed: u32,
    /// (lo, hi): a diffuse particle outside is removed
    pub kill_box: Option<([Real; 3], [Real; 3])>,
    /// what the world is stepped with
    pub gravity: [Real; 3],
}

impl Default for Diffuse {
    fn default() -> Self {
        Self {
            surface_min: 0.25, crest_cos: 0.6, trapped_air: (5.0, 20.0), wave_crest: (2.0, 8.0), energy: (5.0, 50.0), k_ta: 4000.0, k_wc: 50000.0,
            max_per_particle: 16, n_spray: 6, n_bubble: 20, k_b: 2.0, k_d: 0.8, lifetime: (2.0, 5.0), seed: 0, kill_box: None, gravity: [0.0, -9.81, 0.0],
        }
    }
}

impl Diffuse {
    pub(crate) fn raw(&self) -> ffi::SalvaHipDiffuse {
        let mut p: ffi::SalvaHipDiffuse = unsafe { std::mem::zeroed() };
        p.struct_size = ffi::SALVA_HIP_DIFFUSE_BYTES as u32;
        p.version = ffi::SALVA_HIP_DIFFUSE_VERSION as u32;
        p.surface_min = self.surface_min;
        p.crest_cos = self.crest_cos;
        (p.ta_lo, p.ta_hi) = self.trapped_air;
        (p.wc_lo, p.wc_hi) = self.wave_crest;
        (p.en_lo, p.en_hi) = self.energy;
        p.k_ta = self.k_ta;
        p.k_wc = self.k_wc;
        p.max_per_particle = self.max_per_particle;
        p.n_spray = self.n_spray;
        p.n_bubble = self.n_bubble;
        p.k_b = self.k_b;
        p.k_d = self.k_d;
        (p.life_lo, p.life_hi) = self.lifetime;
        p.seed = self.seed;
        p.gravity = self.gravity;
        if let Some((lo, hi)) = self.kill_box {
            p.has_kill_box = 1;
            p.kill_lo = lo;
            p.kill_hi = hi;
        }
        p
    }
}

/// Per particle of the selected fluids, by slot and then by index.
#[derive(Clone, Debug, Default)]
pub struct DiffusePotentials {
    pub trapped_air: Vec<Real>,
    pub wave_crest: Vec<Real>,
    pub energy: Vec<Real>,
    /// the zero vector where the particle is not at the surface
    pub normal: Vec<Vector3<Real>>,
    /// neighbours within h, the particle itself not counted
    pub count: Vec<u32>,
}

pub(crate) fn potentials(world: *mut ffi::SalvaHipWorld, fluid_mask: u32, params: &Diffuse) -> Result<DiffusePotentials, Error> {
    let p = params.raw();
    let mut n = 0u64;
    check(unsafe { ffi::salva_hip_diffuse_potentials(world, fluid_mask, &p, 0, std::ptr::null(), &mut n) })?;
    let rows = n as usize;
    let room = rows.max(1);
    let (mut ta, mut wc, mut en, mut nrm, mut count) =
        (vec![0.0 as Real; room], vec![0.0 as Real; room], vec![0.0 as Real; room], vec![0.0 as Real; 3 * room], vec![0u32; room]);
    let out = ffi::SalvaHipDiffusePotentialsOut {
        trapped_air: ta.as_mut_ptr(), wave_crest: wc.as_mut_ptr(), energy: en.as_mut_ptr(), normal: nrm.as_mut_ptr(), count: count.as_mut_ptr(),
        row_capacity: n,
    };
    check(unsafe { ffi::salva_hip_diffuse_potentials(world, fluid_mask, &p, 0, &out, &mut n) })?;
    ta.truncate(rows);
    wc.truncate(rows);
    en.truncate(rows);
    count.truncate(rows);
    Ok(DiffusePotentials {
        trapped_air: ta, wave_crest: wc, energy: en, count,
        normal: nrm.chunks_exact(3).take(rows).map(|c| Vector3::new(c[0], c[1], c[2])).collect(),
    })
}

/// A diffuse set of a world (`salva_hip_create_diffuse`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct DiffuseHandle(pub(crate) u32);

/// The particles of a set in the order of creation.  kind: 0 spray, 1 foam, 2 bubble, 3 new.
#[derive(Clone, Debug, Default)]
pub struct DiffuseParticles {
    pub positions: Vec<Point3<Real>>,
    pub velocities: Vec<Vector3<Real>>,
    pub lifetime: Vec<Real>,
    pub kind: Vec<u32>,
    pub id: Vec<u32>,
}

pub(crate) fn create(world: *mut ffi::SalvaHipWorld, capacity: u64) -> Result<DiffuseHandle, Error> {
    let mut h = 0u32;
    check(unsafe { ffi::salva_hip_create_diffuse(world, capacity, &mut h) })?;
    Ok(DiffuseHandle(h))
}

pub(crate) fn add(world: *mut ffi::SalvaHipWorld, set: DiffuseHandle, positions: &[Point3<Real>], velocities: &[Vector3<Real>],
                  lifetimes: Option<&[Real]>) -> Result<(), Error> {
    assert!(velocities.len() == positions.len() && lifetimes.map_or(true, |l| l.len() == positions.len()), "one velocity (and lifetime) per position");
    let x: Vec<Real> = positions.iter().flat_map(|p| [p.x, p.y, p.z]).collect();
    let v: Vec<Real> = velocities.iter().flat_map(|p| [p.x, p.y, p.z]).collect();
    let life = lifetimes.map_or(std::ptr::null(), |l| l.as_ptr());
    check(unsafe { ffi::salva_hip_add_diffuse(world, set.0, positions.len() as u64, x.as_ptr(), v.as_ptr(), life, 0) })
}

pub(crate) fn update(world: *mut ffi::SalvaHipWorld, set: DiffuseHandle, fluid_mask: u32, params: &Diffuse, dt: Real) -> Result<(), Error> {
    let p = params.raw();
    check(unsafe { ffi::salva_hip_update_diffuse(world, set.0, fluid_mask, &p, dt) })
}

pub(crate) fn get(world: *mut ffi::SalvaHipWorld, set: DiffuseHandle) -> Result<DiffuseParticles, Error> {
    let mut n = 0u64;
    check(unsafe { ffi::salva_hip_get_diffuse(world, set.0, 0, std::ptr::null(), &mut n) })?;
    let rows = n as usize;
    let room = rows.max(1);
    let (mut x, mut v, mut life, mut kind, mut id) =
        (vec![0.0 as Real; 3 * room], vec![0.0 as Real; 3 * room], vec![0.0 as Real; room], vec![0u32; room], vec![0u32; room]);
    let out = ffi::SalvaHipDiffuseOut {
        positions: x.as_mut_ptr(), velocities: v.as_mut_ptr(), lifetime: life.as_mut_ptr(), kind: kind.as_mut_ptr(), id: id.as_mut_ptr(), row_capacity: n,
    };
    check(unsafe { ffi::salva_hip_get_diffuse(world, set.0, 0, &out, &mut n) })?;
    life.truncate(rows);
    kind.truncate(rows);
    id.truncate(rows);
    Ok(DiffuseParticles {
        positions: x.chunks_exact(3).take(rows).map(|c| Point3::new(c[0], c[1], c[2])).collect(),
        velocities: v.chunks_exact(3).take(rows).map(|c| Vector3::new(c[0], c[1], c[2])).collect(),
        lifetime: life, kind, id,
    })
}

pub(crate) fn stats(world: *mut ffi::SalvaHipWorld, set: DiffuseHandle) -> Result<ffi::SalvaHipDiffuseStats, Error> {
    let mut st: ffi::SalvaHipDiffuseStats = unsafe { std::mem::zeroed() };
    check(unsafe { ffi::salva_hip_get_diffuse_stats(world, set.0, &mut st) })?;
    Ok(st)
}

pub(crate) fn clear(world: *mut ffi::SalvaHipWorld, set: DiffuseHandle) -> Result<(), Error> {
    check(unsafe { ffi::salva_hip_clear_diffuse(world, set.0) })
}

pub(crate) fn destroy(world: *mut ffi::SalvaHipWorld, set: DiffuseHandle) -> Result<(), Error> {
    check(unsafe { ffi::salva_hip_destroy_diffuse(world, set.0) })
}

//! SPH fields at points and on a lattice (`salva_hip_evaluate_fields` / `_lattice`, include/salva_hip.h): the fluid as a
//! continuum, summed on the device over the particles as they are now.  `LiquidWorld::evaluate_fields` / `evaluate_lattice` return a
//! `Fields`; the vectors of the fields not asked for stay empty, `velocity` / `gradient` hold one vector per place, and a lattice's node
//! (ix, iy, iz) is at index (ix * ny + iy) * nz + iz.
use crate::ffi;
use crate::liquid_world::{check, Error};
use nalgebra::{Point3, Vector3};
use salva3d::math::Real;

/// Which fields to compute.
#[derive(Clone, Copy, Debug, Default)]
pub struct FieldSet {
    pub density: bool,
    pub fraction: bool,
    pub velocity: bool,
    pub gradient: bool,
    pub count: bool,
}

impl FieldSet {
    pub fn density() -> Self {
        Self { density: true, ..Self::default() }
    }
    pub fn all() -> Self {
        Self { density: true, fraction: true, velocity: true, gradient: true, count: true }
    }
}

#[derive(Clone, Debug, Default)]
pub struct Fields {
    /// sum_j m_j W(x - x_j)
    pub density: Vec<Real>,
    /// sum_j V_j W(x - x_j)
    pub fraction: Vec<Real>,
    /// sum_j m_j v_j W / sum_j m_j W; zero where the denominator is zero
    pub velocity: Vec<Vector3<Real>>,
    /// sum_j m_j grad W(x - x_j)
    pub gradient: Vec<Vector3<Real>>,
    /// particles with |d|^2 <= h^2
    pub count: Vec<u32>,
}

struct Buffers {
    density: Vec<Real>,
    fraction: Vec<Real>,
    velocity: Vec<Real>,
    gradient: Vec<Real>,
    count: Vec<u32>,
}

impl Buffers {
    fn new(m: usize, want: FieldSet) -> Self {
        let room = |on: bool, width: usize| if on { vec![0.0 as Real; (m * width).max(1)] } else { Vec::new() };
        Self {
            density: room(want.density, 1),
            fraction: room(want.fraction, 1),
            velocity: room(want.velocity, 3),
            gradient: room(want.gradient, 3),
            count: if want.count { vec![0u32; m.max(1)] } else { Vec::new() },
        }
    }
    fn raw(&mut self) -> ffi::SalvaHipFieldOut {
        fn ptr<T>(v: &mut Vec<T>) -> *mut T {
            if v.is_empty() { std::ptr::null_mut() } else { v.as_mut_ptr() }
        }
        ffi::SalvaHipFieldOut {
            density: ptr(&mut self.density),
            fraction: ptr(&mut self.fraction),
            velocity: ptr(&mut self.velocity),
            gradient: ptr(&mut self.gradient),
            count: ptr(&mut self.count),
        }
    }
    fn finish(mut self, m: usize) -> Fields {
        let vectors = |v: &[Real]| v.chunks_exact(3).take(m).map(|c| Vector3::new(c[0], c[1], c[2])).collect::<Vec<_>>();
        self.density.truncate(m);
        self.fraction.truncate(m);
        self.count.truncate(m);
        Fields { velocity: vectors(&self.velocity), gradient: vectors(&self.gradient), density: self.density, fraction: self.fraction, count: self.count }
    }
}

/// The parameters of the anisotropic kernels (`SalvaHipAnisotropy`, include/salva_hip.h "Anisotropic kernels"),
/// lengths in units of h.  `Default` is `salva_hip_default_anisotropy`.
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct Anisotropy {
    /// how far a centre moves towards the weighted mean of its neighbourhood: [0, 1]
    pub lambda: Real,
    /// the largest ratio of two eigenvalues: >= 1
    pub k_r: Real,
    pub k_s: Real,
    /// the stretch of an isolated particle
    pub k_n: Real,
    /// a particle with at most this many neighbours is isolated
    pub n_eps: u32,
}

impl Default for Anisotropy {
    fn default() -> Self {
        Self { lambda: 0.9, k_r: 4.0, k_s: 5.0 / 3.0, k_n: 0.5, n_eps: 25 }
    }
}

impl Anisotropy {
    pub(crate) fn raw(&self) -> ffi::SalvaHipAnisotropy {
        let mut p: ffi::SalvaHipAnisotropy = unsafe { std::mem::zeroed() };
        p.struct_size = ffi::SALVA_HIP_ANISOTROPY_BYTES as u32;
        p.version = ffi::SALVA_HIP_ANISOTROPY_VERSION as u32;
        p.lambda = self.lambda;
        p.k_r = self.k_r;
        p.k_s = self.k_s;
        p.k_n = self.k_n;
        p.n_eps = self.n_eps;
        p
    }
}

/// Per particle of the selected fluids, by slot and then by index: the smoothed centre, the metric G as (xx, xy, xz, yy, yz, zz) and
/// the number of neighbours within 2h.
#[derive(Clone, Debug, Default)]
pub struct AnisotropyRows {
    pub centres: Vec<Point3<Real>>,
    pub metric: Vec<[Real; 6]>,
    pub count: Vec<u32>,
}

pub(crate) fn compute_anisotropy(world: *mut ffi::SalvaHipWorld, fluid_mask: u32, params: &Anisotropy) -> Result<AnisotropyRows, Error> {
    let p = params.raw();
    let mut n = 0u64;
    check(unsafe { ffi::salva_hip_compute_anisotropy(world, fluid_mask, &p, 0, std::ptr::null(), &mut n) })?;
    let rows = n as usize;
    let (mut centres, mut metric, mut count) = (vec![0.0 as Real; 3 * rows.max(1)], vec![0.0 as Real; 6 * rows.max(1)], vec![0u32; rows.max(1)]);
    let out = ffi::SalvaHipAnisotropyOut { centres: centres.as_mut_ptr(), metric: metric.as_mut_ptr(), count: count.as_mut_ptr(), row_capacity: n };
    check(unsafe { ffi::salva_hip_compute_anisotropy(world, fluid_mask, &p, 0, &out, &mut n) })?;
    count.truncate(rows);
    Ok(AnisotropyRows {
        centres: centres.chunks_exact(3).take(rows).map(|c| Point3::new(c[0], c[1], c[2])).collect(),
        metric: metric.chunks_exact(6).take(rows).map(|c| [c[0], c[1], c[2], c[3], c[4], c[5]]).collect(),
        count,
    })
}

/// The anisotropic fields are density, fraction and gradient: `want.velocity` and `want.count` must be false.
fn anisotropic_out(bufs: &mut Buffers, want: FieldSet) -> ffi::SalvaHipAnisoFieldOut {
    assert!(!want.velocity && !want.count, "the anisotropic fields are density, fraction and gradient");
    let raw = bufs.raw();
    ffi::SalvaHipAnisoFieldOut { density: raw.density, fraction: raw.fraction, gradient: raw.gradient }
}

pub(crate) fn evaluate_points_anisotropic(
    world: *mut ffi::SalvaHipWorld, fluid_mask: u32, params: &Anisotropy, points: &[Point3<Real>], want: FieldSet,
) -> Result<Fields, Error> {
    let xyz: Vec<Real> = points.iter().flat_map(|p| [p.x, p.y, p.z]).collect();
    let mut bufs = Buffers::new(points.len(), want);
    let out = anisotropic_out(&mut bufs, want);
    let p = params.raw();
    check(unsafe { ffi::salva_hip_evaluate_fields_anisotropic(world, fluid_mask, &p, points.len() as u64, xyz.as_ptr(), 0, &out) })?;
    Ok(bufs.finish(points.len()))
}

pub(crate) fn evaluate_lattice_anisotropic(
    world: *mut ffi::SalvaHipWorld, fluid_mask: u32, params: &Anisotropy, origin: &Point3<Real>, spacing: Real, dims: [u32; 3], want: FieldSet,
) -> Result<Fields, Error> {
    let nodes = dims.iter().try_fold(1u64, |a, &d| a.checked_mul(d as u64)).filter(|&m| m <= 1u64 << 32);
    let m = nodes.unwrap_or(0) as usize;
    let mut bufs = Buffers::new(m, want);
    let out = anisotropic_out(&mut bufs, want);
    let o = [origin.x, origin.y, origin.z];
    let p = params.raw();
    check(unsafe { ffi::salva_hip_evaluate_fields_anisotropic_lattice(world, fluid_mask, &p, o.as_ptr(), spacing, dims.as_ptr(), 0, &out) })?;
    Ok(bufs.finish(m))
}

/// `fluid_mask`: bit s selects the fluid in slot s.
pub(crate) fn evaluate_points(world: *mut ffi::SalvaHipWorld, fluid_mask: u32, points: &[Point3<Real>], want: FieldSet) -> Result<Fields, Error> {
    let xyz: Vec<Real> = points.iter().flat_map(|p| [p.x, p.y, p.z]).collect();
    let mut bufs = Buffers::new(points.len(), want);
    let out = bufs.raw();
    check(unsafe { ffi::salva_hip_evaluate_fields(world, fluid_mask, points.len() as u64, xyz.as_ptr(), 0, &out) })?;
    Ok(bufs.finish(points.len()))
}

pub(crate) fn evaluate_lattice(
    world: *mut ffi::SalvaHipWorld, fluid_mask: u32, origin: &Point3<Real>, spacing: Real, dims: [u32; 3], want: FieldSet,
) -> Result<Fields, Error> {
    let nodes = dims.iter().try_fold(1u64, |a, &d| a.checked_mul(d as u64)).filter(|&m| m <= 1u64 << 32);
    // (beyond 2^32 nodes the library refuses before it writes: nothing to allocate for)
    let m = nodes.unwrap_or(0) as usize;
    let mut bufs = Buffers::new(m, want);
    let out = bufs.raw();
    let o = [origin.x, origin.y, origin.z];
    check(unsafe { ffi::salva_hip_evaluate_fields_lattice(world, fluid_mask, o.as_ptr(), spacing, dims.as_ptr(), 0, &out) })?;
    Ok(bufs.finish(m))
}

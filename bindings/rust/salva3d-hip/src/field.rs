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

//! Rays cast at the fluid's particles (`salva_hip_cast_rays` / `_cast_rays_camera`, include/salva_hip.h): every particle
//! of the selected fluids is a sphere of `radius`, and a ray is asked for its first hit — `t` in units of |d| (+inf: a miss), the
//! particle (`fluid`, `index`; `u32::MAX`: a miss), the sphere's normal there — and for the thickness of fluid along it.
//! `LiquidWorld::cast_rays` / `cast_camera` return a `RayHits`; the vectors not asked for stay empty, and a camera's pixel (ix, iy)
//! is at index iy * width + ix.
use crate::ffi;
use crate::liquid_world::{check, Error};
use nalgebra::{Point3, Vector3};
use salva3d::math::Real;

/// What to compute: the first hit (t, fluid, index), its normal, the thickness.
#[derive(Clone, Copy, Debug)]
pub struct RaySet {
    pub hit: bool,
    pub normal: bool,
    pub thickness: bool,
}

impl Default for RaySet {
    fn default() -> Self {
        Self { hit: true, normal: false, thickness: false }
    }
}

/// `radius`: None = the world's particle radius (at most h / 2).  `clip`: only the particles in that box (faces included) are seen.
#[derive(Clone, Copy, Debug)]
pub struct RayOptions {
    pub radius: Option<Real>,
    pub tmax: Real,
    pub fluid_mask: u32,
    pub clip: Option<(Point3<Real>, Point3<Real>)>,
}

impl Default for RayOptions {
    fn default() -> Self {
        Self { radius: None, tmax: Real::INFINITY, fluid_mask: u32::MAX, clip: None }
    }
}

/// Pixel (ix, iy) casts `forward + su * right + sv * up` from `origin`, su = (ix + 0.5) * 2 / width - 1 and sv likewise.
#[derive(Clone, Copy, Debug)]
pub struct RayCamera {
    pub origin: Point3<Real>,
    pub forward: Vector3<Real>,
    pub right: Vector3<Real>,
    pub up: Vector3<Real>,
    pub width: u32,
    pub height: u32,
}

#[derive(Clone, Debug, Default)]
pub struct RayHits {
    pub t: Vec<Real>,
    pub fluid: Vec<u32>,
    pub index: Vec<u32>,
    pub normal: Vec<Vector3<Real>>,
    pub thickness: Vec<Real>,
}

struct Buffers {
    t: Vec<Real>,
    fluid: Vec<u32>,
    index: Vec<u32>,
    normal: Vec<Real>,
    thickness: Vec<Real>,
}

impl Buffers {
    fn new(m: usize, want: RaySet) -> Self {
        let room = |on: bool, width: usize| if on { vec![0.0 as Real; (m * width).max(1)] } else { Vec::new() };
        let ids = |on: bool| if on { vec![0u32; m.max(1)] } else { Vec::new() };
        Self { t: room(want.hit, 1), fluid: ids(want.hit), index: ids(want.hit), normal: room(want.normal, 3), thickness: room(want.thickness, 1) }
    }
    fn raw(&mut self) -> ffi::SalvaHipRayOut {
        fn ptr<T>(v: &mut Vec<T>) -> *mut T {
            if v.is_empty() { std::ptr::null_mut() } else { v.as_mut_ptr() }
        }
        ffi::SalvaHipRayOut {
            t: ptr(&mut self.t),
            fluid: ptr(&mut self.fluid),
            index: ptr(&mut self.index),
            normal: ptr(&mut self.normal),
            thickness: ptr(&mut self.thickness),
        }
    }
    fn finish(mut self, m: usize) -> RayHits {
        let normal = self.normal.chunks_exact(3).take(m).map(|c| Vector3::new(c[0], c[1], c[2])).collect::<Vec<_>>();
        self.t.truncate(m);
        self.fluid.truncate(m);
        self.index.truncate(m);
        self.thickness.truncate(m);
        RayHits { t: self.t, fluid: self.fluid, index: self.index, normal, thickness: self.thickness }
    }
}

fn params(opt: &RayOptions, particle_radius: Real) -> ffi::SalvaHipRayParams {
    let (lo, hi) = opt.clip.map_or(([0.0; 3], [0.0; 3]), |(lo, hi)| ([lo.x, lo.y, lo.z], [hi.x, hi.y, hi.z]));
    ffi::SalvaHipRayParams {
        struct_size: ffi::SALVA_HIP_RAY_PARAMS_BYTES as u32,
        version: ffi::SALVA_HIP_RAY_VERSION as u32,
        radius: opt.radius.unwrap_or(particle_radius),
        tmax: opt.tmax,
        has_clip: opt.clip.is_some() as u32,
        clip_lo: lo,
        clip_hi: hi,
        reserved: [0; 5],
    }
}

pub(crate) fn cast_rays(
    world: *mut ffi::SalvaHipWorld, particle_radius: Real, origins: &[Point3<Real>], directions: &[Vector3<Real>], want: RaySet, opt: &RayOptions,
) -> Result<RayHits, Error> {
    if origins.len() != directions.len() {
        return Err(Error { code: ffi::SALVA_HIP_E_INVALID, message: "cast_rays: as many directions as origins".into() });
    }
    let o: Vec<Real> = origins.iter().flat_map(|p| [p.x, p.y, p.z]).collect();
    let d: Vec<Real> = directions.iter().flat_map(|v| [v.x, v.y, v.z]).collect();
    let p = params(opt, particle_radius);
    let mut bufs = Buffers::new(origins.len(), want);
    let out = bufs.raw();
    check(unsafe { ffi::salva_hip_cast_rays(world, opt.fluid_mask, &p, origins.len() as u64, o.as_ptr(), d.as_ptr(), 0, &out) })?;
    Ok(bufs.finish(origins.len()))
}

pub(crate) fn cast_camera(world: *mut ffi::SalvaHipWorld, particle_radius: Real, camera: &RayCamera, want: RaySet, opt: &RayOptions) -> Result<RayHits, Error> {
    let rays = (camera.width as u64) * (camera.height as u64);
    // (beyond 2^32 rays the library refuses before it writes: nothing to allocate for)
    let m = if rays <= 1u64 << 32 { rays as usize } else { 0 };
    let p = params(opt, particle_radius);
    let c = ffi::SalvaHipRayCamera {
        struct_size: ffi::SALVA_HIP_RAY_CAMERA_BYTES as u32,
        version: ffi::SALVA_HIP_RAY_VERSION as u32,
        origin: [camera.origin.x, camera.origin.y, camera.origin.z],
        forward: [camera.forward.x, camera.forward.y, camera.forward.z],
        right: [camera.right.x, camera.right.y, camera.right.z],
        up: [camera.up.x, camera.up.y, camera.up.z],
        width: camera.width,
        height: camera.height,
    };
    let mut bufs = Buffers::new(m, want);
    let out = bufs.raw();
    check(unsafe { ffi::salva_hip_cast_rays_camera(world, opt.fluid_mask, &p, &c, 0, &out) })?;
    Ok(bufs.finish(m))
}

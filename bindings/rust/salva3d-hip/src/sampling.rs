//! `salva3d::sampling::{shape_surface_ray_sample, shape_volume_ray_sample}` (src/sampling/ray_sampling.rs:9-24) over
//! `salva_hip_sample_shape` / `salva_hip_sample_host_shape`: the reference's two signatures, plus the world that supplies the
//! device and the stream.  Ball, cuboid, capsule (y) and cylinder (y) are sampled by closed-form casts on the device; every other
//! parry shape keeps its casts on the host (`cast_local_ray(ray, MAX, false)` per ray, in rounds), and the marked lattice is
//! expanded on the device.  Points come back in lexicographic lattice order (the reference's order is a HashSet's).
use crate::ffi;
use crate::liquid_world::check;
use crate::{Error, LiquidWorld};
use parry3d::query::{Ray, RayCast};
use parry3d::shape::Shape;
use salva3d::math::{Isometry, Point, Real, Vector};

fn analytic(shape: &dyn Shape) -> Option<ffi::SalvaHipShape> {
    if let Some(b) = shape.as_ball() {
        return Some(ffi::SalvaHipShape { kind: ffi::SALVA_HIP_SHAPE_BALL, params: [b.radius, 0.0, 0.0] });
    }
    if let Some(c) = shape.as_cuboid() {
        return Some(ffi::SalvaHipShape { kind: ffi::SALVA_HIP_SHAPE_CUBOID, params: [c.half_extents.x, c.half_extents.y, c.half_extents.z] });
    }
    if let Some(c) = shape.as_capsule() {
        // (only Capsule::new_y: a segment along the local y axis, centred on the origin)
        if c.segment.a.x == 0.0 && c.segment.a.z == 0.0 && c.segment.b.x == 0.0 && c.segment.b.z == 0.0 && c.segment.a.y == -c.segment.b.y {
            return Some(ffi::SalvaHipShape { kind: ffi::SALVA_HIP_SHAPE_CAPSULE, params: [c.segment.b.y.abs(), c.radius, 0.0] });
        }
    }
    if let Some(c) = shape.as_cylinder() {
        return Some(ffi::SalvaHipShape { kind: ffi::SALVA_HIP_SHAPE_CYLINDER, params: [c.half_height, c.radius, 0.0] });
    }
    None
}

unsafe extern "C" fn aabb_thunk(user: *mut std::ffi::c_void, mins: *mut f32, maxs: *mut f32) {
    let shape = &**(user as *const &dyn Shape);
    let aabb = shape.compute_aabb(&Isometry::identity());
    for a in 0..3 {
        *mins.add(a) = aabb.mins[a];
        *maxs.add(a) = aabb.maxs[a];
    }
}

unsafe extern "C" fn cast_thunk(user: *mut std::ffi::c_void, n: u32, origins: *const f32, axis: i32, toi: *mut f32) {
    let shape = &**(user as *const &dyn Shape);
    let mut dir = Vector::zeros();
    dir[axis as usize] = 1.0;
    for r in 0..n as usize {
        let o = Point::new(*origins.add(3 * r), *origins.add(3 * r + 1), *origins.add(3 * r + 2));
        *toi.add(r) = shape.cast_local_ray(&Ray::new(o, dir), Real::MAX, false).unwrap_or(-1.0);
    }
}

fn sample(world: &mut LiquidWorld, shape: &dyn Shape, particle_rad: Real, mode: i32) -> Result<Vec<Point<Real>>, Error> {
    let raw = world.raw();
    let analytic = analytic(shape);
    let user: *const &dyn Shape = &shape;
    let host = ffi::SalvaHipHostRayShape { user: user as *mut std::ffi::c_void, aabb: Some(aabb_thunk), cast: Some(cast_thunk) };
    let call = |capacity: u64, out: *mut f32| -> i64 {
        match &analytic {
            Some(s) => unsafe { ffi::salva_hip_sample_shape(raw, s, particle_rad, mode, capacity, out) },
            None => unsafe { ffi::salva_hip_sample_host_shape(raw, &host, particle_rad, mode, capacity, out) },
        }
    };
    let n = call(0, std::ptr::null_mut());
    if n < 0 {
        check(n as i32)?;
    }
    let mut pts = vec![Point::<Real>::origin(); n as usize];
    if n > 0 {
        let m = call(n as u64, pts.as_mut_ptr() as *mut f32);
        if m < 0 {
            check(m as i32)?;
        }
    }
    Ok(pts)
}

/// Samples the surface of `shape` with a method based on ray-casting (ray_sampling.rs:9-15).
pub fn shape_surface_ray_sample<S: Shape>(world: &mut LiquidWorld, shape: &S, particle_rad: Real) -> Option<Vec<Point<Real>>> {
    sample(world, shape, particle_rad, ffi::SALVA_HIP_SAMPLE_SURFACE).ok()
}

/// Samples the volume of `shape` with a method based on ray-casting (ray_sampling.rs:18-24).
pub fn shape_volume_ray_sample<S: Shape>(world: &mut LiquidWorld, shape: &S, particle_rad: Real) -> Option<Vec<Point<Real>>> {
    sample(world, shape, particle_rad, ffi::SALVA_HIP_SAMPLE_VOLUME).ok()
}

/// A triangle mesh (parry `TriMesh`) or height field (parry `HeightField`) on the device (`salva_hip_create_mesh` /
/// `salva_hip_create_heightfield`).  Belongs to the world it was created in; `destroy` hands it back (refused while a
/// dynamically sampled boundary still uses it), and the world's end releases whatever is left.
pub struct Mesh {
    id: u32,
}

impl Mesh {
    /// `oriented`: the mesh is closed and wound counter-clockwise seen from outside (only such a mesh has an inside).
    pub fn new(world: &mut LiquidWorld, vertices: &[Point<Real>], indices: &[[u32; 3]], oriented: bool) -> Result<Mesh, Error> {
        let mut id = 0u32;
        let flags = if oriented { ffi::SALVA_HIP_MESH_ORIENTED as u32 } else { 0 };
        check(unsafe {
            ffi::salva_hip_create_mesh(world.raw(), vertices.as_ptr() as *const f32, vertices.len() as u32, indices.as_ptr() as *const u32, indices.len() as u32, flags, &mut id)
        })?;
        Ok(Mesh { id })
    }

    /// `HeightField::new(heights, scale)`: `heights` row-major, rows along z.
    pub fn heightfield(world: &mut LiquidWorld, heights: &[Real], nrows: u32, ncols: u32, scale: Vector<Real>) -> Result<Mesh, Error> {
        assert_eq!(heights.len(), nrows as usize * ncols as usize);
        let mut id = 0u32;
        let s = [scale.x, scale.y, scale.z];
        check(unsafe { ffi::salva_hip_create_heightfield(world.raw(), heights.as_ptr(), nrows, ncols, s.as_ptr(), &mut id) })?;
        Ok(Mesh { id })
    }

    pub fn id(&self) -> u32 {
        self.id
    }

    pub fn destroy(self, world: &mut LiquidWorld) -> Result<(), Error> {
        check(unsafe { ffi::salva_hip_destroy_mesh(world.raw(), self.id) })
    }
}

/// One part of a [`Compound`]: a built-in shape (`ffi::SalvaHipShape`: ball, cuboid, capsule (y), cylinder) or a [`Mesh`] of the same
/// world, with its pose in the compound's frame.
pub enum CompoundPartShape<'a> {
    Shape(ffi::SalvaHipShape),
    Mesh(&'a Mesh),
}

/// parry's `Compound` on the device (`salva_hip_create_compound`): 1 to 64 posed parts.  From a parry compound: one
/// part per `(part_pos, shape)` of `compound.shapes()`, a convex part handed over as the oriented triangle mesh of its hull.  Belongs
/// to the world it was created in; `destroy` hands it back (refused while a dynamically sampled boundary still uses it).  Ray
/// sampling of a compound is on the device as well: `surface_ray_sample` / `volume_ray_sample`.
pub struct Compound {
    id: u32,
}

impl Compound {
    pub fn new(world: &mut LiquidWorld, parts: &[(CompoundPartShape, Isometry<Real>)]) -> Result<Compound, Error> {
        let raw: Vec<ffi::SalvaHipCompoundPart> = parts
            .iter()
            .map(|(shape, pos)| {
                let (kind, params, mesh) = match shape {
                    CompoundPartShape::Shape(s) => (s.kind, s.params, 0),
                    CompoundPartShape::Mesh(m) => (ffi::SALVA_HIP_SHAPE_MESH, [0.0; 3], m.id()),
                };
                let q = pos.rotation.coords;
                ffi::SalvaHipCompoundPart { kind, params, mesh, translation: [pos.translation.x, pos.translation.y, pos.translation.z], rotation_ijkw: [q.x, q.y, q.z, q.w] }
            })
            .collect();
        let mut id = 0u32;
        check(unsafe { ffi::salva_hip_create_compound(world.raw(), raw.as_ptr(), raw.len() as u32, &mut id) })?;
        Ok(Compound { id })
    }

    pub fn id(&self) -> u32 {
        self.id
    }

    pub fn destroy(self, world: &mut LiquidWorld) -> Result<(), Error> {
        check(unsafe { ffi::salva_hip_destroy_compound(world.raw(), self.id) })
    }

    fn ray_sample(&self, world: &mut LiquidWorld, particle_rad: Real, mode: i32) -> Result<Vec<Point<Real>>, Error> {
        let raw = world.raw();
        let n = unsafe { ffi::salva_hip_sample_compound(raw, self.id, particle_rad, mode, 0, std::ptr::null_mut()) };
        if n < 0 {
            check(n as i32)?;
        }
        let mut pts = vec![Point::<Real>::origin(); n as usize];
        if n > 0 {
            let m = unsafe { ffi::salva_hip_sample_compound(raw, self.id, particle_rad, mode, n as u64, pts.as_mut_ptr() as *mut f32) };
            if m < 0 {
                check(m as i32)?;
            }
        }
        Ok(pts)
    }

    /// `shape_surface_ray_sample(&compound, particle_rad)` on the device (`salva_hip_sample_compound`): one thread per lattice ray
    /// casts at every part in the part's own frame, no host casts.
    pub fn surface_ray_sample(&self, world: &mut LiquidWorld, particle_rad: Real) -> Option<Vec<Point<Real>>> {
        self.ray_sample(world, particle_rad, ffi::SALVA_HIP_SAMPLE_SURFACE).ok()
    }

    /// `shape_volume_ray_sample(&compound, particle_rad)` on the device.
    pub fn volume_ray_sample(&self, world: &mut LiquidWorld, particle_rad: Real) -> Option<Vec<Point<Real>>> {
        self.ray_sample(world, particle_rad, ffi::SALVA_HIP_SAMPLE_VOLUME).ok()
    }
}

fn sample_mesh(world: &mut LiquidWorld, mesh: &Mesh, particle_rad: Real, mode: i32) -> Result<Vec<Point<Real>>, Error> {
    let raw = world.raw();
    let n = unsafe { ffi::salva_hip_sample_mesh(raw, mesh.id, particle_rad, mode, 0, std::ptr::null_mut()) };
    if n < 0 {
        check(n as i32)?;
    }
    let mut pts = vec![Point::<Real>::origin(); n as usize];
    if n > 0 {
        let m = unsafe { ffi::salva_hip_sample_mesh(raw, mesh.id, particle_rad, mode, n as u64, pts.as_mut_ptr() as *mut f32) };
        if m < 0 {
            check(m as i32)?;
        }
    }
    Ok(pts)
}

/// `shape_surface_ray_sample` for a mesh on the device: one thread per ray, no host casts.
pub fn mesh_surface_ray_sample(world: &mut LiquidWorld, mesh: &Mesh, particle_rad: Real) -> Option<Vec<Point<Real>>> {
    sample_mesh(world, mesh, particle_rad, ffi::SALVA_HIP_SAMPLE_SURFACE).ok()
}

/// `shape_volume_ray_sample` for a mesh on the device.
pub fn mesh_volume_ray_sample(world: &mut LiquidWorld, mesh: &Mesh, particle_rad: Real) -> Option<Vec<Point<Real>>> {
    sample_mesh(world, mesh, particle_rad, ffi::SALVA_HIP_SAMPLE_VOLUME).ok()
}

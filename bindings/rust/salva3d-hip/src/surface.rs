//! The iso-surface of a field as an indexed triangle mesh (`salva_hip_extract_surface` / `_from_values`, `salva_hip_get_fluid_bounds`,
//! include/salva_hip.h), extracted on the device by marching tetrahedra.  `LiquidWorld::extract_surface` makes the
//! count call, then the fill call, and returns a `SurfaceMesh`; the order of its vertices and triangles is fixed by the header's
//! contract, `normals` / `velocities` stay empty unless asked for.
use crate::ffi;
use crate::liquid_world::{check, Error};
use nalgebra::{Point3, Vector3};
use salva3d::math::Real;

/// Which field the surface is a level set of.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum SurfaceField {
    /// sum_j m_j W(x - x_j)
    Density,
    /// sum_j V_j W(x - x_j)
    Fraction,
}

#[derive(Clone, Debug, Default)]
pub struct SurfaceMesh {
    pub vertices: Vec<Point3<Real>>,
    /// unit, towards lower values; the zero vector where the gradient is zero
    pub normals: Vec<Vector3<Real>>,
    /// the evaluator's velocity at the vertices
    pub velocities: Vec<Vector3<Real>>,
    pub triangles: Vec<[u32; 3]>,
}

/// The count call, then the fill call: `call(out or null, counts)` returns the status.
fn fill(normals: bool, velocities: bool, call: impl Fn(*const ffi::SalvaHipSurfaceOut, *mut u64) -> i32) -> Result<SurfaceMesh, Error> {
    let mut counts = [0u64; 2];
    check(call(std::ptr::null(), counts.as_mut_ptr()))?;
    let (nv, nt) = (counts[0] as usize, counts[1] as usize);
    // (room the library can name even for an empty mesh)
    let mut vertices = vec![0.0 as Real; 3 * nv + 3];
    let mut triangles = vec![0u32; 3 * nt + 3];
    let mut n = if normals { vec![0.0 as Real; 3 * nv + 3] } else { Vec::new() };
    let mut v = if velocities { vec![0.0 as Real; 3 * nv + 3] } else { Vec::new() };
    let out = ffi::SalvaHipSurfaceOut {
        vertices: vertices.as_mut_ptr(),
        normals: if normals { n.as_mut_ptr() } else { std::ptr::null_mut() },
        velocities: if velocities { v.as_mut_ptr() } else { std::ptr::null_mut() },
        triangles: triangles.as_mut_ptr(),
        vertex_capacity: nv as u64,
        triangle_capacity: nt as u64,
    };
    check(call(&out, counts.as_mut_ptr()))?;
    let vectors = |a: &[Real]| a.chunks_exact(3).take(nv).map(|c| Vector3::new(c[0], c[1], c[2])).collect::<Vec<_>>();
    Ok(SurfaceMesh {
        vertices: vertices.chunks_exact(3).take(nv).map(|c| Point3::new(c[0], c[1], c[2])).collect(),
        normals: vectors(&n),
        velocities: vectors(&v),
        triangles: triangles.chunks_exact(3).take(nt).map(|c| [c[0], c[1], c[2]]).collect(),
    })
}

#[allow(clippy::too_many_arguments)]
pub(crate) fn extract(
    world: *mut ffi::SalvaHipWorld, fluid_mask: u32, field: SurfaceField, iso: Real, origin: &Point3<Real>, spacing: Real, dims: [u32; 3],
    normals: bool, velocities: bool,
) -> Result<SurfaceMesh, Error> {
    let o = [origin.x, origin.y, origin.z];
    let f = match field {
        SurfaceField::Density => ffi::SALVA_HIP_SURFACE_DENSITY,
        SurfaceField::Fraction => ffi::SALVA_HIP_SURFACE_FRACTION,
    } as u32;
    fill(normals, velocities, |out, counts| unsafe {
        ffi::salva_hip_extract_surface(world, fluid_mask, f, iso, o.as_ptr(), spacing, dims.as_ptr(), 0, out, counts)
    })
}

/// The same with the anisotropic kernels behind the node values and the normals (`salva_hip_extract_surface_anisotropic`).
#[allow(clippy::too_many_arguments)]
pub(crate) fn extract_anisotropic(
    world: *mut ffi::SalvaHipWorld, fluid_mask: u32, params: &crate::field::Anisotropy, field: SurfaceField, iso: Real, origin: &Point3<Real>,
    spacing: Real, dims: [u32; 3], normals: bool, velocities: bool,
) -> Result<SurfaceMesh, Error> {
    let o = [origin.x, origin.y, origin.z];
    let f = match field {
        SurfaceField::Density => ffi::SALVA_HIP_SURFACE_DENSITY,
        SurfaceField::Fraction => ffi::SALVA_HIP_SURFACE_FRACTION,
    } as u32;
    let p = params.raw();
    fill(normals, velocities, |out, counts| unsafe {
        ffi::salva_hip_extract_surface_anisotropic(world, fluid_mask, &p, f, iso, o.as_ptr(), spacing, dims.as_ptr(), 0, out, counts)
    })
}

/// `values`: nx * ny * nz node values, z fastest.
pub(crate) fn extract_from_values(
    world: *mut ffi::SalvaHipWorld, values: &[Real], iso: Real, origin: &Point3<Real>, spacing: Real, dims: [u32; 3],
) -> Result<SurfaceMesh, Error> {
    assert_eq!(values.len() as u64, dims.iter().map(|&d| d as u64).product::<u64>(), "values.len() != nx * ny * nz");
    let o = [origin.x, origin.y, origin.z];
    fill(false, false, |out, counts| unsafe {
        ffi::salva_hip_extract_surface_from_values(world, values.as_ptr(), iso, o.as_ptr(), spacing, dims.as_ptr(), 0, out, counts)
    })
}

/// (lo, hi, how many positions are finite); with none, lo = +inf and hi = -inf.
pub(crate) fn fluid_bounds(world: *mut ffi::SalvaHipWorld, fluid_mask: u32) -> Result<(Point3<Real>, Point3<Real>, u64), Error> {
    let (mut lo, mut hi, mut n) = ([0.0 as Real; 3], [0.0 as Real; 3], 0u64);
    check(unsafe { ffi::salva_hip_get_fluid_bounds(world, fluid_mask, lo.as_mut_ptr(), hi.as_mut_ptr(), &mut n) })?;
    Ok((Point3::new(lo[0], lo[1], lo[2]), Point3::new(hi[0], hi[1], hi[2]), n))
}

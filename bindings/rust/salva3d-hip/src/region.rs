//! Regions (`SalvaHipRegion`, include/salva_hip.h): where `LiquidWorld::delete_particles_in` and the sinks of `LiquidWorld::add_sink`
//! delete particles on the device.  A particle matches when its solid distance to the region is <= `margin`; `inverted()` selects the
//! particles that do not match (a particle with a non-finite position never matches: an inverted region takes it).
use crate::ffi;
use nalgebra::{Point3, UnitQuaternion, Vector3};
use salva3d::math::Real;

#[derive(Clone, Copy, Debug)]
pub struct Region {
    pub(crate) raw: ffi::SalvaHipRegion,
}

impl Region {
    fn base(kind: i32) -> ffi::SalvaHipRegion {
        let mut raw: ffi::SalvaHipRegion = unsafe { std::mem::zeroed() };
        raw.struct_size = ffi::SALVA_HIP_REGION_BYTES as u32;
        raw.version = ffi::SALVA_HIP_REGION_VERSION as u32;
        raw.kind = kind;
        raw.rotation_ijkw = [0.0, 0.0, 0.0, 1.0];
        raw
    }
    fn posed(kind: i32, translation: &Vector3<Real>, rotation: &UnitQuaternion<Real>) -> ffi::SalvaHipRegion {
        let mut raw = Self::base(kind);
        raw.translation = [translation.x, translation.y, translation.z];
        raw.rotation_ijkw = [rotation.i, rotation.j, rotation.k, rotation.w];
        raw
    }
    /// Everything behind the plane through `point` with the outward unit `normal`.
    pub fn half_space(point: &Point3<Real>, normal: &Vector3<Real>) -> Self {
        let mut raw = Self::base(ffi::SALVA_HIP_REGION_HALFSPACE);
        raw.point = [point.x, point.y, point.z];
        raw.normal = [normal.x, normal.y, normal.z];
        Self { raw }
    }
    pub fn aabb(mins: &Point3<Real>, maxs: &Point3<Real>) -> Self {
        let mut raw = Self::base(ffi::SALVA_HIP_REGION_AABB);
        raw.mins = [mins.x, mins.y, mins.z];
        raw.maxs = [maxs.x, maxs.y, maxs.z];
        Self { raw }
    }
    /// A posed ball, cuboid, capsule (y) or cylinder (y).
    pub fn shape(shape: ffi::SalvaHipShape, translation: &Vector3<Real>, rotation: &UnitQuaternion<Real>) -> Self {
        let mut raw = Self::posed(ffi::SALVA_HIP_REGION_SHAPE, translation, rotation);
        raw.shape = shape;
        Self { raw }
    }
    /// A posed oriented mesh of the same world (`salva_hip_create_mesh`'s handle).
    pub fn mesh(mesh: u32, translation: &Vector3<Real>, rotation: &UnitQuaternion<Real>) -> Self {
        let mut raw = Self::posed(ffi::SALVA_HIP_REGION_MESH, translation, rotation);
        raw.handle = mesh;
        Self { raw }
    }
    /// A posed compound of the same world (`salva_hip_create_compound`'s handle).
    pub fn compound(compound: u32, translation: &Vector3<Real>, rotation: &UnitQuaternion<Real>) -> Self {
        let mut raw = Self::posed(ffi::SALVA_HIP_REGION_COMPOUND, translation, rotation);
        raw.handle = compound;
        Self { raw }
    }
    pub fn with_margin(mut self, margin: Real) -> Self {
        self.raw.margin = margin;
        self
    }
    pub fn inverted(mut self) -> Self {
        self.raw.flags |= ffi::SALVA_HIP_REGION_INVERT as u32;
        self
    }
}

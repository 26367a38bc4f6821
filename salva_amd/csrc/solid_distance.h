// solid_distance.h — `shape.distance_to_point(identity, l, solid = true)` on the device, for a point in the shape's own frame: the one
// copy the shape queries (world_query.hip) and the region predicates (sink.hip) share.  f32 throughout; 0 inside a solid.
#pragma once
#include "common.h"
#include "dcs.h"
#include "mesh.h"
#include "compound.h"

namespace salva {

#ifdef __HIPCC__
// a built-in shape: ball max(|l| - radius, 0); capsule: the distance to the segment minus the radius; cylinder: beyond the caps and
// beyond the side; cuboid |max(|l| - half_extents, 0)|
__device__ __forceinline__ float shape_solid_distance(int kind, const float p[3], float lx, float ly, float lz) {
    float d;
    if (kind == SALVA_HIP_SHAPE_BALL) {
        d = fmaxf(sqrtf(lx * lx + ly * ly + lz * lz) - p[0], 0.0f);
    } else if (kind == SALVA_HIP_SHAPE_CAPSULE) {  // distance to the segment (0, -hh..hh, 0), minus the radius
        const float ey = ly - fminf(fmaxf(ly, -p[0]), p[0]);
        d = fmaxf(sqrtf(lx * lx + ey * ey + lz * lz) - p[1], 0.0f);
    } else if (kind == SALVA_HIP_SHAPE_CYLINDER) {  // beyond the caps and beyond the side
        const float ey = fmaxf(fabsf(ly) - p[0], 0.0f), er = fmaxf(sqrtf(lx * lx + lz * lz) - p[1], 0.0f);
        d = sqrtf(ey * ey + er * er);
    } else {
        const float dx = fmaxf(fabsf(lx) - p[0], 0.0f), dy = fmaxf(fabsf(ly) - p[1], 0.0f), dz = fmaxf(fabsf(lz) - p[2], 0.0f);
        d = sqrtf(dx * dx + dy * dy + dz * dz);
    }
    return d;
}
// an oriented mesh: 0 inside, the distance to the closest point outside
__device__ __forceinline__ float mesh_solid_distance(const MeshDev& m, float lx, float ly, float lz) {
    float jx, jy, jz;
    bool inside;
    mesh_project_point(m, lx, ly, lz, jx, jy, jz, inside);
    const float dx = lx - jx, dy = ly - jy, dz = lz - jz;
    return inside ? 0.0f : sqrtf((dx * dx + dy * dy) + dz * dz);
}
// a compound: the smallest of its parts', each taken in the part's frame (pose_k^-1 * l, quat_rot with the conjugate)
__device__ __forceinline__ float compound_solid_distance(const CompoundPartDev* __restrict__ parts, uint32_t nparts, float lx, float ly, float lz) {
    float d = __builtin_inff();
#pragma unroll 1
    for (uint32_t k = 0; k < nparts; ++k) {  // (k is wave-uniform: the table comes through the scalar cache)
        const CompoundPartDev& P = parts[k];
        float kx, ky, kz;
        quat_rot(-P.q[0], -P.q[1], -P.q[2], P.q[3], lx - P.t[0], ly - P.t[1], lz - P.t[2], kx, ky, kz);
        d = fminf(d, P.kind == SALVA_HIP_SHAPE_MESH ? mesh_solid_distance(P.mesh, kx, ky, kz) : shape_solid_distance(P.kind, P.p, kx, ky, kz));
    }
    return d;
}
#endif  // __HIPCC__

}  // namespace salva

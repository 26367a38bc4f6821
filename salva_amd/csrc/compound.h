// compound.h — a device-resident compound collider (compound.hip): a list of at most 64 posed parts, each a ball, a
// cuboid, a capsule, a cylinder or a mesh of the same world, which is what parry's `Compound` is for the bodies rapier users build
// out of several shapes (a hull of cuboids, a ring of slabs, a convex decomposition handed over as oriented meshes).  The device
// functions below are the one walk over the parts that DynamicContactSampling (dcs.hip: k_dcs_compound_project, k_dcsb_project) and the
// shape query (world_query.hip: k_compound_query) share.
//
// The projection is this project's reading of parry 0.18's Compound::project_local_point_and_get_feature (a best-first visit of
// the parts, solid = false): every part projects the point on its own boundary, the part whose projection is nearest wins, ties go
// to the lowest part index, and is_inside is that part's alone — a point deep inside part A but nearer to the surface of a part B it
// lies outside of is reported outside, on B.  Unpinned, like §13 and §14: parry's source is not vendored.
#pragma once
#include <memory>
#include <vector>

#include "common.h"
#include "dcs.h"
#include "mesh.h"
#include "../../include/salva_hip.h"

namespace salva {

// one part as the kernels read it (the table is indexed with a wave-uniform counter: it comes through the scalar cache)
struct CompoundPartDev {
    int kind;             // SALVA_HIP_SHAPE_BALL .. _MESH
    float p[3];           // as SalvaHipShape::params
    float t[3], q[4];     // the part's pose in the compound's frame
    float lo[3], hi[3];   // parry's part.compute_aabb(part_pos), loosened by 2^-18 of the compound's largest coordinate (§14's rule)
    float eps;            // f32::default_epsilon()
    MeshDev mesh;         // kind == SALVA_HIP_SHAPE_MESH
};

struct CompoundRes {
    uint32_t nparts = 0;
    bool solid = true;    // every mesh part is oriented: the compound has a solid distance (the shape query needs one)
    float mins[3] = {0, 0, 0}, maxs[3] = {0, 0, 0};  // the merge of the parts' boxes before they are loosened
    std::vector<std::shared_ptr<MeshRes>> meshes;    // the meshes of the mesh parts, kept alive: salva_hip_destroy_mesh refuses
    DevBuf<CompoundPartDev> parts;
};

// the parts' table and the compound's local box from the caller's parts, validated (SALVA_HIP_E_INVALID); `part_meshes[k]`: the mesh
// of part k, nullptr for the other kinds
void compound_build_table(const SalvaHipCompoundPart* parts, uint32_t nparts, const std::vector<const MeshRes*>& part_meshes,
                          std::vector<CompoundPartDev>& table, float mins[3], float maxs[3]);
// parry's Aabb::transform_by: the local box's centre posed, -+ |R| half_extents (dcs.hip)
void aabb_transform_by(const float mins[3], const float maxs[3], const float t[3], const float q[4], float lo[3], float hi[3]);
DcsParams dcs_params_compound(const CompoundRes& c, const SalvaHipRigidPose& pose, float h, float particle_radius, float dt);
// the compound arm between launch_dcs_gather and launch_dcs_apply: what launch_dcs_project_mesh is for a mesh
void launch_dcs_compound_project(uint32_t cnt, const float4* pred, const CompoundPartDev* parts, uint32_t nparts, const DcsParams& s,
                                 float4* proj, hipStream_t st);

#ifdef __HIPCC__
// the squared distance from l to a part's loosened box
__host__ __device__ __forceinline__ float compound_box_d2(const CompoundPartDev& P, float lx, float ly, float lz) {
#pragma clang fp contract(off)
    const float dx = fmaxf(fmaxf(P.lo[0] - lx, 0.0f), lx - P.hi[0]), dy = fmaxf(fmaxf(P.lo[1] - ly, 0.0f), ly - P.hi[1]),
                dz = fmaxf(fmaxf(P.lo[2] - lz, 0.0f), lz - P.hi[2]);
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// The projection of l (in the compound's frame) on the compound and is_inside.  PRUNE: a part is left out when the squared distance
// from l to its loosened box, times 0.999999, is strictly greater than the best so far — its projection lies in that box, so it cannot
// win, and the result is the walk over all parts bit for bit (tests/compound_walk_check.hip runs both on the host).
template <bool PRUNE>
__host__ __device__ __forceinline__ void compound_project_local(const CompoundPartDev* __restrict__ parts, uint32_t nparts, float lx, float ly,
                                                                float lz, float& ox, float& oy, float& oz, bool& inside) {
#pragma clang fp contract(off)
    float best = __builtin_inff();
    ox = lx; oy = ly; oz = lz;
    inside = false;
#pragma unroll 1
    for (uint32_t k = 0; k < nparts; ++k) {
        const CompoundPartDev& P = parts[k];
        if (PRUNE && compound_box_d2(P, lx, ly, lz) * 0.999999f > best) continue;
        float kx, ky, kz, jx, jy, jz, cx, cy, cz;
        bool in_k;
        quat_rot(-P.q[0], -P.q[1], -P.q[2], P.q[3], lx - P.t[0], ly - P.t[1], lz - P.t[2], kx, ky, kz);
        if (P.kind == SALVA_HIP_SHAPE_MESH) mesh_project_point(P.mesh, kx, ky, kz, jx, jy, jz, in_k);
        else dcs_project_local(P, kx, ky, kz, jx, jy, jz, in_k);
        quat_rot(P.q[0], P.q[1], P.q[2], P.q[3], jx, jy, jz, cx, cy, cz);
        cx += P.t[0]; cy += P.t[1]; cz += P.t[2];
        const float dx = lx - cx, dy = ly - cy, dz = lz - cz;
        const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
        if (d2 < best) { best = d2; ox = cx; oy = cy; oz = cz; inside = in_k; }  // (strict: a tie stays with the lower index)
    }
}

// project_point_and_get_feature(m, pt) of a posed compound: m^-1 * pt, the walk, carried back by m (dcs_project_world's frame change)
__host__ __device__ __forceinline__ void dcs_project_compound_world(const CompoundPartDev* __restrict__ parts, uint32_t nparts, const DcsParams& s,
                                                                    float px, float py, float pz, float& wx, float& wy, float& wz, bool& inside) {
    float lx, ly, lz;
    quat_rot(-s.q[0], -s.q[1], -s.q[2], s.q[3], px - s.t[0], py - s.t[1], pz - s.t[2], lx, ly, lz);
    float jx, jy, jz;
    compound_project_local<true>(parts, nparts, lx, ly, lz, jx, jy, jz, inside);
    quat_rot(s.q[0], s.q[1], s.q[2], s.q[3], jx, jy, jz, wx, wy, wz);
    wx += s.t[0]; wy += s.t[1]; wz += s.t[2];
}
#endif  // __HIPCC__

}  // namespace salva

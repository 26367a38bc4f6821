// dcs.h — DynamicContactSampling (dcs.hip): launcher interface used by world_coupling.hip (the shape helpers also by world_query.hip, sample.hip and compound.hip).
#pragma once
#include <cmath>

#include "common.h"
#include "device_types.h"
#include "mesh.h"
#include "../../include/salva_hip.h"

namespace salva {

struct DcsParams {
    int kind;
    float p[3];           // radius | half extents | (half height, radius) for capsule and cylinder
    float t[3], q[4];     // collider.position(): translation, unit quaternion (i, j, k, w)
    float lo[3], hi[3];   // shape AABB loosened by h + prediction (fluids_pipeline.rs:196-199)
    int clo[3], chi[3];   // HGrid::key(mins) .. key(maxs) (hgrid.rs:128-129)
    float dt;             // timestep.dt(): the previous substep's length (0 before the first step)
    float margin;         // particle_radius * 0.1 (:194)
    float reach;          // h + prediction (:234)
    float eps;            // f32::default_epsilon() (:223)
    float h;              // cell width (on a folded grid the cell a key names is one of several images: the position says which)
};

#ifdef __HIPCC__
// The geometry below is `__host__ __device__` for the sake of tests/compound_walk_check.hip, which runs it on the host; the division
// is the correctly rounded one on both sides.
__host__ __device__ __forceinline__ float dcs_div(float a, float b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// nalgebra UnitQuaternion * Vector3: t = 2 q.vec x v; v' = t w + q.vec x t + v
__host__ __device__ __forceinline__ void quat_rot(float qx, float qy, float qz, float qw, float vx, float vy, float vz, float& ox, float& oy,
                                         float& oz) {
    const float tx = (qy * vz - qz * vy) * 2.0f, ty = (qz * vx - qx * vz) * 2.0f, tz = (qx * vy - qy * vx) * 2.0f;
    const float cx = qy * tz - qz * ty, cy = qz * tx - qx * tz, cz = qx * ty - qy * tx;
    ox = (tx * qw + cx) + vx;
    oy = (ty * qw + cy) + vy;
    oz = (tz * qw + cz) + vz;
}


// project_local of the built-in shapes (see the header of this file) on a collider-local point: the projection and is_inside.
// The one copy of this arithmetic: k_dcs_project, k_dcsb_project and the walk over a compound's parts (compound.h) call it.  `S`: DcsParams
// or a compound's part — anything with `kind`, `p` and `eps`.
template <typename S>
__host__ __device__ __forceinline__ void dcs_project_local(const S& s, float lx, float ly, float lz, float& jx, float& jy, float& jz,
                                                  bool& inside) {
    if (s.kind == SALVA_HIP_SHAPE_BALL) {
        const float r = s.p[0], d2 = (lx * lx + ly * ly) + lz * lz;
        inside = d2 <= r * r;
        const float f = dcs_div(r, sqrtf(d2));
        jx = lx * f; jy = ly * f; jz = lz * f;
    } else if (s.kind == SALVA_HIP_SHAPE_CAPSULE) {
        const float hh = s.p[0], r = s.p[1];
        // a = (0, -hh, 0), ab = (0, hh - (-hh), 0), ap = p - a; dots as ((x0 y0 + x1 y1) + x2 y2)
        const float aby = hh - (-hh);
        const float apx = lx, apy = ly - (-hh), apz = lz;
        const float ab_ap = (0.0f * apx + aby * apy) + 0.0f * apz;
        const float sqnab = (0.0f * 0.0f + aby * aby) + 0.0f * 0.0f;
        float sx = 0.0f, sy, sz = 0.0f;
        if (ab_ap <= 0.0f) sy = -hh;
        else if (ab_ap >= sqnab) sy = hh;
        else { const float u = dcs_div(ab_ap, sqnab); sx = 0.0f + 0.0f * u; sy = -hh + aby * u; sz = 0.0f + 0.0f * u; }
        const float ex = lx - sx, ey = ly - sy, ez = lz - sz;
        const float sq = (ex * ex + ey * ey) + ez * ez;
        if (sq > s.eps * s.eps) {
            const float dist = sqrtf(sq);
            inside = dist <= r;
            jx = sx + dcs_div(ex, dist) * r; jy = sy + dcs_div(ey, dist) * r; jz = sz + dcs_div(ez, dist) * r;
        } else {
            inside = true;
            jx = sx + 1.0f * r; jy = sy + 0.0f * r; jz = sz + 0.0f * r;
        }
    } else if (s.kind == SALVA_HIP_SHAPE_CYLINDER) {
        const float hh = s.p[0], r = s.p[1];
        const float planar = sqrtf(lx * lx + lz * lz);
        float dx2 = dcs_div(lx, planar), dz2 = dcs_div(lz, planar);
        if (planar <= s.eps) { dx2 = 1.0f; dz2 = 0.0f; }
        const float qx = dx2 * r, qz = dz2 * r;
        if (ly >= -hh && ly <= hh && planar <= r) {
            inside = true;
            const float top = hh - ly, bottom = ly - (-hh), side = r - planar;
            if (top < bottom && top < side) { jx = lx; jy = hh; jz = lz; }
            else if (bottom < top && bottom < side) { jx = lx; jy = -hh; jz = lz; }
            else { jx = qx; jy = ly; jz = qz; }
        } else {
            inside = false;
            if (ly > hh) { jy = hh; if (planar <= r) { jx = lx; jz = lz; } else { jx = qx; jz = qz; } }
            else if (ly < -hh) { jy = -hh; if (planar <= r) { jx = lx; jz = lz; } else { jx = qx; jz = qz; } }
            else { jx = qx; jy = ly; jz = qz; }
        }
    } else {
        const float l3[3] = {lx, ly, lz};
        float mins_pt[3], pt_maxs[3], shift[3];
        inside = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mins_pt[a] = -s.p[a] - l3[a];
            pt_maxs[a] = l3[a] - s.p[a];
            shift[a] = fmaxf(mins_pt[a], 0.0f) - fmaxf(pt_maxs[a], 0.0f);
            if (shift[a] != 0.0f) inside = false;
        }
        if (inside) {
            float best = -3.402823466e+38f;
            bool is_mins = false;
            int best_id = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (mins_pt[a] < pt_maxs[a]) {
                    if (pt_maxs[a] > best) { best_id = a; is_mins = false; best = pt_maxs[a]; }
                } else if (mins_pt[a] > best) { best_id = a; is_mins = true; best = mins_pt[a]; }
            }
            const float sh = is_mins ? best : -best;
            shift[0] = best_id == 0 ? sh : 0.0f; shift[1] = best_id == 1 ? sh : 0.0f; shift[2] = best_id == 2 ? sh : 0.0f;
        }
        jx = l3[0] + shift[0]; jy = l3[1] + shift[1]; jz = l3[2] + shift[2];
    }
}
#endif  // __HIPCC__

// number of parameters of a built-in collider shape (include/salva_hip.h); throws SALVA_HIP_E_INVALID for any other kind
int shape_param_count(int kind);
// ... and its parameters are positive and finite: throws SALVA_HIP_E_INVALID with `message` (world_coupling.hip)
void check_shape_params(const SalvaHipShape& shape, const char* message);
// HGrid::key(lo) .. key(hi) per axis (hgrid.rs:128-129): floor(x / h), clamped like the particles' cell coordinates (tile.h cell_coord)
void cell_range(const float lo[3], const float hi[3], float h, int clo[3], int chi[3]);
void shape_world_extent(const SalvaHipShape& shape, const float rotation_ijkw[4], float ext[3]);
DcsParams dcs_params(const SalvaHipShape& shape, const SalvaHipRigidPose& pose, float h, float particle_radius, float dt);
// one candidate (projection xyz, host particle index bits) and one flag per fluid particle; pushes particles inside the
// shape out of it in place (positions and velocities of the sorted working set).  gtag != nullptr (decomposed run): ghosts are
// pushed but emit nothing, and the rows carry the sorted index instead of perm[] (launch_dcs_pack)
void launch_dcs_project(uint32_t n, float4* posm, float4* vel, const uint32_t* keys, const uint32_t* perm, const uint32_t* gtag, TileGrid g,
                        const DcsParams& s, float4* cand, uint8_t* flag, hipStream_t st);
// host-shape arm (salva_hip_set_boundary_dynamic_sampling_host): box tests -> (predicted position, sorted index) per passing
// particle; then, from the host's (projection, is_inside != 0) per compacted candidate, the push-out and the emitted point
DcsParams dcs_params_host(const float mins[3], const float maxs[3], float h, float particle_radius, float dt);
void launch_dcs_gather(uint32_t n, const float4* posm, const float4* vel, const uint32_t* keys, TileGrid g, const DcsParams& s, float4* cand,
                       uint8_t* flag, hipStream_t st);
void launch_dcs_apply(uint32_t cnt, const float4* pred, const float4* proj, float4* posm, float4* vel, const uint32_t* perm,
                      const uint32_t* gtag, const DcsParams& s, float4* cand, uint8_t* flag, hipStream_t st);
// mesh arm (salva_hip_set_boundary_dynamic_sampling_mesh): the same two kernels around a projection on the device — per compacted
// candidate (predicted position) the closest point of the posed mesh and is_inside, in the layout launch_dcs_apply reads
DcsParams dcs_params_mesh(const float mins[3], const float maxs[3], const SalvaHipRigidPose& pose, float h, float particle_radius, float dt);
void launch_dcs_project_mesh(uint32_t cnt, const float4* pred, const MeshDev& mesh, const DcsParams& s, float4* proj, hipStream_t st);
// decomposed run: compacted rows (point, sorted index) -> (point, global id of the source particle), fluid of the source
void launch_dcs_pack(uint32_t cnt, const float4* rows, const uint32_t* gid, const uint32_t* model, float4* out_rows, uint32_t* out_models,
                     hipStream_t st);
// compacted candidates -> boundary rows (position, volume 0), (velocity at the point, boundary slot), source particle
void launch_dcs_emit(uint32_t cnt, const float4* cand, const SalvaHipRigidPose& pose, uint32_t slot, float4* pos, float4* vel,
                     uint32_t* src, hipStream_t st);

// ---- batched runs (dcs.hip "batched runs").  One entry per collider of a run, in slot order; the pass reads `s` and
// `mesh`, the emit `pose`, `slot` and what the host fills in once it has the counts: the collider's first boundary row, its first
// sorted record, and where its rows' source particles go (DynSampling::src, world.h).
struct CompoundPartDev;  // compound.h
struct DcsbEntry {
    DcsParams s;
    MeshDev mesh;  // s.kind == SALVA_HIP_SHAPE_MESH
    const CompoundPartDev* parts;  // s.kind == SALVA_HIP_SHAPE_COMPOUND: the parts' table (compound.h) ...
    uint32_t nparts;               // ... and its length
    SalvaHipRigidPose pose;
    uint32_t slot, row0, rec0;
    uint32_t* src;
};
// counts: ncol + 2 words, zeroed by the caller (records per collider, all records, pushed particles); cap: records / pushes that fit
void launch_dcsb_project(uint32_t n, const float4* posm, const float4* vel, const uint32_t* keys, const uint32_t* perm, TileGrid g,
                         const DcsbEntry* tab, uint32_t ncol, uint32_t cap, uint32_t shift, unsigned long long* counts,
                         unsigned long long* rec_key, uint32_t* rec_idx, float4* rec, uint32_t* push_idx, float4* push_pos, float4* push_vel,
                         hipStream_t st);
// a run with compounds in it: the colliders [c0, c1) — all compounds (`compound`) or none — in a launch of their own; st_*: one entry per
// fluid particle, the particle's state between the launches of a run
void launch_dcsb_segment(bool compound, uint32_t n, const float4* posm, const float4* vel, const uint32_t* keys, const uint32_t* perm, TileGrid g,
                         const DcsbEntry* tab, uint32_t ncol, uint32_t c0, uint32_t c1, uint32_t cap, uint32_t shift, unsigned long long* counts,
                         unsigned long long* rec_key, uint32_t* rec_idx, float4* rec, uint32_t* push_idx, float4* push_pos, float4* push_vel,
                         float4* st_pos, float4* st_vel, uint8_t* st_moved, hipStream_t st);
void launch_dcsb_push(uint32_t cnt, const uint32_t* push_idx, const float4* push_pos, const float4* push_vel, float4* posm, float4* vel,
                      hipStream_t st);
void launch_dcsb_emit(uint32_t cnt, const unsigned long long* skey, const uint32_t* sidx, const float4* rec, const DcsbEntry* tab,
                      uint32_t shift, float4* pos, float4* vel, float4* force, hipStream_t st);

}  // namespace salva

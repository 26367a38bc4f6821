// dcs.hip — ColliderSampling::DynamicContactSampling on the device for ball, cuboid, capsule and cylinder colliders
// (integrations/rapier/fluids_pipeline.rs:193-259).
//
// The reference walks the cells of the fluid grid that the collider's loosened AABB touches, projects every fluid particle
// whose PREDICTED position (x + v dt) lies in that box onto the shape, pushes particles that are inside out of it, and
// emits one boundary particle per projection.  All of that is a per-particle predicate, so here it is one pass over the
// fluid particles (k_dcs_project) followed by a stable compaction of the emitted points (DeviceSelect) and one pass that
// writes them into the boundary's rows (k_dcs_emit).  The grid is not rebuilt after the push-out in the reference — a
// pushed particle stays registered in the cell of its old position for this substep — so the pass runs between the cell-key
// kernel and the sort, and reads each particle's cell back from its key.
//
// parry3d 0.18 (an un-vendored dependency of the reference) supplies the geometry; restated from its published source and
// followed operation by operation:
//   Ball::compute_aabb(pos)   = [t - r, t + r]; Cuboid::compute_aabb(pos) = t -+ |R| half_extents with
//                               R = UnitQuaternion::to_rotation_matrix; Aabb::loosened(m) = [mins - m, maxs + m];
//                               Aabb::contains_local_point: mins <= p <= maxs on every axis
//   project_point_and_get_feature(m, pt) = project_local(m^-1 pt) carried back by m, solid = false:
//     Ball:   inside = |p|^2 <= r^2; proj = p * (r / |p|)
//     Cuboid: shift = sup(mins - p, 0) - sup(p - maxs, 0); outside iff shift != 0 -> p + shift; inside -> the nearest face
//             (the largest of mins - p, p - maxs over the axes)
//     Capsule (new_y: segment a = (0, -hh, 0), b = (0, hh, 0)): s = the segment's closest point (ab.ap <= 0 -> a; >= |ab|^2 -> b;
//             else a + ab (ab.ap / |ab|^2)); (dir, dist) = try_new_and_get(p - s, eps): inside = dist <= r, proj = s + dir r;
//             a point ON the segment: s + (1, 0, 0) r (orthonormal_basis of the axis), inside
//     Cylinder (axis y): planar = |(x, z)|, dir2 = (x, z) / planar ((1, 0) if planar <= eps); inside (|y| <= hh and planar <= r):
//             the nearest of top / bottom / side (strict <, side wins ties); outside: clamp y to the caps and the plane
//             point to the circle
//   Capsule::aabb(pos) = [inf(A, B) - r, sup(A, B) + r] with A, B the posed segment ends; Cylinder::aabb(pos) = t -+ |R| (r, hh, r)
// This file is compiled with -ffp-contract=off (see Makefile): Rust never fuses a*b+c, and the emitted points feed the
// exact d^2 <= h^2 contact test.
#include "dcs.h"
#include "compound.h"
#include "mesh.h"
#include "dist.h"
#include "tile.h"
#include <cmath>

namespace salva {

// the cell the particle was inserted under (hgrid.rs:122-133 filters CELLS by the box, then :211 tests the prediction)
// On a FOLDED grid (device_types.h TileGrid; round 6: worlds with dynamically sampled colliders fold too) the key names the cell modulo
// the axis' period: the image is the one nearest to where the particle is now — an earlier collider of this pass may have pushed it, by
// a fraction of a cell; the periods are at least 64 cells.
__device__ __forceinline__ int dcs_unfold(int rel, uint32_t mask, float x, float h, int origin) {
    if (mask == 0xffffffffu) return origin + rel;
    bool bad = false;
    const int period = (int)(mask + 1u), d = (cell_coord(x, h, bad) - origin) - rel;
    return origin + rel + floor_div(d + period / 2, period) * period;
}
__device__ __forceinline__ bool dcs_in_cells(uint32_t k, const TileGrid& g, const DcsParams& s, const float4& p) {
    const uint32_t tile = k / TCELLS, loc = k % TCELLS;
    const int tz = (int)(tile % (uint32_t)g.ntz), ty = (int)((tile / (uint32_t)g.ntz) % (uint32_t)g.nty),
              tx = (int)(tile / ((uint32_t)g.ntz * (uint32_t)g.nty));
    const int cx = dcs_unfold(tx * TX + (int)(loc / (TY * TZ)), g.mx, p.x, s.h, g.ox), cy = dcs_unfold(ty * TY + (int)((loc / TZ) % TY), g.my, p.y, s.h, g.oy),
              cz = dcs_unfold(tz * TZ + (int)(loc % TZ), g.mz, p.z, s.h, g.oz);
    return !(cx < s.clo[0] || cx > s.chi[0] || cy < s.clo[1] || cy > s.chi[1] || cz < s.clo[2] || cz > s.chi[2]);
}

// :219-243 from the projection on: dpt = particle_pos - proj.point; a particle inside the shape is pushed out along dpt by
// depth + margin and loses its velocity along it; one outside and farther than h + prediction emits nothing (false).
__device__ __forceinline__ bool dcs_finish_reg(float4& p, float4& v, float px, float py, float pz, float wx, float wy, float wz, bool inside,
                                               const DcsParams& s, bool& moved, bool& slowed) {
    const float dx = px - wx, dy = py - wy, dz = pz - wz;
    const float sq = (dx * dx + dy * dy) + dz * dz;
    if (sq > s.eps * s.eps) {  // Unit::try_new_and_get(dpt, f32::EPSILON)
        const float depth = sqrtf(sq);
        const float nx = __fdiv_rn(dx, depth), ny = __fdiv_rn(dy, depth), nz = __fdiv_rn(dz, depth);
        if (inside) {
            const float m = depth + s.margin;
            p.x -= nx * m; p.y -= ny * m; p.z -= nz * m;
            moved = true;
            const float vel_err = (nx * v.x + ny * v.y) + nz * v.z;
            if (vel_err > 0.0f) {
                v.x -= nx * vel_err; v.y -= ny * vel_err; v.z -= nz * vel_err;
                slowed = true;
            }
        } else if (depth > s.reach) {
            return false;
        }
    }
    return true;
}
// ... on the particle in memory (the per-collider kernels); the batched kernel keeps it in registers (k_dcsb_project)
__device__ __forceinline__ bool dcs_finish(uint32_t i, float4 p, float4 v, float px, float py, float pz, float wx, float wy, float wz,
                                           bool inside, const DcsParams& s, float4* __restrict__ posm, float4* __restrict__ vel) {
    bool moved = false, slowed = false;
    const bool keep = dcs_finish_reg(p, v, px, py, pz, wx, wy, wz, inside, s, moved, slowed);
    if (moved) posm[i] = p;
    if (slowed) vel[i] = v;
    return keep;
}

// project_point_and_get_feature(m, pt) of a built-in shape: m^-1 * pt, project_local, carried back by m
__device__ __forceinline__ void dcs_project_world(const DcsParams& s, float px, float py, float pz, float& wx, float& wy, float& wz,
                                                  bool& inside) {
    float lx, ly, lz;
    quat_rot(-s.q[0], -s.q[1], -s.q[2], s.q[3], px - s.t[0], py - s.t[1], pz - s.t[2], lx, ly, lz);
    float jx, jy, jz;
    dcs_project_local(s, lx, ly, lz, jx, jy, jz, inside);
    quat_rot(s.q[0], s.q[1], s.q[2], s.q[3], jx, jy, jz, wx, wy, wz);
    wx += s.t[0]; wy += s.t[1]; wz += s.t[2];
}
// ... of a posed mesh: the closest point over all triangles (mesh.h) in place of project_local
__device__ __forceinline__ void dcs_project_mesh_world(const MeshDev& mesh, const DcsParams& s, float px, float py, float pz, float& wx,
                                                       float& wy, float& wz, bool& inside) {
    float lx, ly, lz;
    quat_rot(-s.q[0], -s.q[1], -s.q[2], s.q[3], px - s.t[0], py - s.t[1], pz - s.t[2], lx, ly, lz);
    float jx, jy, jz;
    mesh_project_point(mesh, lx, ly, lz, jx, jy, jz, inside);
    quat_rot(s.q[0], s.q[1], s.q[2], s.q[3], jx, jy, jz, wx, wy, wz);
    wx += s.t[0]; wy += s.t[1]; wz += s.t[2];
}

__global__ __launch_bounds__(BLOCK) void k_dcs_project(uint32_t n, float4* __restrict__ posm, float4* __restrict__ vel,
                                                       const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm,
                                                       const uint32_t* __restrict__ gtag, TileGrid g, DcsParams s,
                                                       float4* __restrict__ cand, uint8_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    flag[i] = 0;
    float4 p = posm[i];
    if (!dcs_in_cells(keys[i], g, s, p)) return;
    float4 v = vel[i];
    const float px = p.x + v.x * s.dt, py = p.y + v.y * s.dt, pz = p.z + v.z * s.dt;  // :206-207
    if (px < s.lo[0] || px > s.hi[0] || py < s.lo[1] || py > s.hi[1] || pz < s.lo[2] || pz > s.hi[2]) return;  // NaN: passes, as `<` / `>` do
    float wx, wy, wz;
    bool inside;
    dcs_project_world(s, px, py, pz, wx, wy, wz, inside);
    if (dcs_finish(i, p, v, px, py, pz, wx, wy, wz, inside, s, posm, vel)) {
        // decomposed run (gtag != nullptr): a ghost is pushed like its owner — same inputs, same arithmetic — but only the owner
        // emits; the row then carries the SORTED index (k_dcs_pack turns it into global id + fluid)
        if (gtag && (gtag[i] & GTAG_GHOST)) return;
        cand[i] = make_float4(wx, wy, wz, __uint_as_float(gtag ? i : perm[i]));
        flag[i] = 1;
    }
}

// The host-shape arm (salva_hip_set_boundary_dynamic_sampling_host): the same pass cut in two around the host's
// `project_point_and_get_feature`.  k_dcs_gather: the particles whose cell and predicted position pass the box tests
// (:204-211), as (predicted position, sorted index); k_dcs_apply: the rest of the loop body for those, from the host's
// (projection, is_inside).
__global__ __launch_bounds__(BLOCK) void k_dcs_gather(uint32_t n, const float4* __restrict__ posm, const float4* __restrict__ vel,
                                                      const uint32_t* __restrict__ keys, TileGrid g, DcsParams s,
                                                      float4* __restrict__ cand, uint8_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    flag[i] = 0;
    const float4 p = posm[i];
    if (!dcs_in_cells(keys[i], g, s, p)) return;
    const float4 v = vel[i];
    const float px = p.x + v.x * s.dt, py = p.y + v.y * s.dt, pz = p.z + v.z * s.dt;
    if (px < s.lo[0] || px > s.hi[0] || py < s.lo[1] || py > s.hi[1] || pz < s.lo[2] || pz > s.hi[2]) return;
    cand[i] = make_float4(px, py, pz, __uint_as_float(i));
    flag[i] = 1;
}
__global__ __launch_bounds__(BLOCK) void k_dcs_apply(uint32_t cnt, const float4* __restrict__ pred, const float4* __restrict__ proj,
                                                     float4* __restrict__ posm, float4* __restrict__ vel, const uint32_t* __restrict__ perm,
                                                     const uint32_t* __restrict__ gtag, DcsParams s, float4* __restrict__ cand,
                                                     uint8_t* __restrict__ flag) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= cnt) return;
    const float4 pr = pred[k], w = proj[k];
    const uint32_t i = __float_as_uint(pr.w);
    const float4 p = posm[i], v = vel[i];
    bool keep = dcs_finish(i, p, v, pr.x, pr.y, pr.z, w.x, w.y, w.z, w.w != 0.0f, s, posm, vel);
    if (gtag && (gtag[i] & GTAG_GHOST)) keep = false;  // (decomposed run: pushed here too, emitted by its owner; see k_dcs_project)
    flag[k] = keep ? 1 : 0;
    if (keep) cand[k] = make_float4(w.x, w.y, w.z, __uint_as_float(gtag ? i : perm[i]));
}

// The mesh arm (salva_hip_set_boundary_dynamic_sampling_mesh): the host arm's pass with the host taken out of it.  Between
// k_dcs_gather and k_dcs_apply one thread per compacted candidate projects its predicted position onto the posed mesh —
// m^-1 pt as in k_dcs_project, the closest point over all triangles (mesh.h), carried back by the pose — and writes what the host's
// callback would have written: (projection, is_inside ? 1 : 0).
__global__ __launch_bounds__(BLOCK) void k_dcs_project_mesh(uint32_t cnt, const float4* __restrict__ pred, MeshDev mesh, DcsParams s,
                                                            float4* __restrict__ proj) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= cnt) return;
    const float4 pr = pred[k];
    float wx, wy, wz;
    bool inside;
    dcs_project_mesh_world(mesh, s, pr.x, pr.y, pr.z, wx, wy, wz, inside);
    proj[k] = make_float4(wx, wy, wz, inside ? 1.0f : 0.0f);
}

// The compound arm (salva_hip_set_boundary_dynamic_sampling_compound; compound.h): the mesh arm's pass with the walk over
// the compound's parts in place of the walk over one mesh.  The part index is wave-uniform, so the table is read through the scalar
// cache.
__global__ __launch_bounds__(BLOCK) void k_dcs_compound_project(uint32_t cnt, const float4* __restrict__ pred,
                                                                const CompoundPartDev* __restrict__ parts, uint32_t nparts, DcsParams s,
                                                                float4* __restrict__ proj) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= cnt) return;
    const float4 pr = pred[k];
    float wx, wy, wz;
    bool inside;
    dcs_project_compound_world(parts, nparts, s, pr.x, pr.y, pr.z, wx, wy, wz, inside);
    proj[k] = make_float4(wx, wy, wz, inside ? 1.0f : 0.0f);
}

// Decomposed run: this rank's compacted rows (point, sorted index of the source particle) -> its section of the table every
// rank assembles (World::dist_gather_emitted): (point, global id of the source) and the source's fluid.
__global__ __launch_bounds__(BLOCK) void k_dcs_pack(uint32_t cnt, const float4* __restrict__ rows, const uint32_t* __restrict__ gid,
                                                    const uint32_t* __restrict__ model, float4* __restrict__ out_rows,
                                                    uint32_t* __restrict__ out_models) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= cnt) return;
    const float4 r = rows[k];
    const uint32_t i = __float_as_uint(r.w);
    out_rows[k] = make_float4(r.x, r.y, r.z, __uint_as_float(gid[i]));
    out_models[k] = model[i];
}

// one boundary row from one accepted projection (the one copy: k_dcs_emit and k_dcsb_emit)
__device__ __forceinline__ void dcs_emit_row(const float4 c, const SalvaHipRigidPose& pose, uint32_t slot, float4& pos, float4& vel, uint32_t& src) {
    pos = make_float4(c.x, c.y, c.z, 0.0f);  // boundary.volumes.push(0) :249
    float vx = 0.0f, vy = 0.0f, vz = 0.0f;
    if (pose.has_body) {  // body.velocity_at_point(&proj.point) :241-242 (the WORLD point here, unlike the static arm)
        const float rx = c.x - pose.world_com[0], ry = c.y - pose.world_com[1], rz = c.z - pose.world_com[2];
        vx = pose.linvel[0] + (pose.angvel[1] * rz - pose.angvel[2] * ry);
        vy = pose.linvel[1] + (pose.angvel[2] * rx - pose.angvel[0] * rz);
        vz = pose.linvel[2] + (pose.angvel[0] * ry - pose.angvel[1] * rx);
    }
    vel = make_float4(vx, vy, vz, __uint_as_float(slot));
    src = __float_as_uint(c.w);
}
__global__ __launch_bounds__(BLOCK) void k_dcs_emit(uint32_t cnt, const float4* __restrict__ cand, SalvaHipRigidPose pose, uint32_t slot,
                                                    float4* __restrict__ pos, float4* __restrict__ vel, uint32_t* __restrict__ src) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= cnt) return;
    dcs_emit_row(cand[i], pose, slot, pos[i], vel[i], src[i]);
}

// ------------------------------------------------------------------------------------------------ batched runs
// A run of consecutive device-shape colliders in ONE pass over the fluid.  What collider c does to particle i depends on particle
// i's own state and on collider c alone, so a thread that keeps its particle in registers and goes through the colliders in slot
// order computes what C passes of k_dcs_project / k_dcs_gather + k_dcs_project_mesh + k_dcs_apply compute, operation for operation
// (the same device functions).  The pass itself writes no particle: accepted projections are appended to a record buffer, pushed
// particles to a push list, both through one wave-aggregated atomic each; when the record buffer was too small the host grows it and
// repeats the pass from the unmodified state (World::run_dynamic_sampling_batch).  Keys (collider << shift | sorted index) are
// unique, so the radix sort behind the pass gives one order whatever order the atomics ran in: by slot, then by sorted index — the
// order of the per-collider stable selects.
// counts: [0, ncol) records per collider, [ncol] all records, [ncol + 1] pushed particles
__device__ __forceinline__ uint32_t dcsb_append(bool mine, unsigned long long* total, unsigned long long* per_collider) {
    const unsigned long long m = __ballot(mine);
    if (m == 0ull) return 0xffffffffu;
    const int lane = (int)(threadIdx.x & (WAVE - 1)), leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0ull;
    if (lane == leader) {
        base = atomicAdd(total, (unsigned long long)__popcll(m));
        if (per_collider) atomicAdd(per_collider, (unsigned long long)__popcll(m));
    }
    base = __shfl(base, leader, WAVE);
    const unsigned long long k = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
    return (mine && k < 0xffffffffull) ? (uint32_t)k : 0xffffffffu;
}
// What collider c of the table does to the particle a thread holds in registers, and the record it appends.  COMPOUND picks the
// projection at compile time: false — a built-in shape or a mesh, the arithmetic of k_dcs_project / k_dcs_project_mesh; true — the walk
// over a compound's parts (compound.h).  The two never share a kernel: with the walk in it k_dcsb_project would need 106 VGPRs and
// lose its fifth wave, so a run that holds compounds goes through k_dcsb_segment below, one launch per stretch of
// colliders of one class.
template <bool COMPOUND>
__device__ __forceinline__ void dcsb_collider(uint32_t c, uint32_t i, bool live, uint32_t key, float4& p, float4& v, bool& have_v, bool& moved,
                                              bool& slowed, const float4* __restrict__ vel, const uint32_t* __restrict__ perm, const TileGrid& g,
                                              const DcsbEntry* __restrict__ tab, uint32_t ncol, uint32_t cap, uint32_t shift,
                                              unsigned long long* __restrict__ counts, unsigned long long* __restrict__ rec_key,
                                              uint32_t* __restrict__ rec_idx, float4* __restrict__ rec) {
    const DcsParams& s = tab[c].s;
    bool accept = false;
    float wx = 0.0f, wy = 0.0f, wz = 0.0f;
    if (live && dcs_in_cells(key, g, s, p)) {
        if (!have_v) { v = vel[i]; have_v = true; }
        const float px = p.x + v.x * s.dt, py = p.y + v.y * s.dt, pz = p.z + v.z * s.dt;  // :206-207
        if (!(px < s.lo[0] || px > s.hi[0] || py < s.lo[1] || py > s.hi[1] || pz < s.lo[2] || pz > s.hi[2])) {
            bool inside;
            if (COMPOUND) dcs_project_compound_world(tab[c].parts, tab[c].nparts, s, px, py, pz, wx, wy, wz, inside);
            else if (s.kind == SALVA_HIP_SHAPE_MESH) dcs_project_mesh_world(tab[c].mesh, s, px, py, pz, wx, wy, wz, inside);
            else dcs_project_world(s, px, py, pz, wx, wy, wz, inside);
            accept = dcs_finish_reg(p, v, px, py, pz, wx, wy, wz, inside, s, moved, slowed);
        }
    }
    const uint32_t k = dcsb_append(accept, counts + ncol, counts + c);
    if (k < cap) {
        rec_key[k] = ((unsigned long long)c << shift) | (unsigned long long)i;
        rec_idx[k] = k;
        rec[k] = make_float4(wx, wy, wz, __uint_as_float(perm[i]));
    }
}
__global__ __launch_bounds__(BLOCK) void k_dcsb_project(uint32_t n, const float4* __restrict__ posm, const float4* __restrict__ vel,
                                                        const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm, TileGrid g,
                                                        const DcsbEntry* __restrict__ tab, uint32_t ncol, uint32_t cap, uint32_t shift,
                                                        unsigned long long* __restrict__ counts, unsigned long long* __restrict__ rec_key,
                                                        uint32_t* __restrict__ rec_idx, float4* __restrict__ rec,
                                                        uint32_t* __restrict__ push_idx, float4* __restrict__ push_pos,
                                                        float4* __restrict__ push_vel) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < n;  // (every lane stays to the end: the appends are wave-wide)
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v = p;
    uint32_t key = 0u;
    if (live) { p = posm[i]; key = keys[i]; }
    bool have_v = false, moved = false, slowed = false;
#pragma unroll 1
    for (uint32_t c = 0; c < ncol; ++c)  // (c is wave-uniform: the table comes through the scalar cache)
        dcsb_collider<false>(c, i, live, key, p, v, have_v, moved, slowed, vel, perm, g, tab, ncol, cap, shift, counts, rec_key, rec_idx, rec);
    // (a pushed particle has an accepted record: pushes <= records, so the push list fits whenever the records do)
    const uint32_t k = dcsb_append(moved, counts + ncol + 1, nullptr);
    if (k < cap) { push_idx[k] = i; push_pos[k] = p; push_vel[k] = v; }
}
// A run that holds compounds: the colliders [c0, c1) of the table — all compounds (COMPOUND) or none — in a launch of their own.  The
// particle a thread holds travels from one launch to the next through `st_pos` / `st_vel` / `st_moved` (the pass still writes no
// particle of the working set), so the launches of a run, in slot order, compute what k_dcsb_project would: the same device function
// per collider on the same values.  The first launch (c0 == 0) reads the working set, the last (c1 == ncol) appends the pushes.
template <bool COMPOUND>
__global__ __launch_bounds__(BLOCK) void k_dcsb_segment(uint32_t n, const float4* __restrict__ posm, const float4* __restrict__ vel,
                                                        const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm, TileGrid g,
                                                        const DcsbEntry* __restrict__ tab, uint32_t ncol, uint32_t c0, uint32_t c1, uint32_t cap,
                                                        uint32_t shift, unsigned long long* __restrict__ counts,
                                                        unsigned long long* __restrict__ rec_key, uint32_t* __restrict__ rec_idx,
                                                        float4* __restrict__ rec, uint32_t* __restrict__ push_idx, float4* __restrict__ push_pos,
                                                        float4* __restrict__ push_vel, float4* __restrict__ st_pos, float4* __restrict__ st_vel,
                                                        uint8_t* __restrict__ st_moved) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < n;
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v = p;
    uint32_t key = 0u;
    bool have_v = false, moved = false, slowed = false;
    if (live) {
        key = keys[i];
        if (c0 == 0u) p = posm[i];
        else { p = st_pos[i]; v = st_vel[i]; have_v = true; moved = st_moved[i] != 0; }
    }
#pragma unroll 1
    for (uint32_t c = c0; c < c1; ++c)
        dcsb_collider<COMPOUND>(c, i, live, key, p, v, have_v, moved, slowed, vel, perm, g, tab, ncol, cap, shift, counts, rec_key, rec_idx, rec);
    if (c1 == ncol) {
        const uint32_t k = dcsb_append(moved, counts + ncol + 1, nullptr);
        if (k < cap) { push_idx[k] = i; push_pos[k] = p; push_vel[k] = v; }
    } else if (live) {
        if (!have_v) v = vel[i];
        st_pos[i] = p; st_vel[i] = v; st_moved[i] = moved ? 1 : 0;
    }
}
// the pushes of a pass whose records fitted (a velocity that no collider changed is written back as it was read)
__global__ __launch_bounds__(BLOCK) void k_dcsb_push(uint32_t cnt, const uint32_t* __restrict__ push_idx, const float4* __restrict__ push_pos,
                                                     const float4* __restrict__ push_vel, float4* __restrict__ posm, float4* __restrict__ vel) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= cnt) return;
    const uint32_t i = push_idx[k];
    posm[i] = push_pos[k];
    vel[i] = push_vel[k];
}
// sorted records -> the rows of their boundaries (DcsbEntry::row0 / rec0: first boundary row / first sorted record of the collider),
// forces cleared (clear_forces(true) :262)
__global__ __launch_bounds__(BLOCK) void k_dcsb_emit(uint32_t cnt, const unsigned long long* __restrict__ skey, const uint32_t* __restrict__ sidx,
                                                     const float4* __restrict__ rec, const DcsbEntry* __restrict__ tab, uint32_t shift,
                                                     float4* __restrict__ pos, float4* __restrict__ vel, float4* __restrict__ force) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= cnt) return;
    const uint32_t c = (uint32_t)(skey[k] >> shift);
    const DcsbEntry& e = tab[c];
    const uint32_t j = k - e.rec0, row = e.row0 + j;
    dcs_emit_row(rec[sidx[k]], e.pose, e.slot, pos[row], vel[row], e.src[j]);
    force[row] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// half extents of the posed shape's AABB about the pose's translation (parry compute_aabb, see the header of this file)
void shape_world_extent(const SalvaHipShape& shape, const float q[4], float ext[3]) {
    if (shape.kind == SALVA_HIP_SHAPE_BALL) {
        ext[0] = ext[1] = ext[2] = shape.params[0];
    } else if (shape.kind == SALVA_HIP_SHAPE_CAPSULE) {
        // the posed segment ends are t -+ q * (0, hh, 0): extent = |q * b| + radius
        const float qx = q[0], qy = q[1], qz = q[2], qw = q[3];
        const float bx = 0.0f, by = shape.params[0], bz = 0.0f;
        const float tx = (qy * bz - qz * by) * 2.0f, ty = (qz * bx - qx * bz) * 2.0f, tz = (qx * by - qy * bx) * 2.0f;
        const float cx = qy * tz - qz * ty, cy = qz * tx - qx * tz, cz = qx * ty - qy * tx;
        const float u[3] = {(tx * qw + cx) + bx, (ty * qw + cy) + by, (tz * qw + cz) + bz};
        for (int a = 0; a < 3; ++a) ext[a] = std::fabs(u[a]) + shape.params[1];
    } else {
        // UnitQuaternion::to_rotation_matrix (nalgebra geometry/quaternion.rs), then |R| * half_extents
        // (cylinder: the half extents of its local box are (radius, half_height, radius))
        const float i = q[0], j = q[1], k = q[2], w = q[3];
        const float ww = w * w, ii = i * i, jj = j * j, kk = k * k;
        const float ij = i * j * 2.0f, wk = w * k * 2.0f, wj = w * j * 2.0f, ik = i * k * 2.0f, jk = j * k * 2.0f, wi = w * i * 2.0f;
        const float m[3][3] = {{ww + ii - jj - kk, ij - wk, wj + ik}, {wk + ij, ww - ii + jj - kk, jk - wi}, {ik - wj, wi + jk, ww - ii - jj + kk}};
        const bool cyl = shape.kind == SALVA_HIP_SHAPE_CYLINDER;
        const float he[3] = {cyl ? shape.params[1] : shape.params[0], cyl ? shape.params[0] : shape.params[1], cyl ? shape.params[1] : shape.params[2]};
        for (int a = 0; a < 3; ++a)
            ext[a] = (std::fabs(m[a][0]) * he[0] + std::fabs(m[a][1]) * he[1]) + std::fabs(m[a][2]) * he[2];
    }
}

void cell_range(const float lo[3], const float hi[3], float h, int clo[3], int chi[3]) {
    for (int a = 0; a < 3; ++a) {
        clo[a] = (int)std::fmin(std::fmax(std::floor(lo[a] / h), -1073741824.0f), 1073741824.0f);
        chi[a] = (int)std::fmin(std::fmax(std::floor(hi[a] / h), -1073741824.0f), 1073741824.0f);
    }
}

// Ball::compute_aabb / Cuboid::compute_aabb of the posed shape, loosened by h + prediction (:196-199), and the cell range
// HGrid::cells_intersecting_aabb walks (hgrid.rs:128-131).
DcsParams dcs_params(const SalvaHipShape& shape, const SalvaHipRigidPose& pose, float h, float particle_radius, float dt) {
    DcsParams s{};
    s.kind = shape.kind;
    for (int a = 0; a < 3; ++a) { s.p[a] = shape.params[a]; s.t[a] = pose.translation[a]; }
    for (int a = 0; a < 4; ++a) s.q[a] = pose.rotation[a];
    const float prediction = h * 0.5f;
    s.margin = particle_radius * 0.1f;
    s.reach = h + prediction;
    s.h = h;
    s.dt = dt;
    s.eps = 1.1920929e-7f;
    float ext[3];
    shape_world_extent(shape, pose.rotation, ext);
    for (int a = 0; a < 3; ++a) {
        s.lo[a] = (pose.translation[a] - ext[a]) - s.reach;
        s.hi[a] = (pose.translation[a] + ext[a]) + s.reach;
    }
    cell_range(s.lo, s.hi, h, s.clo, s.chi);
    return s;
}

// the host-shape arm: the box is the host's `collider.shape().compute_aabb(&collider_pos)`
DcsParams dcs_params_host(const float mins[3], const float maxs[3], float h, float particle_radius, float dt) {
    DcsParams s{};
    s.kind = SALVA_HIP_SHAPE_HOST;
    s.q[3] = 1.0f;
    const float prediction = h * 0.5f;
    s.margin = particle_radius * 0.1f;
    s.reach = h + prediction;
    s.h = h;
    s.dt = dt;
    s.eps = 1.1920929e-7f;
    for (int a = 0; a < 3; ++a) {
        s.lo[a] = mins[a] - s.reach;
        s.hi[a] = maxs[a] + s.reach;
    }
    cell_range(s.lo, s.hi, h, s.clo, s.chi);
    return s;
}

// the mesh arm: parry's Aabb::transform_by — the local box's centre posed by the collider's pose, -+ |R| half_extents (the matrix
// form of shape_world_extent)
void aabb_transform_by(const float mins[3], const float maxs[3], const float t[3], const float q[4], float lo[3], float hi[3]) {
    SalvaHipShape box{};
    box.kind = SALVA_HIP_SHAPE_CUBOID;
    float c[3], ext[3];
    for (int a = 0; a < 3; ++a) { c[a] = (mins[a] + maxs[a]) * 0.5f; box.params[a] = (maxs[a] - mins[a]) * 0.5f; }
    shape_world_extent(box, q, ext);
    // quat_rot on the host
    const float tx = (q[1] * c[2] - q[2] * c[1]) * 2.0f, ty = (q[2] * c[0] - q[0] * c[2]) * 2.0f, tz = (q[0] * c[1] - q[1] * c[0]) * 2.0f;
    const float cx = q[1] * tz - q[2] * ty, cy = q[2] * tx - q[0] * tz, cz = q[0] * ty - q[1] * tx;
    const float w[3] = {((tx * q[3] + cx) + c[0]) + t[0], ((ty * q[3] + cy) + c[1]) + t[1], ((tz * q[3] + cz) + c[2]) + t[2]};
    for (int a = 0; a < 3; ++a) { lo[a] = w[a] - ext[a]; hi[a] = w[a] + ext[a]; }
}
DcsParams dcs_params_mesh(const float mins[3], const float maxs[3], const SalvaHipRigidPose& pose, float h, float particle_radius, float dt) {
    float lo[3], hi[3];
    aabb_transform_by(mins, maxs, pose.translation, pose.rotation, lo, hi);
    DcsParams s = dcs_params_host(lo, hi, h, particle_radius, dt);
    s.kind = SALVA_HIP_SHAPE_MESH;
    for (int a = 0; a < 3; ++a) s.t[a] = pose.translation[a];
    for (int a = 0; a < 4; ++a) s.q[a] = pose.rotation[a];
    return s;
}

// the compound arm: the box of the mesh arm on the compound's local box
DcsParams dcs_params_compound(const CompoundRes& c, const SalvaHipRigidPose& pose, float h, float particle_radius, float dt) {
    DcsParams s = dcs_params_mesh(c.mins, c.maxs, pose, h, particle_radius, dt);
    s.kind = SALVA_HIP_SHAPE_COMPOUND;
    return s;
}

void launch_dcs_project(uint32_t n, float4* posm, float4* vel, const uint32_t* keys, const uint32_t* perm, const uint32_t* gtag, TileGrid g,
                        const DcsParams& s, float4* cand, uint8_t* flag, hipStream_t st) {
    if (n == 0) return;
    k_dcs_project<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, posm, vel, keys, perm, gtag, g, s, cand, flag);
    SALVA_HIP_CHECK(hipGetLastError());
}
void launch_dcs_gather(uint32_t n, const float4* posm, const float4* vel, const uint32_t* keys, TileGrid g, const DcsParams& s, float4* cand,
                       uint8_t* flag, hipStream_t st) {
    if (n == 0) return;
    k_dcs_gather<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, posm, vel, keys, g, s, cand, flag);
    SALVA_HIP_CHECK(hipGetLastError());
}
void launch_dcs_apply(uint32_t cnt, const float4* pred, const float4* proj, float4* posm, float4* vel, const uint32_t* perm,
                      const uint32_t* gtag, const DcsParams& s, float4* cand, uint8_t* flag, hipStream_t st) {
    if (cnt == 0) return;
    k_dcs_apply<<<div_up(cnt, BLOCK), BLOCK, 0, st>>>(cnt, pred, proj, posm, vel, perm, gtag, s, cand, flag);
    SALVA_HIP_CHECK(hipGetLastError());
}
void launch_dcs_project_mesh(uint32_t cnt, const float4* pred, const MeshDev& mesh, const DcsParams& s, float4* proj, hipStream_t st) {
    if (cnt == 0) return;
    k_dcs_project_mesh<<<div_up(cnt, BLOCK), BLOCK, 0, st>>>(cnt, pred, mesh, s, proj);
    SALVA_HIP_CHECK(hipGetLastError());
}
void launch_dcs_compound_project(uint32_t cnt, const float4* pred, const CompoundPartDev* parts, uint32_t nparts, const DcsParams& s,
                                 float4* proj, hipStream_t st) {
    if (cnt == 0) return;
    k_dcs_compound_project<<<div_up(cnt, BLOCK), BLOCK, 0, st>>>(cnt, pred, parts, nparts, s, proj);
    SALVA_HIP_CHECK(hipGetLastError());
}
void launch_dcs_pack(uint32_t cnt, const float4* rows, const uint32_t* gid, const uint32_t* model, float4* out_rows, uint32_t* out_models,
                     hipStream_t st) {
    if (cnt == 0) return;
    k_dcs_pack<<<div_up(cnt, BLOCK), BLOCK, 0, st>>>(cnt, rows, gid, model, out_rows, out_models);
    SALVA_HIP_CHECK(hipGetLastError());
}
void launch_dcs_emit(uint32_t cnt, const float4* cand, const SalvaHipRigidPose& pose, uint32_t slot, float4* pos, float4* vel,
                     uint32_t* src, hipStream_t st) {
    if (cnt == 0) return;
    k_dcs_emit<<<div_up(cnt, BLOCK), BLOCK, 0, st>>>(cnt, cand, pose, slot, pos, vel, src);
    SALVA_HIP_CHECK(hipGetLastError());
}

void launch_dcsb_project(uint32_t n, const float4* posm, const float4* vel, const uint32_t* keys, const uint32_t* perm, TileGrid g,
                         const DcsbEntry* tab, uint32_t ncol, uint32_t cap, uint32_t shift, unsigned long long* counts,
                         unsigned long long* rec_key, uint32_t* rec_idx, float4* rec, uint32_t* push_idx, float4* push_pos, float4* push_vel,
                         hipStream_t st) {
    if (n == 0) return;
    k_dcsb_project<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, posm, vel, keys, perm, g, tab, ncol, cap, shift, counts, rec_key, rec_idx, rec, push_idx,
                                                       push_pos, push_vel);
    SALVA_HIP_CHECK(hipGetLastError());
}
void launch_dcsb_segment(bool compound, uint32_t n, const float4* posm, const float4* vel, const uint32_t* keys, const uint32_t* perm, TileGrid g,
                         const DcsbEntry* tab, uint32_t ncol, uint32_t c0, uint32_t c1, uint32_t cap, uint32_t shift, unsigned long long* counts,
                         unsigned long long* rec_key, uint32_t* rec_idx, float4* rec, uint32_t* push_idx, float4* push_pos, float4* push_vel,
                         float4* st_pos, float4* st_vel, uint8_t* st_moved, hipStream_t st) {
    if (n == 0) return;
    if (compound)
        k_dcsb_segment<true><<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, posm, vel, keys, perm, g, tab, ncol, c0, c1, cap, shift, counts, rec_key, rec_idx,
                                                                 rec, push_idx, push_pos, push_vel, st_pos, st_vel, st_moved);
    else
        k_dcsb_segment<false><<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, posm, vel, keys, perm, g, tab, ncol, c0, c1, cap, shift, counts, rec_key, rec_idx,
                                                                  rec, push_idx, push_pos, push_vel, st_pos, st_vel, st_moved);
    SALVA_HIP_CHECK(hipGetLastError());
}
void launch_dcsb_push(uint32_t cnt, const uint32_t* push_idx, const float4* push_pos, const float4* push_vel, float4* posm, float4* vel,
                      hipStream_t st) {
    if (cnt == 0) return;
    k_dcsb_push<<<div_up(cnt, BLOCK), BLOCK, 0, st>>>(cnt, push_idx, push_pos, push_vel, posm, vel);
    SALVA_HIP_CHECK(hipGetLastError());
}
void launch_dcsb_emit(uint32_t cnt, const unsigned long long* skey, const uint32_t* sidx, const float4* rec, const DcsbEntry* tab,
                      uint32_t shift, float4* pos, float4* vel, float4* force, hipStream_t st) {
    if (cnt == 0) return;
    k_dcsb_emit<<<div_up(cnt, BLOCK), BLOCK, 0, st>>>(cnt, skey, sidx, rec, tab, shift, pos, vel, force);
    SALVA_HIP_CHECK(hipGetLastError());
}

}  // namespace salva

// world_query.hip — the particle queries of libsalva_hip (LiquidWorld::particles_intersecting_aabb / _shape): where a query finds its
// particles, the five query kernels, and the host code that runs them and maps their hits to (kind, slot, index) triples.
#include "world.h"
#include "dcs.h"
#include "solid_distance.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace salva {

// LiquidWorld::particles_intersecting_aabb (liquid_world.rs:210-243): particles whose distance to the box is below the
// particle radius.  The reference walks the cells of its (last step's) grid; here every particle's current position is
// tested, which finds the same particles plus those that entered the box's cells since the grid was built.
// Where a query finds its fluid particles.  Single domain: the staging arrays (host order; index = position in the concatenation of
// the fluids).  Decomposed run: the rank's working set after its last step — ghosts are skipped (their owner reports them), the
// index is the particle's GLOBAL id and the fluid slot rides in bits 8.. of the kind word.
struct QuerySrc {
    const float4* pos; uint32_t n;
    const uint32_t* gtag;   // nullptr: no ghosts in `pos`
    const uint32_t* gid;    // nullptr: index = i
    const uint32_t* model;  // nullptr: the slot follows from the index (collect_query)
};
__device__ __forceinline__ bool query_skip(const QuerySrc& q, uint32_t i) { return q.gtag && (q.gtag[i] & 0x80000000u); }
__device__ __forceinline__ void query_emit(const QuerySrc& q, uint32_t i, uint32_t kind, unsigned int* counter, uint32_t cap, uint32_t* out_kind,
                                           uint32_t* out_index) {
    const uint32_t k = atomicAdd(counter, 1u);
    if (k < cap) { out_kind[k] = kind | (q.model ? q.model[i] << 8 : 0u); out_index[k] = q.gid ? q.gid[i] : i; }
}
__global__ __launch_bounds__(BLOCK) void k_aabb_query(QuerySrc q, float3 lo, float3 hi, float r2,
                                                      uint32_t kind, unsigned int* __restrict__ counter, uint32_t cap,
                                                      uint32_t* __restrict__ out_kind, uint32_t* __restrict__ out_index) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= q.n || query_skip(q, i)) return;
    const float4 p = q.pos[i];
    const float dx = fmaxf(fmaxf(lo.x - p.x, p.x - hi.x), 0.0f), dy = fmaxf(fmaxf(lo.y - p.y, p.y - hi.y), 0.0f),
                dz = fmaxf(fmaxf(lo.z - p.z, p.z - hi.z), 0.0f);
    if (!(dx * dx + dy * dy + dz * dz < r2)) return;
    query_emit(q, i, kind, counter, cap, out_kind, out_index);
}
// Single domain: the staging arrays, refreshed from the working set.  Decomposed run (after its first step): the owned particles of
// the working set with their global ids — a query is a per-rank operation there, each rank reports what it owns; the union over
// the ranks is the undivided world's answer (boundary particles near a slab face are held, and reported, by both neighbours).
QuerySrc World::query_fluid_source() {
    if (comm && dist_started && sorted_valid) return QuerySrc{posm[cur].p, n, gtag[cur].p, perm[cur].p, model[cur].p};
    if (comm) throw HipError(SALVA_HIP_E_INVALID, "a query in a decomposed run needs a completed step (global ids exist from then on)");
    ensure_staging_current();
    return QuerySrc{st_pos.p, n, nullptr, nullptr, nullptr};
}

// (kind, global index) pairs collected on the device -> sorted (kind, slot, index-in-slot) triples on the host
uint64_t World::collect_query(unsigned int* d_count, uint32_t* d_kind, uint32_t* d_index, uint32_t cap, uint32_t* kinds, uint32_t* slots,
                              uint32_t* indices) {
    unsigned int total = 0;
    SALVA_HIP_CHECK(hipMemcpyAsync(&total, d_count, sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    const uint32_t m = std::min<uint32_t>(total, cap);
    if (m == 0 || !kinds || !slots || !indices) return total;
    std::vector<uint32_t> hk(m), hi_(m);
    SALVA_HIP_CHECK(hipMemcpy(hk.data(), d_kind, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    SALVA_HIP_CHECK(hipMemcpy(hi_.data(), d_index, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<uint64_t> keys(m);
    for (uint32_t k = 0; k < m; ++k) keys[k] = ((uint64_t)hk[k] << 32) | hi_[k];
    map_query_hits(keys, kinds, slots, indices);
    return total;
}
// (kind word << 32 | global index) keys -> sorted (kind, slot, index-in-slot) triples
void World::map_query_hits(std::vector<uint64_t>& keys, uint32_t* kinds, uint32_t* slots, uint32_t* indices) {
    const uint32_t m = (uint32_t)keys.size();
    std::sort(keys.begin(), keys.end());
    for (uint32_t k = 0; k < m; ++k) {
        uint32_t kind = (uint32_t)(keys[k] >> 32);
        uint64_t g = keys[k] & 0xffffffffull;
        uint32_t s = 0;
        if (comm && (kind & 0xffu) == 0) {  // decomposed run: the slot came with the kind word, the index is a global id
            kinds[k] = 0u; slots[k] = kind >> 8; indices[k] = (uint32_t)g;
            continue;
        }
        kind &= 0xffu;
        if (kind == 0) { while (s + 1 < fluids.size() && g >= fluids[s].n) { g -= fluids[s].n; ++s; } }
        else { while (s + 1 < bounds.size() && g >= bounds[s].n) { g -= bounds[s].n; ++s; } }
        kinds[k] = kind; slots[k] = s; indices[k] = (uint32_t)g;
    }
}

// One query on the device: the hit buffers, the cleared counter, `launch(source, kind, counter, cap, out_kind, out_index)` over the
// fluid particles (kind 0) and over the boundary particles (kind 1), and the hits as triples
template <typename Launch>
uint64_t World::run_query(uint64_t capacity, uint32_t* kinds, uint32_t* slots, uint32_t* indices, Launch&& launch) {
    const QuerySrc qf = query_fluid_source(), qb{bst_pos.p, nb, nullptr, nullptr, nullptr};
    const uint32_t cap = (uint32_t)std::min<uint64_t>(capacity, 0xfffffff0ull);
    DevBuf<unsigned int> cnt;
    DevBuf<uint32_t> dk, di;
    cnt.ensure(1); dk.ensure(std::max(cap, 1u)); di.ensure(std::max(cap, 1u));
    SALVA_HIP_CHECK(hipMemsetAsync(cnt.p, 0, sizeof(unsigned int), stream));
    if (qf.n) launch(qf, 0u, cnt.p, cap, dk.p, di.p);
    if (nb) launch(qb, 1u, cnt.p, cap, dk.p, di.p);
    SALVA_HIP_CHECK(hipGetLastError());
    return collect_query(cnt.p, dk.p, di.p, cap, kinds, slots, indices);
}

uint64_t World::particles_in_aabb(const float mins[3], const float maxs[3], uint64_t capacity, uint32_t* kinds, uint32_t* slots,
                                  uint32_t* indices) {
    use_device();
    const float r = prm.particle_radius;
    const float3 lo = make_float3(mins[0], mins[1], mins[2]), hi = make_float3(maxs[0], maxs[1], maxs[2]);
    return run_query(capacity, kinds, slots, indices, [&](const QuerySrc& q, uint32_t kind, unsigned int* cnt, uint32_t cap, uint32_t* dk, uint32_t* di) {
        k_aabb_query<<<nblk(q.n), BLOCK, 0, stream>>>(q, lo, hi, r * r, kind, cnt, cap, dk, di);
    });
}

// LiquidWorld::particles_intersecting_shape (liquid_world.rs:245-280) for a ball / cuboid posed by (t, q): the particle must lie
// in a grid cell the shape's world AABB touches (hgrid.cells_intersecting_aabb: cell range floor(mins / h) .. floor(maxs / h),
// hgrid.rs:122-133) and `shape.distance_to_point(pos, pt, solid = true) <= particle_radius`.  The point goes into the shape's
// frame with the inverse isometry (conjugate quaternion); ball: max(|p| - radius, 0); cuboid: |max(|p| - half_extents, 0)|.
struct ShapeQuery {
    float t[3], q[4];       // isometry
    int kind; float p[3];   // shape
    int clo[3], chi[3];     // cell range of the world AABB
    float h, r;             // cell width, particle radius
};
__global__ __launch_bounds__(BLOCK) void k_shape_query(QuerySrc q, ShapeQuery s, uint32_t kind,
                                                       unsigned int* __restrict__ counter, uint32_t cap, uint32_t* __restrict__ out_kind,
                                                       uint32_t* __restrict__ out_index) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= q.n || query_skip(q, i)) return;
    const float4 pt = q.pos[i];
    bool bad = false;
    const int cx = cell_coord(pt.x, s.h, bad), cy = cell_coord(pt.y, s.h, bad), cz = cell_coord(pt.z, s.h, bad);
    if (bad || cx < s.clo[0] || cx > s.chi[0] || cy < s.clo[1] || cy > s.chi[1] || cz < s.clo[2] || cz > s.chi[2]) return;
    // inverse isometry: q^-1 * (pt - t)
    const float vx = pt.x - s.t[0], vy = pt.y - s.t[1], vz = pt.z - s.t[2];
    const float qx = -s.q[0], qy = -s.q[1], qz = -s.q[2], qw = s.q[3];
    const float tx = (qy * vz - qz * vy) * 2.0f, ty = (qz * vx - qx * vz) * 2.0f, tz = (qx * vy - qy * vx) * 2.0f;
    const float lx = vx + qw * tx + (qy * tz - qz * ty), ly = vy + qw * ty + (qz * tx - qx * tz), lz = vz + qw * tz + (qx * ty - qy * tx);
    const float d = shape_solid_distance(s.kind, s.p, lx, ly, lz);
    if (!(d <= s.r)) return;
    query_emit(q, i, kind, counter, cap, out_kind, out_index);
}

// The same query for a posed compound and for a posed oriented mesh (the distances: solid_distance.h).  The cell range comes from the posed local box (parry's Aabb::transform_by, dcs.hip).
struct PosedQuery {
    float t[3], q[4];       // isometry
    int clo[3], chi[3];     // cell range of the world AABB
    float h, r;             // cell width, particle radius
};
__device__ __forceinline__ bool posed_query_local(const QuerySrc& q, const PosedQuery& s, uint32_t i, float& lx, float& ly, float& lz) {
    if (i >= q.n || query_skip(q, i)) return false;
    const float4 pt = q.pos[i];
    bool bad = false;
    const int cx = cell_coord(pt.x, s.h, bad), cy = cell_coord(pt.y, s.h, bad), cz = cell_coord(pt.z, s.h, bad);
    if (bad || cx < s.clo[0] || cx > s.chi[0] || cy < s.clo[1] || cy > s.chi[1] || cz < s.clo[2] || cz > s.chi[2]) return false;
    quat_rot(-s.q[0], -s.q[1], -s.q[2], s.q[3], pt.x - s.t[0], pt.y - s.t[1], pt.z - s.t[2], lx, ly, lz);
    return true;
}
__global__ __launch_bounds__(BLOCK) void k_compound_query(QuerySrc q, PosedQuery s, const CompoundPartDev* __restrict__ parts, uint32_t nparts,
                                                          uint32_t kind, unsigned int* __restrict__ counter, uint32_t cap,
                                                          uint32_t* __restrict__ out_kind, uint32_t* __restrict__ out_index) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    float lx, ly, lz;
    if (!posed_query_local(q, s, i, lx, ly, lz)) return;
    const float d = compound_solid_distance(parts, nparts, lx, ly, lz);
    if (!(d <= s.r)) return;
    query_emit(q, i, kind, counter, cap, out_kind, out_index);
}
__global__ __launch_bounds__(BLOCK) void k_mesh_query(QuerySrc q, PosedQuery s, MeshDev mesh, uint32_t kind, unsigned int* __restrict__ counter,
                                                      uint32_t cap, uint32_t* __restrict__ out_kind, uint32_t* __restrict__ out_index) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    float lx, ly, lz;
    if (!posed_query_local(q, s, i, lx, ly, lz)) return;
    if (!(mesh_solid_distance(mesh, lx, ly, lz) <= s.r)) return;
    query_emit(q, i, kind, counter, cap, out_kind, out_index);
}

// ---- a geometry, resolved (world.h Geom)
Geom World::geom_of(const SalvaHipShape& shape) const {
    Geom g;
    g.shape = shape;
    g.kind = shape.kind;
    if (!g.built_in()) g.kind = 0;  // (a handle's kind in a SalvaHipShape is an unknown shape kind like any other)
    return g;
}
Geom World::geom_of(int kind, uint32_t handle) const {
    Geom g;
    g.kind = kind;
    if (kind == SALVA_HIP_SHAPE_MESH) g.mesh = mesh_at(handle);
    else g.compound = compound_at(handle);
    return g;
}
void World::refuse_handle_when_decomposed(const GeomArg& a) const {
    if (a.shape || !(comm && dist_started)) return;
    throw HipError(SALVA_HIP_E_INVALID, a.kind == SALVA_HIP_SHAPE_MESH ? "mesh colliders are not available in a running decomposed world"
                                                                      : "compound colliders are not available in a running decomposed world");
}
// A pose must be a rigid motion (the reference takes an Isometry, which cannot be anything else): NaN / huge values would otherwise
// reach the cell range's float -> int conversion
void check_pose(const float t[3], const float q[4], const char* what) {
    const std::string w(what);
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(t[a])) throw HipError(SALVA_HIP_E_INVALID, w + ": non-finite translation");
    float qn = 0.0f;
    for (int a = 0; a < 4; ++a) {
        if (!std::isfinite(q[a])) throw HipError(SALVA_HIP_E_INVALID, w + ": non-finite rotation");
        qn += q[a] * q[a];
    }
    if (fabsf(qn - 1.0f) > 1.0e-3f) throw HipError(SALVA_HIP_E_INVALID, w + ": the rotation must be a unit quaternion (x, y, z, w)");
}
void check_solid(const Geom& g, const char* what, const char* hint) {
    if (g.solid()) return;
    throw HipError(SALVA_HIP_E_INVALID, std::string(what) + (g.mesh ? ": a mesh without SALVA_HIP_MESH_ORIENTED has no solid distance"
                                                                     : ": a mesh part of the compound lacks SALVA_HIP_MESH_ORIENTED and has no solid distance") + hint);
}

// LiquidWorld::particles_intersecting_shape for any geometry.  What the forms do differently, kept as it was and not yet decided
// (DESIGN.md §19), stands in the lines marked `form:`.
uint64_t World::particles_in(const GeomArg& geom, const float t[3], const float q[4], uint64_t capacity, uint32_t* kinds, uint32_t* slots,
                             uint32_t* indices) {
    use_device();
    if (geom.shape) shape_param_count(geom.shape->kind);  // form: a shape's unknown kind is reported before a bad pose, its parameters after
    refuse_handle_when_decomposed(geom);                   // form: a shape is queried in a running decomposed world, a handle is not
    const Geom g = geom_of(geom);                          // form: an unknown handle and a handle without a solid distance, before a bad pose
    check_solid(g, "shape query", " (use salva_hip_particles_intersecting_host_shape)");
    check_pose(t, q, "shape query");
    if (g.mesh || g.compound) {
        PosedQuery s{};
        for (int a = 0; a < 3; ++a) s.t[a] = t[a];
        for (int a = 0; a < 4; ++a) s.q[a] = q[a];
        s.h = sc.h; s.r = prm.particle_radius;
        float lo[3], hi[3];
        aabb_transform_by(g.mins(), g.maxs(), t, q, lo, hi);  // form: the cell range of the posed local box
        cell_range(lo, hi, sc.h, s.clo, s.chi);
        return run_query(capacity, kinds, slots, indices, [&](const QuerySrc& src, uint32_t kind, unsigned int* cnt, uint32_t cap, uint32_t* dk, uint32_t* di) {
            if (g.mesh) k_mesh_query<<<nblk(src.n), BLOCK, 0, stream>>>(src, s, g.mesh->dev(), kind, cnt, cap, dk, di);
            else k_compound_query<<<nblk(src.n), BLOCK, 0, stream>>>(src, s, g.parts(), g.nparts(), kind, cnt, cap, dk, di);
        });
    }
    const SalvaHipShape& shape = g.shape;
    check_shape_params(shape, "shape query: radius / half extents must be positive and finite");  // (the shape non-degenerate, likewise)
    ShapeQuery s{};
    for (int a = 0; a < 3; ++a) { s.t[a] = t[a]; s.p[a] = shape.params[a]; }
    for (int a = 0; a < 4; ++a) s.q[a] = q[a];
    s.kind = shape.kind; s.h = sc.h; s.r = prm.particle_radius;
    // form: the cell range of the world AABB about the centre (parry compute_aabb; dcs.hip), and a kernel of its own — it rotates into
    // the local frame in another order of operations than quat_rot, and a hit is decided by d <= r
    float ext[3], lo[3], hi[3];
    shape_world_extent(shape, q, ext);
    for (int a = 0; a < 3; ++a) { lo[a] = t[a] - ext[a]; hi[a] = t[a] + ext[a]; }
    cell_range(lo, hi, sc.h, s.clo, s.chi);
    return run_query(capacity, kinds, slots, indices, [&](const QuerySrc& src, uint32_t kind, unsigned int* cnt, uint32_t cap, uint32_t* dk, uint32_t* di) {
        k_shape_query<<<nblk(src.n), BLOCK, 0, stream>>>(src, s, kind, cnt, cap, dk, di);
    });
}

// LiquidWorld::particles_intersecting_shape for a shape whose geometry stays with the host (any parry `Shape`: the reference's
// query is generic, liquid_world.rs:247-280): the two parry calls — `shape.compute_aabb(pos)` and `shape.distance_to_point(pos,
// &pt, true)` — are callbacks; the device keeps the cell filter (hgrid.cells_intersecting_aabb, hgrid.rs:122-133) and hands the
// particles of those cells to the host in one copy.
__global__ __launch_bounds__(BLOCK) void k_cell_range_query(QuerySrc q, int clo0, int clo1, int clo2, int chi0, int chi1, int chi2, float h,
                                                            uint32_t kind, unsigned int* __restrict__ counter, uint32_t cap,
                                                            uint32_t* __restrict__ out_kind, uint32_t* __restrict__ out_index,
                                                            float4* __restrict__ out_pos) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= q.n || query_skip(q, i)) return;
    const float4 pt = q.pos[i];
    bool bad = false;
    const int cx = cell_coord(pt.x, h, bad), cy = cell_coord(pt.y, h, bad), cz = cell_coord(pt.z, h, bad);
    if (bad || cx < clo0 || cx > chi0 || cy < clo1 || cy > chi1 || cz < clo2 || cz > chi2) return;
    const uint32_t k = atomicAdd(counter, 1u);
    if (k < cap) { out_kind[k] = kind | (q.model ? q.model[i] << 8 : 0u); out_index[k] = q.gid ? q.gid[i] : i; out_pos[k] = pt; }
}
uint64_t World::particles_in_host_shape(const SalvaHipHostQueryShape& shape, uint64_t capacity, uint32_t* kinds, uint32_t* slots,
                                        uint32_t* indices) {
    use_device();
    if (!shape.aabb || !shape.distance) throw HipError(SALVA_HIP_E_INVALID, "a host query shape needs both callbacks");
    float mins[3], maxs[3];
    shape.aabb(shape.user, mins, maxs);
    int clo[3], chi[3];
    for (int a = 0; a < 3; ++a)
        if (!(mins[a] <= maxs[a]) || !std::isfinite(mins[a]) || !std::isfinite(maxs[a]))
            throw HipError(SALVA_HIP_E_INVALID, "host query shape: the aabb callback returned an empty, infinite or NaN box");
    cell_range(mins, maxs, sc.h, clo, chi);
    const QuerySrc qf = query_fluid_source(), qb{bst_pos.p, nb, nullptr, nullptr, nullptr};
    // Candidates go into scratch buffers the world keeps (three fresh (n + nb)-sized buffers per call were 190 MB at
    // 8 x 10^6 particles, allocated and freed synchronously): sized for what queries have needed so far; the kernel counts every
    // candidate and stores those that fit, so a box that holds more than the buffers do costs one repetition with room.
    const uint32_t all = qf.n + nb;
    unsigned int m = 0;
    for (int attempt = 0;; ++attempt) {
        const uint32_t ccap = std::min<uint32_t>(std::max<uint32_t>(hq_need, 65536u), std::max(all, 1u));
        hq_cnt.ensure(1); hq_kind.ensure(ccap, stream, false, 1.25f); hq_index.ensure(ccap, stream, false, 1.25f); hq_pos.ensure(ccap, stream, false, 1.25f);
        SALVA_HIP_CHECK(hipMemsetAsync(hq_cnt.p, 0, sizeof(unsigned int), stream));
        if (qf.n) k_cell_range_query<<<nblk(qf.n), BLOCK, 0, stream>>>(qf, clo[0], clo[1], clo[2], chi[0], chi[1], chi[2], sc.h, 0u, hq_cnt.p, ccap, hq_kind.p, hq_index.p, hq_pos.p);
        if (nb) k_cell_range_query<<<nblk(nb), BLOCK, 0, stream>>>(qb, clo[0], clo[1], clo[2], chi[0], chi[1], chi[2], sc.h, 1u, hq_cnt.p, ccap, hq_kind.p, hq_index.p, hq_pos.p);
        SALVA_HIP_CHECK(hipGetLastError());
        SALVA_HIP_CHECK(hipMemcpyAsync(&m, hq_cnt.p, sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
        if (m <= ccap) break;
        if (attempt >= 1) throw HipError(SALVA_HIP_E_HIP, "internal error: the candidate count of a host shape query grew between two passes");
        hq_need = m + m / 4u;
    }
    DevBuf<uint32_t>& dk = hq_kind; DevBuf<uint32_t>& di = hq_index; DevBuf<float4>& dp = hq_pos;
    if (m == 0) return 0;
    std::vector<uint32_t> hk(m), hi_(m);
    std::vector<float4> hp(m);
    SALVA_HIP_CHECK(hipMemcpy(hk.data(), dk.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    SALVA_HIP_CHECK(hipMemcpy(hi_.data(), di.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    SALVA_HIP_CHECK(hipMemcpy(hp.data(), dp.p, m * sizeof(float4), hipMemcpyDeviceToHost));
    std::vector<float> pts(3 * (size_t)m), dist((size_t)m, std::numeric_limits<float>::infinity());
    for (unsigned int k = 0; k < m; ++k) { pts[3 * k] = hp[k].x; pts[3 * k + 1] = hp[k].y; pts[3 * k + 2] = hp[k].z; }
    shape.distance(shape.user, m, pts.data(), dist.data());
    std::vector<uint64_t> keys;
    keys.reserve(m);
    for (unsigned int k = 0; k < m; ++k)
        if (dist[k] <= prm.particle_radius) keys.push_back(((uint64_t)hk[k] << 32) | hi_[k]);  // liquid_world.rs:263, :272 (NaN: not a hit)
    const uint64_t total = keys.size();
    if (total == 0 || !kinds || !slots || !indices) return total;
    if (keys.size() > capacity) {  // the first `capacity` in the sorted order, like the device arms
        std::sort(keys.begin(), keys.end());
        keys.resize((size_t)capacity);
    }
    map_query_hits(keys, kinds, slots, indices);
    return total;
}

}  // namespace salva

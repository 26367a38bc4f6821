// fluidcast.hip — the walk of a ray through a cast's own cell table (fluidcast.h; the contract: include/salva_hip.h).
//
// One lane per ray.  The ray is advanced to the box G first (o' = o + ta d), so that everything below is bounded by the size of the box
// and not by the distance of the camera.  The walk goes by slices of cells along the ray's dominant axis k (the largest |d|, the lower
// index on a tie), from the slice of o' - (R + eps) to the face of the grid the ray travels towards: the trip count is an integer
// number of slices of the grid, whatever the floats say.  In slice s, between the planes x_k = (o_k + s) h and (o_k + s + 1) h, the
// ray covers an interval of each of the other two axes; a particle of that slice whose sphere the ray can meet lies within
// sqrt(3) (R + error) of that interval on either axis (the point of the ray at the particle's own x_k is at most sqrt(3)
// times the ray's distance away, because d_k is the largest component).  The interval is dilated by D = 1.75 R + eps and every cell
// it touches is tested with the exact cast of the contract.  Cell indices are computed as the table computed them, floor(x / h) with the
// f32 division, which is monotone: no fuzz on those two axes.  eps = 2^-19 (max |coordinate| of G + the extents of G) covers the f32
// error of p in ray_ball, of the planes and of the interval's ends (32 units of 2^-24 of that magnitude; §22 counts 22).
// A first-hit walk stops before a slice whose earliest possible entry, ((near plane -+ (R + eps)) - o'_k) / d_k, added to ta, lies
// behind the best t: a later particle cannot come earlier or tie.  A walk that sums the thickness visits every slice; every cell is
// visited at most once per ray, so no particle is counted twice.  No LDS, no atomics, plain stores.
#include "fluidcast.h"
#include "raycast.h"

namespace salva {

float cast_eps(const float glo[3], const float ghi[3]) {
    float m = 0.0f, e = 0.0f;
    for (int a = 0; a < 3; ++a) {
        m = fmaxf(m, fmaxf(fabsf(glo[a]), fabsf(ghi[a])));
        e += ghi[a] - glo[a];
    }
    return (m + e) * 1.9073486328125e-06f;  // 2^-19 (a margin: its last bit matters to nothing)
}

__device__ __forceinline__ float cast_sel3(int k, float x, float y, float z) { return k == 0 ? x : (k == 1 ? y : z); }
__device__ __forceinline__ uint32_t cast_sel3u(int k, uint32_t x, uint32_t y, uint32_t z) { return k == 0 ? x : (k == 1 ? y : z); }

// floor(x / h) - o as the table computes it (tile.h cell_coord), not yet clamped to the grid; NaN: `nan_cell`
__device__ __forceinline__ long long cast_cell(float x, float h, int o, long long nan_cell) {
    float f = floorf(__fdiv_rn(x, h));
    if (!(f == f)) return nan_cell;
    f = fminf(fmaxf(f, -1073741824.0f), 1073741824.0f);
    return (long long)(int)f - (long long)o;
}

__device__ __forceinline__ void cast_store_miss(const CastOutDev& out, uint64_t i) {
    if (out.t) out.t[i] = __builtin_inff();
    if (out.fluid) out.fluid[i] = CAST_NONE;
    if (out.index) out.index[i] = CAST_NONE;
    if (out.normal) { out.normal[3 * i] = 0.0f; out.normal[3 * i + 1] = 0.0f; out.normal[3 * i + 2] = 0.0f; }
    if (out.thickness) out.thickness[i] = 0.0f;
    if (out.tested) out.tested[i] = 0u;
}

__global__ __launch_bounds__(BLOCK) void k_fluid_cast_miss(uint64_t nrays, CastOutDev out) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < nrays) cast_store_miss(out, i);
}
void launch_fluid_cast_miss(uint64_t nrays, const CastOutDev& out, hipStream_t st) {
    if (!nrays) return;
    k_fluid_cast_miss<<<div_up(nrays, BLOCK), BLOCK, 0, st>>>(nrays, out);
    SALVA_HIP_CHECK(hipGetLastError());
}

// COUNT: the instance behind salva_hip_count_ray_candidates - the same walk, and besides it the number of exact casts the lane made,
// a plain store per ray
template <bool HIT, bool THICK, bool COUNT>
__global__ __launch_bounds__(BLOCK) void k_fluid_cast(CastRays rays, CastParams P, FieldGrid g, CastTable tab, CastOutDev out) {
#pragma clang fp contract(off)
    const uint64_t tid = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint64_t i;
    float ox, oy, oz, dx, dy, dz;
    if (rays.origins) {
        i = tid;
        if (i >= rays.nrays) return;
        ox = rays.origins[3 * i]; oy = rays.origins[3 * i + 1]; oz = rays.origins[3 * i + 2];
        dx = rays.directions[3 * i]; dy = rays.directions[3 * i + 1]; dz = rays.directions[3 * i + 2];
    } else {
        // a wave takes a tile of 8 x 8 pixels, so that its lanes walk the same cells
        const uint64_t wave = tid / WAVE;
        const uint32_t lane = (uint32_t)(tid & (WAVE - 1)), tiles_x = (rays.width + CAST_TILE - 1u) / CAST_TILE;
        const uint64_t ty = wave / tiles_x;
        const uint32_t ix = (uint32_t)(wave % tiles_x) * CAST_TILE + (lane & (CAST_TILE - 1u));
        const uint64_t iy = ty * CAST_TILE + (lane / CAST_TILE);
        if (ix >= rays.width || iy >= rays.height) return;
        i = iy * rays.width + ix;
        // (no FMA: the pragma above, and the file's -ffp-contract=off)
        const float su = (((float)ix + 0.5f) * (2.0f / (float)rays.width)) - 1.0f;
        const float sv = (((float)(uint32_t)iy + 0.5f) * (2.0f / (float)rays.height)) - 1.0f;
        ox = rays.cam_o[0]; oy = rays.cam_o[1]; oz = rays.cam_o[2];
        dx = (rays.cam_f[0] + (su * rays.cam_r[0])) + (sv * rays.cam_u[0]);
        dy = (rays.cam_f[1] + (su * rays.cam_r[1])) + (sv * rays.cam_u[1]);
        dz = (rays.cam_f[2] + (su * rays.cam_r[2])) + (sv * rays.cam_u[2]);
    }
    const float inf = __builtin_inff();
    const float dd = ray_dot(dx, dy, dz, dx, dy, dz);
    bool live = isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(dx) && isfinite(dy) && isfinite(dz) && isfinite(dd) && dd > 0.0f;
    // the advance: the ray's interval in G, axis by axis
    float ta = 0.0f;
    if (live) {
        float t0 = -inf, t1 = inf;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float o = cast_sel3(a, ox, oy, oz), d = cast_sel3(a, dx, dy, dz);
            if (d == 0.0f) {
                live = live && o >= P.glo[a] && o <= P.ghi[a];
            } else {
                const float u = (P.glo[a] - o) / d, v = (P.ghi[a] - o) / d;
                t0 = fmaxf(t0, fminf(u, v)); t1 = fminf(t1, fmaxf(u, v));
            }
        }
        live = live && t0 <= t1 && !(t1 < 0.0f) && !(t0 > P.tmax);
        ta = fmaxf(t0, 0.0f);
    }
    if (!live) {
        cast_store_miss(out, i);
        return;
    }
    const float px = ox + (ta * dx), py = oy + (ta * dy), pz = oz + (ta * dz);

    const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
    const int k = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    // the axes (k, a, b) = (k, k + 1, k + 2) mod 3
    const float dk = cast_sel3(k, dx, dy, dz), da = cast_sel3(k, dy, dz, dx), db = cast_sel3(k, dz, dx, dy);
    const float pk = cast_sel3(k, px, py, pz), pa = cast_sel3(k, py, pz, px), pb = cast_sel3(k, pz, px, py);
    const int ok = k == 0 ? g.o[0] : (k == 1 ? g.o[1] : g.o[2]), oa = k == 0 ? g.o[1] : (k == 1 ? g.o[2] : g.o[0]),
              ob = k == 0 ? g.o[2] : (k == 1 ? g.o[0] : g.o[1]);
    const uint32_t nk = cast_sel3u(k, g.d[0], g.d[1], g.d[2]), na = cast_sel3u(k, g.d[1], g.d[2], g.d[0]), nb = cast_sel3u(k, g.d[2], g.d[0], g.d[1]);
    const uint32_t sx = g.d[1] * g.d[2], sy = g.d[2];
    const uint32_t stk = cast_sel3u(k, sx, sy, 1u), sta = cast_sel3u(k, sy, 1u, sx), stb = cast_sel3u(k, 1u, sx, sy);
    const float h = g.h, reach = P.radius + P.eps, dil = (1.75f * P.radius) + P.eps;
    const bool fwd = dk > 0.0f;

    // the slices: from the one of o' - (R + eps) against the direction of travel to the grid's face
    long long s_first = cast_cell(fwd ? pk - reach : pk + reach, h, ok, fwd ? 0ll : (long long)nk - 1);
    s_first = s_first < 0 ? 0 : (s_first > (long long)nk - 1 ? (long long)nk - 1 : s_first);
    const uint32_t s0 = (uint32_t)s_first, nslices = fwd ? nk - s0 : s0 + 1u;

    float best_t = inf, thick = 0.0f;
    uint32_t best_row = CAST_NONE, best_at = 0u, tested = 0u;
    for (uint32_t it = 0; it < nslices; ++it) {
        const uint32_t s = fwd ? s0 + it : s0 - it;
        const float plo = (float)(ok + (int)s) * h, phi = (float)(ok + (int)s + 1) * h;
        if (HIT && !THICK && it > 0u && best_row != CAST_NONE) {
            const float edge = fwd ? plo - reach : phi + reach;
            const float tlb = (edge - pk) / dk;
            if (best_t < ta + tlb) break;
        }
        const float ua = (plo - pk) / dk, ub = (phi - pk) / dk;
        const float a0 = pa + (ua * da), a1 = pa + (ub * da), b0 = pb + (ua * db), b1 = pb + (ub * db);
        long long ca0 = cast_cell(fminf(a0, a1) - dil, h, oa, 0ll), ca1 = cast_cell(fmaxf(a0, a1) + dil, h, oa, (long long)na - 1);
        long long cb0 = cast_cell(fminf(b0, b1) - dil, h, ob, 0ll), cb1 = cast_cell(fmaxf(b0, b1) + dil, h, ob, (long long)nb - 1);
        if (ca0 < 0) ca0 = 0;
        if (cb0 < 0) cb0 = 0;
        if (ca1 > (long long)na - 1) ca1 = (long long)na - 1;
        if (cb1 > (long long)nb - 1) cb1 = (long long)nb - 1;
        for (long long ca = ca0; ca <= ca1; ++ca)
            for (long long cb = cb0; cb <= cb1; ++cb) {
                const uint32_t cell = s * stk + (uint32_t)ca * sta + (uint32_t)cb * stb;
                const uint32_t b = tab.cells[cell], e = tab.cells[cell + 1u];
                for (uint32_t p = b; p < e; ++p) {
                    const float4 r = tab.rec0[p];
                    if (!(r.x >= P.blo[0] && r.x <= P.bhi[0] && r.y >= P.blo[1] && r.y <= P.bhi[1] && r.z >= P.blo[2] && r.z <= P.bhi[2])) continue;
                    float t0, t1;
                    if (COUNT) ++tested;
                    ray_ball(px - r.x, py - r.y, pz - r.z, dx, dy, dz, P.radius, t0, t1);
                    const float tj = ta + fmaxf(t0, 0.0f);
                    if (THICK) thick += fmaxf(0.0f, fminf(ta + t1, P.tmax) - tj);
                    if (HIT && t1 >= 0.0f && tj <= P.tmax && tj <= best_t) {
                        const uint32_t row = tab.rows[p];
                        if (tj < best_t || row < best_row) { best_t = tj; best_row = row; best_at = p; }
                    }
                }
            }
    }
    if (COUNT) out.tested[i] = tested;
    if (THICK && out.thickness) out.thickness[i] = thick;
    if (!HIT) return;
    if (best_row == CAST_NONE) {
        CastOutDev o2 = out;
        o2.thickness = nullptr; o2.tested = nullptr;
        cast_store_miss(o2, i);
        return;
    }
    if (out.t) out.t[i] = best_t;
    if (out.fluid || out.index) {
        const uint32_t m = tab.st_model[best_row] & (FIELD_MAX_SLOTS - 1u);
        uint32_t first = 0u;
#pragma unroll
        for (uint32_t q = 0; q < FIELD_MAX_SLOTS; ++q) first = q == m ? tab.first[q] : first;
        if (out.fluid) out.fluid[i] = m;
        if (out.index) out.index[i] = best_row - first;
    }
    if (out.normal) {
        const float4 r = tab.rec0[best_at];
        const float w = best_t - ta;
        const float gx = (px - r.x) + (w * dx), gy = (py - r.y) + (w * dy), gz = (pz - r.z) + (w * dz);
        // scaled by the largest component first, as surface.hip k_surface_normals
        const float m = fmaxf(fabsf(gx), fmaxf(fabsf(gy), fabsf(gz)));
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        if (m > 0.0f && isfinite(m)) {
            const float ux = gx / m, uy = gy / m, uz = gz / m;
            const float len = sqrtf(ux * ux + uy * uy + uz * uz);
            nx = ux / len; ny = uy / len; nz = uz / len;
        }
        out.normal[3 * i] = nx; out.normal[3 * i + 1] = ny; out.normal[3 * i + 2] = nz;
    }
}

void launch_fluid_cast(const CastRays& rays, const CastParams& p, const FieldGrid& g, const CastTable& tab, const CastOutDev& out, bool hit,
                       bool thick, hipStream_t st) {
    uint64_t lanes = rays.nrays;
    if (!rays.origins) lanes = (uint64_t)div_up(rays.width, CAST_TILE) * div_up(rays.height, CAST_TILE) * WAVE;
    if (!lanes || !(hit || thick)) return;
    const uint64_t blocks = (lanes + BLOCK - 1) / BLOCK;
    if (blocks > 0x7fffffffull) throw HipError(SALVA_HIP_E_CAPACITY, "ray cast: more rays than one launch takes; split the call");
    if (out.tested && hit) k_fluid_cast<true, false, true><<<(unsigned)blocks, BLOCK, 0, st>>>(rays, p, g, tab, out);
    else if (out.tested) k_fluid_cast<false, true, true><<<(unsigned)blocks, BLOCK, 0, st>>>(rays, p, g, tab, out);
    else if (hit && thick) k_fluid_cast<true, true, false><<<(unsigned)blocks, BLOCK, 0, st>>>(rays, p, g, tab, out);
    else if (hit) k_fluid_cast<true, false, false><<<(unsigned)blocks, BLOCK, 0, st>>>(rays, p, g, tab, out);
    else k_fluid_cast<false, true, false><<<(unsigned)blocks, BLOCK, 0, st>>>(rays, p, g, tab, out);
    SALVA_HIP_CHECK(hipGetLastError());
}

}  // namespace salva

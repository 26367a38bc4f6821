// diffuse.hip — the potentials of diffuse particles (include/salva_hip.h "Diffuse particles").  k_diffuse_sums: one lane
// per particle over the 27 cells of width h around it — nine runs of three contiguous cells in the sorted records of the field
// evaluator's table (field.hip) —, the neighbour count, the trapped-air sum and the gradient of the colour field in registers, then the
// normal and the energy.  k_diffuse_crest: the same walk once more, reading the neighbours' normals where pass 1 left them in sorted
// order.  Every sum is a named scalar; no LDS, no scratch (tests/test_diffuse_resources.py).  Both kernels visit cells in ascending
// order and rows in ascending host index within a cell: the order of every sum is fixed.
//
// Compiled once, like field.hip, with the reference's other kernels switched in as wave-uniform branches of kernel_eval.
#define SALVA_OTHER_KERNELS 1
#include "diffuse.h"
#include "tile.h"

namespace salva {

// the cell of a position in g (field.hip field_cell); false: outside or not finite
__device__ __forceinline__ bool diffuse_cell(const FieldGrid& g, float x, float y, float z, uint32_t& ux, uint32_t& uy, uint32_t& uz) {
    bool bad = false;
    const int cx = cell_coord(x, g.h, bad), cy = cell_coord(y, g.h, bad), cz = cell_coord(z, g.h, bad);
    ux = (uint32_t)cx - (uint32_t)g.o[0]; uy = (uint32_t)cy - (uint32_t)g.o[1]; uz = (uint32_t)cz - (uint32_t)g.o[2];
    return !bad && isfinite(x) && isfinite(y) && isfinite(z) && ux < g.d[0] && uy < g.d[1] && uz < g.d[2];
}
// dot(a, b) = ((ax bx) + (ay by)) + (az bz), every product and sum rounded in f32 (dist2_exact's device)
__device__ __forceinline__ float dot_exact(float ax, float ay, float az, float bx, float by, float bz) {
    float xx = ax * bx, yy = ay * by, zz = az * bz;
    asm volatile("" : "+v"(xx), "+v"(yy), "+v"(zz));
    float xy = xx + yy;
    asm volatile("" : "+v"(xy));
    return xy + zz;
}

__global__ __launch_bounds__(BLOCK) void k_diffuse_sums(uint32_t n, FieldGrid g, FieldCandidates cand, const uint32_t* __restrict__ rows, SphConsts c,
                                                        DiffuseParams prm, uint32_t want, DiffuseRows out) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n || p >= cand.cells[g.ncells]) return;  // (cells[ncells]: the kept rows)
    const uint32_t v = rows[p];
    if (v >= n) return;
    const float4 xi = cand.rec0[p];
    const float4 vi = cand.rec1 ? cand.rec1[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // (null, uniformly: the count alone is wanted)
    uint32_t ux, uy, uz;
    if (!diffuse_cell(g, xi.x, xi.y, xi.z, ux, uy, uz)) return;  // (cannot happen: the row was sorted into g by this test)
    const bool want_ta = (want & DIFFUSE_WANT_TRAPPED) != 0u, want_n = (want & (DIFFUSE_WANT_NORMAL | DIFFUSE_WANT_CREST)) != 0u;  // (uniform)
    float ta = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
    uint32_t cnt = 0;
    const uint32_t x0 = ux ? ux - 1u : 0u, x1 = min(ux + 1u, g.d[0] - 1u), y0 = uy ? uy - 1u : 0u, y1 = min(uy + 1u, g.d[1] - 1u),
                   z0 = uz ? uz - 1u : 0u, z1 = min(uz + 1u, g.d[2] - 1u);
    for (uint32_t cx = x0; cx <= x1; ++cx)
        for (uint32_t cy = y0; cy <= y1; ++cy) {
            const uint32_t row = (cx * g.d[1] + cy) * g.d[2];
            const uint32_t b = cand.cells[row + z0], e = min(cand.cells[row + z1 + 1u], n);
            for (uint32_t j = b; j < e; ++j) {
                const float4 xj = cand.rec0[j];
                const float dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
                const float r2 = dist2_exact(dx, dy, dz);
                if (!(r2 <= c.h2) || j == p) continue;
                cnt += 1u;
                if (!(want_ta || want_n)) continue;
                const float4 vj = cand.rec1[j];  // (v_j, V_j)
                if (want_ta) {
                    const float wx = vi.x - vj.x, wy = vi.y - vj.y, wz = vi.z - vj.z;
                    const float ww = dist2_exact(wx, wy, wz);
                    if (ww > 0.0f && r2 > 0.0f) {
                        const float wn = sqrtf(ww), r = sqrtf(r2);
                        const float cosine = fminf(fmaxf((dot_exact(wx, wy, wz, dx, dy, dz) / wn) / r, -1.0f), 1.0f);
                        ta += (wn * (1.0f - cosine)) * (1.0f - r / c.h);
                    }
                }
                if (want_n) {
                    const float vg = vj.w * kernel_eval(r2, c).g;
                    gx += vg * dx; gy += vg * dy; gz += vg * dz;
                }
            }
        }
    float4 nrm = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (want_n) {
        const float gn = sqrtf(dist2_exact(gx, gy, gz));
        if (gn > 0.0f && c.h * gn >= prm.surface_min) nrm = make_float4(-gx / gn, -gy / gn, -gz / gn, 1.0f);
        out.normal_sorted[p] = nrm;
        out.normal[v] = nrm;
    }
    const float energy = (0.5f * xi.w) * dist2_exact(vi.x, vi.y, vi.z);  // (xi.w: m_i = V_i density0, one f32 product)
    out.a[v] = make_float4(ta, energy, 0.0f, __uint_as_float(cnt));
}
void launch_diffuse_sums(uint32_t n, const FieldGrid& g, const FieldCandidates& cand, const uint32_t* rows, const SphConsts& c, const DiffuseParams& prm,
                         uint32_t want, const DiffuseRows& out, hipStream_t st) {
    if (!n) return;
    k_diffuse_sums<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, g, cand, rows, c, prm, want, out);
    SALVA_HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(BLOCK) void k_diffuse_crest(uint32_t n, FieldGrid g, FieldCandidates cand, const uint32_t* __restrict__ rows, SphConsts c,
                                                         DiffuseParams prm, DiffuseRows out) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n || p >= cand.cells[g.ncells]) return;
    const uint32_t v = rows[p];
    if (v >= n) return;
    const float4 ni = out.normal_sorted[p];
    if (ni.w == 0.0f) return;  // (a[v].z stays 0)
    const float4 xi = cand.rec0[p], vi = cand.rec1[p];
    const float vv = dist2_exact(vi.x, vi.y, vi.z);
    if (!(vv > 0.0f)) return;
    if (!(dot_exact(vi.x, vi.y, vi.z, ni.x, ni.y, ni.z) / sqrtf(vv) >= prm.crest_cos)) return;
    uint32_t ux, uy, uz;
    if (!diffuse_cell(g, xi.x, xi.y, xi.z, ux, uy, uz)) return;
    float kappa = 0.0f;
    const uint32_t x0 = ux ? ux - 1u : 0u, x1 = min(ux + 1u, g.d[0] - 1u), y0 = uy ? uy - 1u : 0u, y1 = min(uy + 1u, g.d[1] - 1u),
                   z0 = uz ? uz - 1u : 0u, z1 = min(uz + 1u, g.d[2] - 1u);
    for (uint32_t cx = x0; cx <= x1; ++cx)
        for (uint32_t cy = y0; cy <= y1; ++cy) {
            const uint32_t row = (cx * g.d[1] + cy) * g.d[2];
            const uint32_t b = cand.cells[row + z0], e = min(cand.cells[row + z1 + 1u], n);
            for (uint32_t j = b; j < e; ++j) {
                const float4 xj = cand.rec0[j];
                const float dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
                const float r2 = dist2_exact(dx, dy, dz);
                if (!(r2 <= c.h2) || j == p) continue;
                // x_ji . n_i < 0 with x_ji = -(x_i - x_j): the sign of the dot product of the unit vector, and no division
                if (!(dot_exact(dx, dy, dz, ni.x, ni.y, ni.z) > 0.0f)) continue;
                const float4 nj = out.normal_sorted[j];
                if (nj.w == 0.0f) continue;
                kappa += (1.0f - fminf(dot_exact(ni.x, ni.y, ni.z, nj.x, nj.y, nj.z), 1.0f)) * (1.0f - sqrtf(r2) / c.h);
            }
        }
    float4 a = out.a[v];
    a.z = kappa;
    out.a[v] = a;
}
void launch_diffuse_crest(uint32_t n, const FieldGrid& g, const FieldCandidates& cand, const uint32_t* rows, const SphConsts& c, const DiffuseParams& prm,
                          const DiffuseRows& out, hipStream_t st) {
    if (!n) return;
    k_diffuse_crest<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, g, cand, rows, c, prm, out);
    SALVA_HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(BLOCK) void k_diffuse_pack(uint32_t n, const uint32_t* __restrict__ st_model, RowPack pk, DiffuseRows in,
                                                        float* __restrict__ trapped_air, float* __restrict__ wave_crest, float* __restrict__ energy,
                                                        float* __restrict__ normal, uint32_t* __restrict__ count) {
    const uint32_t v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= n) return;
    const uint32_t s = st_model[v];
    if (s >= FIELD_MAX_SLOTS || !((pk.mask >> s) & 1u) || v < pk.first[s] || v - pk.first[s] >= pk.len[s]) return;
    const uint64_t r = (uint64_t)pk.base[s] + (v - pk.first[s]);
    const float4 a = in.a[v];
    if (trapped_air) trapped_air[r] = a.x;
    if (energy) energy[r] = a.y;
    if (wave_crest) wave_crest[r] = a.z;
    if (count) count[r] = __float_as_uint(a.w);
    if (normal) {
        const float4 nv = in.normal[v];
        normal[3 * r] = nv.x; normal[3 * r + 1] = nv.y; normal[3 * r + 2] = nv.z;
    }
}
void launch_diffuse_pack(uint32_t n, const uint32_t* st_model, const RowPack& pk, const DiffuseRows& in, float* trapped_air, float* wave_crest,
                         float* energy, float* normal, uint32_t* count, hipStream_t st) {
    if (!n) return;
    k_diffuse_pack<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, st_model, pk, in, trapped_air, wave_crest, energy, normal, count);
    SALVA_HIP_CHECK(hipGetLastError());
}


// ------------------------------------------------------------------------------------------------ the diffuse set
__global__ __launch_bounds__(BLOCK) void k_diffuse_add(uint32_t n, const float* __restrict__ pos, const float* __restrict__ vel,
                                                       const float* __restrict__ lifetimes, float life, uint32_t at, uint32_t first_id,
                                                       DiffuseSetDev set) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    set.pos[at + i] = make_float4(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], lifetimes ? lifetimes[i] : life);
    set.vel[at + i] = make_float4(vel[3 * i], vel[3 * i + 1], vel[3 * i + 2], __uint_as_float((uint32_t)SALVA_HIP_DIFFUSE_NEW));
    set.id[at + i] = first_id + i;
}
void launch_diffuse_add(uint32_t n, const float* pos, const float* vel, const float* lifetimes, float life, uint32_t at, uint32_t first_id,
                        const DiffuseSetDev& set, hipStream_t st) {
    if (!n) return;
    k_diffuse_add<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, pos, vel, lifetimes, life, at, first_id, set);
    SALVA_HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(BLOCK) void k_diffuse_get(uint32_t n, DiffuseSetDev set, float* __restrict__ pos, float* __restrict__ vel,
                                                       float* __restrict__ life, uint32_t* __restrict__ kind, uint32_t* __restrict__ id) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 x = set.pos[i], v = set.vel[i];
    if (pos) { pos[3 * i] = x.x; pos[3 * i + 1] = x.y; pos[3 * i + 2] = x.z; }
    if (vel) { vel[3 * i] = v.x; vel[3 * i + 1] = v.y; vel[3 * i + 2] = v.z; }
    if (life) life[i] = x.w;
    if (kind) kind[i] = __float_as_uint(v.w);
    if (id) id[i] = set.id[i];
}
void launch_diffuse_get(uint32_t n, const DiffuseSetDev& set, float* pos, float* vel, float* life, uint32_t* kind, uint32_t* id, hipStream_t st) {
    if (!n) return;
    k_diffuse_get<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, set, pos, vel, life, kind, id);
    SALVA_HIP_CHECK(hipGetLastError());
}
void launch_diffuse_set_points(uint32_t n, const DiffuseSetDev& set, float* pts, hipStream_t st) {
    launch_diffuse_get(n, set, pts, nullptr, nullptr, nullptr, nullptr, st);
}

// one count per wave and kind of removal or survival, not one per lane
__device__ __forceinline__ void diffuse_tally(bool mine, uint32_t* counter) {
    const unsigned long long m = __ballot(mine);
    if (m && (threadIdx.x & (WAVE - 1)) == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(counter, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(BLOCK) void k_diffuse_advect(uint32_t n, DiffuseSetDev set, const float* __restrict__ fv, const uint32_t* __restrict__ fc,
                                                          DiffuseParams prm, float dt, uint32_t* __restrict__ keep, DiffuseCounters* counters) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    bool killed = false, dissolved = false;
    if (i < n) {
        float4 x = set.pos[i], v = set.vel[i];
        const uint32_t cnt = fc[i];
        uint32_t kind;
        if (cnt < prm.n_spray) {
            kind = SALVA_HIP_DIFFUSE_SPRAY;
            v.x = v.x + dt * prm.gravity[0]; v.y = v.y + dt * prm.gravity[1]; v.z = v.z + dt * prm.gravity[2];
        } else if (cnt <= prm.n_bubble) {
            kind = SALVA_HIP_DIFFUSE_FOAM;
            v.x = fv[3 * i]; v.y = fv[3 * i + 1]; v.z = fv[3 * i + 2];
            x.w = x.w - dt;
        } else {
            kind = SALVA_HIP_DIFFUSE_BUBBLE;
            const float b = dt * prm.k_b;
            v.x = (v.x - b * prm.gravity[0]) + prm.k_d * (fv[3 * i] - v.x);
            v.y = (v.y - b * prm.gravity[1]) + prm.k_d * (fv[3 * i + 1] - v.y);
            v.z = (v.z - b * prm.gravity[2]) + prm.k_d * (fv[3 * i + 2] - v.z);
        }
        x.x = x.x + dt * v.x; x.y = x.y + dt * v.y; x.z = x.z + dt * v.z;
        v.w = __uint_as_float(kind);
        set.pos[i] = x;
        set.vel[i] = v;
        killed = !(isfinite(x.x) && isfinite(x.y) && isfinite(x.z));
        if (prm.has_kill_box)
            killed = killed || x.x < prm.kill_lo[0] || x.x > prm.kill_hi[0] || x.y < prm.kill_lo[1] || x.y > prm.kill_hi[1] || x.z < prm.kill_lo[2] ||
                     x.z > prm.kill_hi[2];
        dissolved = !killed && x.w <= 0.0f;
        keep[i] = (killed || dissolved) ? 0u : 1u;
    }
    // (every lane of the wave arrives)
    diffuse_tally(killed, &counters->killed);
    diffuse_tally(dissolved, &counters->dissolved);
}
void launch_diffuse_advect(uint32_t n, const DiffuseSetDev& set, const float* fv, const uint32_t* fc, const DiffuseParams& prm, float dt,
                           uint32_t* keep, DiffuseCounters* counters, hipStream_t st) {
    if (!n) return;
    k_diffuse_advect<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, set, fv, fc, prm, dt, keep, counters);
    SALVA_HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(BLOCK) void k_diffuse_compact(uint32_t n, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ off,
                                                           DiffuseSetDev src, DiffuseSetDev dst, DiffuseCounters* counters) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t kind = 0xffffffffu;
    if (i < n && keep[i]) {
        const uint32_t at = off[i];
        if (at < n) {  // (cannot fail: an exclusive scan of flags)
            const float4 v = src.vel[i];
            dst.pos[at] = src.pos[i];
            dst.vel[at] = v;
            dst.id[at] = src.id[i];
            kind = __float_as_uint(v.w);
        }
    }
    if (i == n - 1u) counters->kept = off[i] + keep[i];
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) diffuse_tally(kind == k, &counters->kinds[k]);
}
void launch_diffuse_compact(uint32_t n, const uint32_t* keep, const uint32_t* off, const DiffuseSetDev& src, const DiffuseSetDev& dst,
                            DiffuseCounters* counters, hipStream_t st) {
    if (!n) return;
    k_diffuse_compact<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, keep, off, src, dst, counters);
    SALVA_HIP_CHECK(hipGetLastError());
}

// the pinned mixing function and the uniform of the header
__device__ __forceinline__ uint32_t diffuse_fmix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float diffuse_uniform(uint32_t key, uint32_t draw) {  // key: fmix(fmix(fmix(fmix(seed) + updates) + slot) + index)
    return (float)(diffuse_fmix(key + draw) >> 8) * 5.9604644775390625e-8f;
}
__device__ __forceinline__ uint32_t diffuse_key(const DiffuseEmit& em, uint32_t slot, uint32_t index) {
    return diffuse_fmix(diffuse_fmix(diffuse_fmix(diffuse_fmix(em.seed) + em.updates) + slot) + index);
}
__device__ __forceinline__ float diffuse_phi(float value, float lo, float hi) { return (fminf(value, hi) - fminf(value, lo)) / (hi - lo); }
// the packed row of host row v and its fluid, or false: the row is not of a selected fluid
__device__ __forceinline__ bool diffuse_row(const RowPack& pk, uint32_t s, uint32_t v, uint32_t& r, uint32_t& index) {
    if (s >= FIELD_MAX_SLOTS || !((pk.mask >> s) & 1u) || v < pk.first[s] || v - pk.first[s] >= pk.len[s]) return false;
    index = v - pk.first[s];
    r = pk.base[s] + index;
    return true;
}

__global__ __launch_bounds__(BLOCK) void k_diffuse_rate(uint32_t n, const float4* __restrict__ st_pos, const float4* __restrict__ st_vel,
                                                        const uint32_t* __restrict__ st_model, DiffuseRows rows, DiffuseParams prm, DiffuseEmit em,
                                                        uint32_t* __restrict__ cnt) {
    const uint32_t v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= n) return;
    const uint32_t s = st_model[v];
    uint32_t r, index;
    if (!diffuse_row(em.pk, s, v, r, index) || r >= em.total) return;
    const float4 x = st_pos[v], u = st_vel[v], a = rows.a[v];  // a = (trapped air, energy, wave crest, count)
    uint32_t c = 0;
    if (isfinite(x.x) && isfinite(x.y) && isfinite(x.z) && dist2_exact(u.x, u.y, u.z) > 0.0f) {
        const float rate = (diffuse_phi(a.y, prm.en_lo, prm.en_hi) *
                            (prm.k_ta * diffuse_phi(a.x, prm.ta_lo, prm.ta_hi) + prm.k_wc * diffuse_phi(a.z, prm.wc_lo, prm.wc_hi))) * em.dt;
        const float t = rate + diffuse_uniform(diffuse_key(em, s, index), 0u);
        if (t >= 1.0f) c = (uint32_t)fminf(floorf(t), (float)prm.max_per_particle);
    }
    cnt[r] = c;
}
void launch_diffuse_rate(uint32_t n, const float4* st_pos, const float4* st_vel, const uint32_t* st_model, const DiffuseRows& rows,
                         const DiffuseParams& prm, const DiffuseEmit& em, uint32_t* cnt, hipStream_t st) {
    if (!n) return;
    k_diffuse_rate<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, st_pos, st_vel, st_model, rows, prm, em, cnt);
    SALVA_HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(BLOCK) void k_diffuse_emit(uint32_t n, const float4* __restrict__ st_pos, const float4* __restrict__ st_vel,
                                                        const uint32_t* __restrict__ st_model, DiffuseParams prm, DiffuseEmit em,
                                                        const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off, DiffuseSetDev set,
                                                        DiffuseCounters* counters) {
    const uint32_t v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= n) return;
    const uint32_t s = st_model[v];
    uint32_t r, index;
    if (!diffuse_row(em.pk, s, v, r, index) || r >= em.total) return;
    const uint32_t c = cnt[r], first = off[r], kept = min(counters->kept, em.capacity);
    const uint32_t room = em.capacity - kept;
    if (r == em.total - 1u) {  // the last row knows the total
        const uint32_t all = first + c, emitted = min(all, room);
        counters->emitted = emitted;
        counters->dropped = all - emitted;
        counters->kinds[3] = emitted;
    }
    if (!c || first >= room) return;
    const float4 x = st_pos[v], u = st_vel[v];
    const uint32_t key = diffuse_key(em, s, index);
    // the orthonormal pair normal to the direction of motion (the header's construction)
    const float sp = sqrtf(dist2_exact(u.x, u.y, u.z));
    const float wx = u.x / sp, wy = u.y / sp, wz = u.z / sp;
    const float ax = fabsf(wx), ay = fabsf(wy), az = fabsf(wz);
    const int m = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
    const float tx = m == 0 ? 1.0f : 0.0f, ty = m == 1 ? 1.0f : 0.0f, tz = m == 2 ? 1.0f : 0.0f;
    const float cx = wy * tz - wz * ty, cy = wz * tx - wx * tz, cz = wx * ty - wy * tx;
    const float cn = sqrtf(dist2_exact(cx, cy, cz));
    const float e1x = cx / cn, e1y = cy / cn, e1z = cz / cn;
    const float e2x = wy * e1z - wz * e1y, e2y = wz * e1x - wx * e1z, e2z = wx * e1y - wy * e1x;
    for (uint32_t k = 0; k < c && first + k < room; ++k) {
        const uint32_t d = 1u + 20u * k;
        float a = 0.0f, b = 0.0f;
        for (uint32_t t = 0; t < 8u; ++t) {
            const float ta = 2.0f * diffuse_uniform(key, d + 2u * t) - 1.0f, tb = 2.0f * diffuse_uniform(key, d + 2u * t + 1u) - 1.0f;
            if (ta * ta + tb * tb <= 1.0f) { a = ta; b = tb; break; }
        }
        const float cc = diffuse_uniform(key, d + 16u) * em.dt;
        const float life = prm.life_lo + diffuse_uniform(key, d + 17u) * (prm.life_hi - prm.life_lo);
        const uint32_t at = kept + first + k;  // (< capacity: first + k < room)
        set.pos[at] = make_float4((x.x + em.radius * (a * e1x + b * e2x)) + cc * u.x, (x.y + em.radius * (a * e1y + b * e2y)) + cc * u.y,
                                  (x.z + em.radius * (a * e1z + b * e2z)) + cc * u.z, life);
        set.vel[at] = make_float4(u.x, u.y, u.z, __uint_as_float((uint32_t)SALVA_HIP_DIFFUSE_NEW));
        set.id[at] = em.first_id + first + k;
    }
}
void launch_diffuse_emit(uint32_t n, const float4* st_pos, const float4* st_vel, const uint32_t* st_model, const DiffuseParams& prm,
                         const DiffuseEmit& em, const uint32_t* cnt, const uint32_t* off, const DiffuseSetDev& set, DiffuseCounters* counters,
                         hipStream_t st) {
    if (!n) return;
    k_diffuse_emit<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, st_pos, st_vel, st_model, prm, em, cnt, off, set, counters);
    SALVA_HIP_CHECK(hipGetLastError());
}

}  // namespace salva

// field.hip — SPH fields at points and on a lattice.  (a) The evaluator's own grid: the box of the finite points, the
// cell of every particle of the selected fluids inside the query's box, and their order "by cell, then by host index" gathered into
// two float4 records per particle.  (b) The sums: k_field_points, one lane per point over the 27 cells around it, and k_field_lattice,
// one workgroup per brick of 8 x 8 x 8 nodes, which stages the candidates of the brick's cell range through LDS in fixed-size chunks.
// Both visit a place's particles in ascending cell (x slowest, z fastest) and ascending host index within a cell, and both add a
// particle with the same field_term: the order of every sum is fixed.
//
// The reference's other kernels (Poly6 / Spiky / Viscosity) ride along as wave-uniform branches of kernel_eval: this file is compiled
// once, with sph_math.h's generic paths switched in.  Register pressure is no concern here (tests/test_field_resources.py).
#define SALVA_OTHER_KERNELS 1
#include "field.h"
#include "tile.h"

namespace salva {

static_assert(FIELD_MAX_SLOTS == (uint32_t)MAX_MODELS, "one rest density per fluid of a world");
static_assert(FIELD_CHUNK == FIELD_BRICK_THREADS, "a brick stages one candidate per thread and chunk");
static_assert(FIELD_BRICK_THREADS % WAVE == 0, "whole waves");

// ------------------------------------------------------------------------------------------------ (a) the evaluator's grid
__device__ __forceinline__ int32_t field_ordered_dev(float f) {
    const int32_t i = __float_as_int(f);
    return i ^ ((i >> 31) & 0x7fffffff);
}
__global__ __launch_bounds__(BLOCK) void k_field_bbox(const float* __restrict__ pts, uint64_t npoints, int32_t* __restrict__ box6) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    if (i < npoints) {
        const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        if (isfinite(x) && isfinite(y) && isfinite(z)) {
            lo[0] = hi[0] = field_ordered_dev(x); lo[1] = hi[1] = field_ordered_dev(y); lo[2] = hi[2] = field_ordered_dev(z);
        }
    }
    // (every lane of the wave arrives: the reductions are wave-wide)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int32_t l = wave_min_i32(lo[a]), h = wave_max_i32(hi[a]);
        if ((threadIdx.x & (WAVE - 1)) == 0 && l <= h) { atomicMin(&box6[a], l); atomicMax(&box6[3 + a], h); }
    }
}
void launch_field_bbox(const float* pts, uint64_t npoints, int32_t* box6, hipStream_t st) {
    if (!npoints) return;
    k_field_bbox<<<div_up(npoints, BLOCK), BLOCK, 0, st>>>(pts, npoints, box6);
    SALVA_HIP_CHECK(hipGetLastError());
}

// the linear cell of a position in g; false: outside (or not finite)
__device__ __forceinline__ bool field_cell(const FieldGrid& g, float x, float y, float z, uint32_t& ux, uint32_t& uy, uint32_t& uz) {
    bool bad = false;
    const int cx = cell_coord(x, g.h, bad), cy = cell_coord(y, g.h, bad), cz = cell_coord(z, g.h, bad);
    // (cell coordinates are clamped to +-2^30 and g.d <= 2^27: the unsigned differences wrap to something >= g.d outside)
    ux = (uint32_t)cx - (uint32_t)g.o[0]; uy = (uint32_t)cy - (uint32_t)g.o[1]; uz = (uint32_t)cz - (uint32_t)g.o[2];
    return !bad && isfinite(x) && isfinite(y) && isfinite(z) && ux < g.d[0] && uy < g.d[1] && uz < g.d[2];
}

__global__ __launch_bounds__(BLOCK) void k_field_keys(const float4* __restrict__ st_pos, const uint32_t* __restrict__ st_model, uint32_t n,
                                                      FieldFluids f, FieldGrid g, uint32_t* __restrict__ keys, uint32_t* __restrict__ rank,
                                                      uint32_t* __restrict__ cells) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 p = st_pos[i];
    const uint32_t m = st_model[i];
    uint32_t ux, uy, uz, k = FIELD_DROPPED;
    if (m < FIELD_MAX_SLOTS && ((f.mask >> m) & 1u) && field_cell(g, p.x, p.y, p.z, ux, uy, uz)) k = (ux * g.d[1] + uy) * g.d[2] + uz;
    keys[i] = k;
    if (k != FIELD_DROPPED) rank[i] = atomicAdd(&cells[k], 1u);
}
void launch_field_keys(const float4* st_pos, const uint32_t* st_model, uint32_t n, const FieldFluids& f, const FieldGrid& g, uint32_t* keys,
                       uint32_t* rank, uint32_t* cells, hipStream_t st) {
    if (!n) return;
    k_field_keys<<<div_up(n, BLOCK), BLOCK, 0, st>>>(st_pos, st_model, n, f, g, keys, rank, cells);
    SALVA_HIP_CHECK(hipGetLastError());
}

// kept row i -> position cells[key] + rank: sorted by cell, in the atomics' order within a cell
__global__ __launch_bounds__(BLOCK) void k_field_scatter(uint32_t n, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ rank,
                                                         const uint32_t* __restrict__ cells, uint32_t ncells, uint32_t* __restrict__ keys_sorted,
                                                         uint32_t* __restrict__ idx_tmp) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = keys[i];
    if (k >= ncells) return;
    const uint32_t p = cells[k] + rank[i];
    if (p >= n) return;  // (cannot happen: the table counts kept rows only)
    keys_sorted[p] = k;
    idx_tmp[p] = i;
}
// within each cell, ascending host index (grid.hip k_cell_order), and the records of the row at its final place
__global__ __launch_bounds__(BLOCK) void k_field_order(uint32_t n, const uint32_t* __restrict__ keys_sorted, const uint32_t* __restrict__ cells,
                                                       uint32_t ncells, const uint32_t* __restrict__ idx_tmp, const float4* __restrict__ st_pos,
                                                       const float4* __restrict__ st_vel, const uint32_t* __restrict__ st_model, FieldFluids f,
                                                       float4* __restrict__ rec0, float4* __restrict__ rec1, uint32_t* __restrict__ rows) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n || p >= cells[ncells]) return;  // (cells[ncells]: the kept rows)
    const uint32_t k = keys_sorted[p];
    if (k >= ncells) return;
    const uint32_t b = cells[k], e = min(cells[k + 1], n), v = idx_tmp[p];
    uint32_t below = 0;
    for (uint32_t q = b; q < e; ++q) below += idx_tmp[q] < v ? 1u : 0u;
    const uint32_t at = b + below;
    if (at >= n || v >= n) return;
    const float4 x = st_pos[v];
    // particle_mass = volumes[i] * density0 (fluid.rs:183-185), as k_stage_to_sorted (grid.hip)
    rec0[at] = make_float4(x.x, x.y, x.z, x.w * f.density0[st_model[v] & (FIELD_MAX_SLOTS - 1u)]);
    if (rec1) {
        const float4 u = st_vel[v];
        rec1[at] = make_float4(u.x, u.y, u.z, x.w);
    }
    if (rows) rows[at] = v;  // (fluidcast.h: who the sorted row is)
}
void launch_field_sort(const float4* st_pos, const float4* st_vel, const uint32_t* st_model, uint32_t n, const FieldFluids& f, const FieldGrid& g,
                       const uint32_t* keys, const uint32_t* rank, const uint32_t* cells, uint32_t* keys_sorted, uint32_t* idx_tmp, float4* rec0,
                       float4* rec1, uint32_t* rows, hipStream_t st) {
    if (!n) return;
    k_field_scatter<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, keys, rank, cells, g.ncells, keys_sorted, idx_tmp);
    k_field_order<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, keys_sorted, cells, g.ncells, idx_tmp, st_pos, st_vel, st_model, f, rec0, rec1, rows);
    SALVA_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ (b) the sums
struct FieldAcc {
    float rho = 0.0f, frac = 0.0f, px = 0.0f, py = 0.0f, pz = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
    uint32_t cnt = 0;
};
__device__ __forceinline__ uint32_t field_want(const FieldOutDev& o) {
    return (o.density ? FIELD_WANT_DENSITY : 0u) | (o.fraction ? FIELD_WANT_FRACTION : 0u) | (o.velocity ? FIELD_WANT_VELOCITY : 0u) |
           (o.gradient ? FIELD_WANT_GRADIENT : 0u) | (o.count ? FIELD_WANT_COUNT : 0u);
}
// One candidate (r0 = (x_j, m_j), r1 = (v_j, V_j)) seen from x: d = x - x_j, in support iff dist2_exact(d) <= h^2, the contact search's
// test with its rounding.  `want` is uniform over the wave.  A NaN in x fails the test: such a lane never adds anything.
__device__ __forceinline__ void field_term(FieldAcc& a, uint32_t want, float x, float y, float z, const float4& r0, const float4& r1,
                                           const SphConsts& c) {
    const float dx = x - r0.x, dy = y - r0.y, dz = z - r0.z;
    const float r2 = dist2_exact(dx, dy, dz);
    if (!(r2 <= c.h2)) return;
    const KernelEval e = kernel_eval(r2, c);
    const float mw = r0.w * e.w;
    a.rho += mw;
    a.cnt += 1u;
    if (want & FIELD_WANT_FRACTION) a.frac += r1.w * e.w;
    if (want & FIELD_WANT_VELOCITY) { a.px += mw * r1.x; a.py += mw * r1.y; a.pz += mw * r1.z; }
    if (want & FIELD_WANT_GRADIENT) {
        const float mg = r0.w * e.g;
        a.gx += mg * dx; a.gy += mg * dy; a.gz += mg * dz;
    }
}
__device__ __forceinline__ void field_store(const FieldOutDev& o, uint64_t i, const FieldAcc& a) {
    if (o.density) o.density[i] = a.rho;
    if (o.fraction) o.fraction[i] = a.frac;
    if (o.velocity) {
        const bool nz = a.rho != 0.0f;
        o.velocity[3 * i] = nz ? a.px / a.rho : 0.0f;
        o.velocity[3 * i + 1] = nz ? a.py / a.rho : 0.0f;
        o.velocity[3 * i + 2] = nz ? a.pz / a.rho : 0.0f;
    }
    if (o.gradient) { o.gradient[3 * i] = a.gx; o.gradient[3 * i + 1] = a.gy; o.gradient[3 * i + 2] = a.gz; }
    if (o.count) o.count[i] = a.cnt;
}
// origin + (float)i * spacing: the product and the sum each rounded in f32 (the file is built without contraction, and the product is
// made opaque for good measure).  Never call this from a SALVA_PAIR_MATH scope.
__device__ __forceinline__ float field_node(float origin, float spacing, uint32_t i) { return origin + opaque((float)i * spacing); }

// One lane per point; the 27 cells around it as nine runs along z, in ascending cell order.
__global__ __launch_bounds__(BLOCK) void k_field_points(FieldQuery q, FieldGrid g, FieldCandidates cand, SphConsts c, FieldOutDev out) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= q.npoints) return;
    const uint32_t want = field_want(out);
    const bool second = (want & (FIELD_WANT_FRACTION | FIELD_WANT_VELOCITY)) != 0u && cand.rec1;
    float x, y, z;
    if (q.pts) {
        x = q.pts[3 * i]; y = q.pts[3 * i + 1]; z = q.pts[3 * i + 2];
    } else {
        const uint64_t nz = q.dims[2], ny = q.dims[1];
        const uint32_t iz = (uint32_t)(i % nz), iy = (uint32_t)((i / nz) % ny), ix = (uint32_t)(i / (nz * ny));
        x = field_node(q.origin[0], q.spacing, ix); y = field_node(q.origin[1], q.spacing, iy); z = field_node(q.origin[2], q.spacing, iz);
    }
    FieldAcc a;
    uint32_t ux, uy, uz;
    if (field_cell(g, x, y, z, ux, uy, uz)) {
        const uint32_t x0 = ux ? ux - 1u : 0u, x1 = min(ux + 1u, g.d[0] - 1u), y0 = uy ? uy - 1u : 0u, y1 = min(uy + 1u, g.d[1] - 1u),
                       z0 = uz ? uz - 1u : 0u, z1 = min(uz + 1u, g.d[2] - 1u);
        for (uint32_t cx = x0; cx <= x1; ++cx)
            for (uint32_t cy = y0; cy <= y1; ++cy) {
                const uint32_t row = (cx * g.d[1] + cy) * g.d[2];
                const uint32_t b = cand.cells[row + z0], e = cand.cells[row + z1 + 1u];
                for (uint32_t p = b; p < e; ++p) {
                    const float4 r0 = cand.rec0[p];
                    const float4 r1 = second ? cand.rec1[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    field_term(a, want, x, y, z, r0, r1, c);
                }
            }
    }
    field_store(out, i, a);
}
void launch_field_points(const FieldQuery& q, const FieldGrid& g, const FieldCandidates& cand, const SphConsts& c, const FieldOutDev& out,
                         hipStream_t st) {
    if (!q.npoints) return;
    k_field_points<<<div_up(q.npoints, BLOCK), BLOCK, 0, st>>>(q, g, cand, c, out);
    SALVA_HIP_CHECK(hipGetLastError());
}

// One workgroup per brick of 8 x 8 x 8 nodes, one lane per node.  The brick's nodes name a cell range (the cells of its first and last
// node per axis, grown by one); its candidates are the runs along z of that range, (x, y) ascending.  Groups of up to one run per
// thread are scanned by length, and the concatenation of a group's runs is staged FIELD_CHUNK candidates at a time: thread t finds the
// run of candidate base + t by bisection over the scan.  Every lane then walks the chunk — all lanes read the same LDS address, a
// broadcast — with the exact test.  A crowded cell or a coarse lattice only means more chunks; a brick without candidates stages nothing.
__global__ __launch_bounds__(FIELD_BRICK_THREADS) void k_field_lattice(FieldQuery q, FieldGrid g, FieldCandidates cand, SphConsts c, FieldOutDev out) {
    __shared__ float4 s_r0[FIELD_CHUNK];
    __shared__ float4 s_r1[FIELD_CHUNK];
    __shared__ uint32_t s_end[FIELD_BRICK_THREADS];    // inclusive scan of the group's run lengths
    __shared__ uint32_t s_start[FIELD_BRICK_THREADS];  // first row of each run
    __shared__ uint32_t s_wave[FIELD_BRICK_THREADS / WAVE];
    const uint32_t t = threadIdx.x, lane = t & (WAVE - 1), wid = t / WAVE;
    const uint32_t want = field_want(out);
    const bool second = (want & (FIELD_WANT_FRACTION | FIELD_WANT_VELOCITY)) != 0u && cand.rec1;
    const uint32_t nb[3] = {(q.dims[0] + FIELD_BRICK - 1u) / FIELD_BRICK, (q.dims[1] + FIELD_BRICK - 1u) / FIELD_BRICK,
                            (q.dims[2] + FIELD_BRICK - 1u) / FIELD_BRICK};
    const uint32_t bz = blockIdx.x % nb[2], by = (blockIdx.x / nb[2]) % nb[1], bx = blockIdx.x / (nb[2] * nb[1]);
    const uint32_t first[3] = {bx * FIELD_BRICK, by * FIELD_BRICK, bz * FIELD_BRICK};
    const uint32_t ix = first[0] + (t >> 6), iy = first[1] + ((t >> 3) & 7u), iz = first[2] + (t & 7u);
    const bool node = bx < nb[0] && ix < q.dims[0] && iy < q.dims[1] && iz < q.dims[2];
    const float nan = __builtin_nanf("");
    // (a lane without a node, or with a node that is not finite, carries NaN: it adds nothing and its node gets zeros)
    float x = field_node(q.origin[0], q.spacing, ix), y = field_node(q.origin[1], q.spacing, iy), z = field_node(q.origin[2], q.spacing, iz);
    if (!(node && isfinite(x) && isfinite(y) && isfinite(z))) x = y = z = nan;
    // the brick's cell range (uniform over the workgroup)
    long long lo[3], hi[3];
    bool empty = bx >= nb[0];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const uint32_t last = min(first[a] + FIELD_BRICK - 1u, q.dims[a] - 1u);
        bool bad = false;
        const int c0 = cell_coord(field_node(q.origin[a], q.spacing, first[a]), g.h, bad);
        const int c1 = cell_coord(field_node(q.origin[a], q.spacing, last), g.h, bad);
        lo[a] = (long long)c0 - (long long)g.o[a] - 1;
        hi[a] = (long long)c1 - (long long)g.o[a] + 1;
        if (lo[a] < 0) lo[a] = 0;
        if (hi[a] > (long long)g.d[a] - 1) hi[a] = (long long)g.d[a] - 1;
        empty = empty || bad || lo[a] > hi[a];
    }
    FieldAcc acc;
    if (!empty) {
        const uint32_t nyr = (uint32_t)(hi[1] - lo[1] + 1);
        const uint64_t nruns = (uint64_t)(hi[0] - lo[0] + 1) * nyr;
        for (uint64_t r0 = 0; r0 < nruns; r0 += FIELD_BRICK_THREADS) {  // (uniform)
            const uint64_t r = r0 + t;
            uint32_t start = 0, len = 0;
            if (r < nruns) {
                const uint32_t cx = (uint32_t)lo[0] + (uint32_t)(r / nyr), cy = (uint32_t)lo[1] + (uint32_t)(r % nyr);
                const uint32_t row = (cx * g.d[1] + cy) * g.d[2];
                start = cand.cells[row + (uint32_t)lo[2]];
                const uint32_t end = cand.cells[row + (uint32_t)hi[2] + 1u];
                len = end > start ? end - start : 0u;
            }
            // inclusive scan of len over the workgroup
            uint32_t inc = len;
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1) {
                const uint32_t o = __shfl_up(inc, d);
                if (lane >= (uint32_t)d) inc += o;
            }
            if (lane == WAVE - 1) s_wave[wid] = inc;
            __syncthreads();
            uint32_t base_w = 0;
#pragma unroll
            for (uint32_t k = 0; k < FIELD_BRICK_THREADS / WAVE; ++k)
                if (k < wid) base_w += s_wave[k];
            s_end[t] = base_w + inc;
            s_start[t] = start;
            __syncthreads();
            const uint32_t total = s_end[FIELD_BRICK_THREADS - 1u];
            for (uint32_t base = 0; base < total; base += FIELD_CHUNK) {  // (uniform)
                const uint32_t v = base + t;
                if (v < total) {
                    uint32_t a = 0, b = FIELD_BRICK_THREADS - 1u;  // the first run whose inclusive end exceeds v
                    while (a < b) {
                        const uint32_t mid = (a + b) >> 1;
                        if (s_end[mid] > v) b = mid; else a = mid + 1u;
                    }
                    const uint32_t before = a ? s_end[a - 1u] : 0u;
                    const uint32_t src = s_start[a] + (v - before);
                    s_r0[t] = cand.rec0[src];
                    if (second) s_r1[t] = cand.rec1[src];
                }
                __syncthreads();
                const uint32_t cnt = min(FIELD_CHUNK, total - base);
                for (uint32_t j = 0; j < cnt; ++j) {
                    const float4 p0 = lds_f4(&s_r0[j]);
                    const float4 p1 = second ? lds_f4(&s_r1[j]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    field_term(acc, want, x, y, z, p0, p1, c);
                }
                __syncthreads();
            }
        }
    }
    if (node) field_store(out, ((uint64_t)ix * q.dims[1] + iy) * q.dims[2] + iz, acc);
}
void launch_field_lattice(const FieldQuery& q, const FieldGrid& g, const FieldCandidates& cand, const SphConsts& c, const FieldOutDev& out,
                          hipStream_t st) {
    const uint64_t bricks = (uint64_t)div_up(q.dims[0], FIELD_BRICK) * div_up(q.dims[1], FIELD_BRICK) * div_up(q.dims[2], FIELD_BRICK);
    if (!bricks) return;
    if (bricks > 0x7fffffffull) throw HipError(SALVA_HIP_E_CAPACITY, "field lattice: more bricks than one launch takes; split the query");
    k_field_lattice<<<(unsigned)bricks, FIELD_BRICK_THREADS, 0, st>>>(q, g, cand, c, out);
    SALVA_HIP_CHECK(hipGetLastError());
}

}  // namespace salva

// sink.hip — deleting particles by region on the device.  (a) The region predicates: one kernel per kind family
// (half-space / box, built-in shape, mesh, compound), one thread per row, one keep flag per row; the distances are the queries'
// (solid_distance.h).  (b) One stable stream compaction of up to four float4 arrays from a single scan of the flags: counts per
// workgroup (wave64 ballots and population counts), a two-level exclusive scan of the counts, and a scatter that recomputes its ranks
// from the same ballots.  Every launch depends only on the completed launch before it: no workgroup waits for another.
#include "sink.h"
#include "solid_distance.h"

namespace salva {

static_assert(SINK_ROWS == (uint32_t)BLOCK, "one row per thread");
static_assert(SINK_SCAN_SPAN == 4u * (uint32_t)BLOCK, "a scan workgroup takes four counts per thread");

// ------------------------------------------------------------------------------------------------ wave / workgroup helpers
__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {  // set bits of m below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// exclusive scan of one value per thread over the workgroup; *total: the sum, in every thread.  lds: BLOCK / WAVE words.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
    const uint32_t lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= (uint32_t)d) inc += o;
    }
    if (lane == WAVE - 1) lds[wid] = inc;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)(BLOCK / WAVE); ++k) {
        const uint32_t w = lds[k];
        if (k < wid) base += w;
        sum += w;
    }
    __syncthreads();
    *total = sum;
    return base + inc - v;
}

// ------------------------------------------------------------------------------------------------ (a) predicates
// What every predicate ends with.  All lanes of the wave arrive (rows beyond n with in_range = false): the tally is wave-wide.
// A particle matches when its position is finite and d <= margin; the region selects matches, or with INVERT everything else.
__device__ __forceinline__ void sink_decide(const SinkSrc& s, const SinkRegionDev& r, uint32_t i, bool in_range, bool finite, float d,
                                            uint8_t* __restrict__ keep, uint32_t* __restrict__ deleted) {
    const uint32_t m = in_range ? s.model[i] : 0u;
    const bool scope = in_range && (s.slot == SALVA_HIP_ALL_FLUIDS || m == s.slot);
    const bool match = finite && d <= r.margin;
    const bool gone = s.accumulate != 0u && in_range && keep[i] == 0;  // an earlier region of this edit took the row
    const bool del = scope && !gone && (match != (r.invert != 0u));
    if (in_range && !gone) keep[i] = del ? 0 : 1;
    if (!deleted) return;
    // one atomic per fluid present among the wave's selected rows
    unsigned long long left = __ballot(del);
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    while (left) {
        const int first = __ffsll((long long)left) - 1;
        const uint32_t mm = (uint32_t)__shfl((int)m, first);
        const unsigned long long same = __ballot(del && m == mm);
        if (lane == (uint32_t)first && mm < SINK_MAX_SLOTS) atomicAdd(&deleted[mm], (uint32_t)__popcll(same));
        left &= ~same;
    }
}
__device__ __forceinline__ bool sink_load(const SinkSrc& s, uint32_t i, float4& p, bool& finite) {
    const bool in_range = i < s.n;
    p = in_range ? s.pos[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    finite = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    return in_range;
}
__device__ __forceinline__ void sink_local(const SinkRegionDev& r, const float4& p, float& lx, float& ly, float& lz) {
    quat_rot(-r.q[0], -r.q[1], -r.q[2], r.q[3], p.x - r.t[0], p.y - r.t[1], p.z - r.t[2], lx, ly, lz);
}

// half-space: n . (x - p); box: the distance k_aabb_query squares (world_query.hip)
__global__ __launch_bounds__(BLOCK) void k_sink_plane_box(SinkSrc s, SinkRegionDev r, uint8_t* __restrict__ keep, uint32_t* __restrict__ deleted) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    float4 p;
    bool finite;
    const bool in_range = sink_load(s, i, p, finite);
    float d;
    if (r.kind == SALVA_HIP_REGION_HALFSPACE) {
        d = (r.b[0] * (p.x - r.a[0]) + r.b[1] * (p.y - r.a[1])) + r.b[2] * (p.z - r.a[2]);
    } else {
        const float dx = fmaxf(fmaxf(r.a[0] - p.x, p.x - r.b[0]), 0.0f), dy = fmaxf(fmaxf(r.a[1] - p.y, p.y - r.b[1]), 0.0f),
                    dz = fmaxf(fmaxf(r.a[2] - p.z, p.z - r.b[2]), 0.0f);
        d = sqrtf(dx * dx + dy * dy + dz * dz);
    }
    sink_decide(s, r, i, in_range, finite, d, keep, deleted);
}
__global__ __launch_bounds__(BLOCK) void k_sink_shape(SinkSrc s, SinkRegionDev r, uint8_t* __restrict__ keep, uint32_t* __restrict__ deleted) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    float4 p;
    bool finite;
    const bool in_range = sink_load(s, i, p, finite);
    float lx, ly, lz;
    sink_local(r, p, lx, ly, lz);
    sink_decide(s, r, i, in_range, finite, shape_solid_distance(r.shape_kind, r.p, lx, ly, lz), keep, deleted);
}
// (a row out of range, of another fluid or not finite does not walk the hierarchy: its distance is not looked at)
__global__ __launch_bounds__(BLOCK) void k_sink_mesh(SinkSrc s, SinkRegionDev r, MeshDev mesh, uint8_t* __restrict__ keep, uint32_t* __restrict__ deleted) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    float4 p;
    bool finite;
    const bool in_range = sink_load(s, i, p, finite);
    float d = __builtin_inff();
    if (in_range && finite && (s.slot == SALVA_HIP_ALL_FLUIDS || s.model[i] == s.slot)) {
        float lx, ly, lz;
        sink_local(r, p, lx, ly, lz);
        d = mesh_solid_distance(mesh, lx, ly, lz);
    }
    sink_decide(s, r, i, in_range, finite, d, keep, deleted);
}
__global__ __launch_bounds__(BLOCK) void k_sink_compound(SinkSrc s, SinkRegionDev r, const CompoundPartDev* __restrict__ parts, uint32_t nparts,
                                                         uint8_t* __restrict__ keep, uint32_t* __restrict__ deleted) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    float4 p;
    bool finite;
    const bool in_range = sink_load(s, i, p, finite);
    float d = __builtin_inff();
    if (in_range && finite && (s.slot == SALVA_HIP_ALL_FLUIDS || s.model[i] == s.slot)) {
        float lx, ly, lz;
        sink_local(r, p, lx, ly, lz);
        d = compound_solid_distance(parts, nparts, lx, ly, lz);
    }
    sink_decide(s, r, i, in_range, finite, d, keep, deleted);
}

void launch_sink_predicate(const SinkSrc& src, const SinkRegionDev& r, const MeshDev* mesh, const CompoundPartDev* parts, uint32_t nparts,
                           uint8_t* keep, uint32_t* deleted, hipStream_t st) {
    if (!src.n) return;
    const unsigned nb = div_up(src.n, BLOCK);
    if (r.kind == SALVA_HIP_REGION_HALFSPACE || r.kind == SALVA_HIP_REGION_AABB) k_sink_plane_box<<<nb, BLOCK, 0, st>>>(src, r, keep, deleted);
    else if (r.kind == SALVA_HIP_REGION_SHAPE) k_sink_shape<<<nb, BLOCK, 0, st>>>(src, r, keep, deleted);
    else if (r.kind == SALVA_HIP_REGION_MESH && mesh) k_sink_mesh<<<nb, BLOCK, 0, st>>>(src, r, *mesh, keep, deleted);
    else if (r.kind == SALVA_HIP_REGION_COMPOUND && parts) k_sink_compound<<<nb, BLOCK, 0, st>>>(src, r, parts, nparts, keep, deleted);
    else throw HipError(SALVA_HIP_E_INVALID, "internal error: a region without a predicate kernel");
    SALVA_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ (b) compaction
__device__ __forceinline__ bool sink_kept(const uint8_t* __restrict__ keep, uint32_t nflag, uint32_t n, uint32_t i) {
    return i < n && (i >= nflag || keep[i] != 0);
}
// counts[b] = kept rows of workgroup b
__global__ __launch_bounds__(BLOCK) void k_sink_block_counts(const uint8_t* __restrict__ keep, uint32_t nflag, uint32_t n, uint32_t* __restrict__ counts) {
    __shared__ uint32_t lds[BLOCK / WAVE];
    const uint32_t i = blockIdx.x * SINK_ROWS + threadIdx.x;
    const unsigned long long m = __ballot(sink_kept(keep, nflag, n, i));
    if ((threadIdx.x & (WAVE - 1)) == 0) lds[threadIdx.x / WAVE] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < BLOCK / WAVE; ++k) c += lds[k];
        counts[blockIdx.x] = c;
    }
}
// counts[b * SPAN ..] -> their exclusive scan inside the span, in place; totals[b] = the span's sum
__global__ __launch_bounds__(BLOCK) void k_sink_scan_counts(uint32_t* __restrict__ counts, uint32_t nblocks, uint32_t* __restrict__ totals) {
    __shared__ uint32_t lds[BLOCK / WAVE];
    const uint32_t base = blockIdx.x * SINK_SCAN_SPAN + threadIdx.x * 4u;
    uint32_t c[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) c[k] = base + k < nblocks ? counts[base + k] : 0u;
    uint32_t total;
    uint32_t run = block_exclusive_scan((c[0] + c[1]) + (c[2] + c[3]), lds, &total);
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        if (base + k < nblocks) counts[base + k] = run;
        run += c[k];
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}
// one workgroup: totals -> their exclusive scan in place, BLOCK at a time with a running carry; *kept = the sum
__global__ __launch_bounds__(BLOCK) void k_sink_scan_totals(uint32_t* __restrict__ totals, uint32_t nscan, uint32_t* __restrict__ kept) {
    __shared__ uint32_t lds[BLOCK / WAVE];
    uint32_t carry = 0;
    for (uint32_t at = 0; at < nscan; at += BLOCK) {  // (uniform over the workgroup)
        const uint32_t k = at + threadIdx.x;
        const uint32_t v = k < nscan ? totals[k] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(v, lds, &total);
        if (k < nscan) totals[k] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *kept = carry;
}
struct SinkArrays { const float4* src[4]; float4* dst[4]; int narr; uint32_t cap; };
__global__ __launch_bounds__(BLOCK) void k_sink_scatter(const uint8_t* __restrict__ keep, uint32_t nflag, uint32_t n, const uint32_t* __restrict__ counts,
                                                        const uint32_t* __restrict__ totals, SinkArrays a) {
    __shared__ uint32_t lds[BLOCK / WAVE];
    const uint32_t i = blockIdx.x * SINK_ROWS + threadIdx.x, wid = threadIdx.x / WAVE;
    const bool k = sink_kept(keep, nflag, n, i);
    const unsigned long long m = __ballot(k);
    if ((threadIdx.x & (WAVE - 1)) == 0) lds[wid] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!k) return;
    uint32_t at = counts[blockIdx.x] + totals[blockIdx.x / SINK_SCAN_SPAN] + lanes_below(m);
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)(BLOCK / WAVE); ++w)
        if (w < wid) at += lds[w];
    if (at >= a.cap) return;  // (at <= i: a kept row never moves up; dst is cut for the kept rows the caller counted)
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (q < a.narr) a.dst[q][at] = a.src[q][i];
}

size_t sink_scan_words(uint32_t n) {
    const size_t nblocks = div_up(n ? n : 1, SINK_ROWS), nscan = div_up(nblocks, SINK_SCAN_SPAN);
    return nblocks + nscan + 1;
}
void launch_sink_compact(const uint8_t* keep, uint32_t nflag, uint32_t n, uint32_t* scratch, const float4* const src[4], float4* const dst[4],
                         int narr, uint32_t cap, hipStream_t st) {
    if (narr < 1 || narr > 4) throw HipError(SALVA_HIP_E_INVALID, "internal error: a compaction moves one to four arrays");
    const uint32_t nblocks = div_up(n ? n : 1, SINK_ROWS), nscan = div_up(nblocks, SINK_SCAN_SPAN);
    uint32_t* counts = scratch;
    uint32_t* totals = scratch + nblocks;
    uint32_t* kept = totals + nscan;
    SinkArrays a{};
    a.narr = narr; a.cap = cap;
    for (int q = 0; q < narr; ++q) { a.src[q] = src[q]; a.dst[q] = dst[q]; }
    k_sink_block_counts<<<nblocks, BLOCK, 0, st>>>(keep, nflag, n, counts);
    k_sink_scan_counts<<<nscan, BLOCK, 0, st>>>(counts, nblocks, totals);
    k_sink_scan_totals<<<1, BLOCK, 0, st>>>(totals, nscan, kept);
    k_sink_scatter<<<nblocks, BLOCK, 0, st>>>(keep, nflag, n, counts, totals, a);
    SALVA_HIP_CHECK(hipGetLastError());
}

}  // namespace salva

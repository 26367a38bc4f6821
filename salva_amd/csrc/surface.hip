// surface.hip — the iso-surface of a lattice of values as an indexed triangle mesh (the contract is in
// include/salva_hip.h).  Marching tetrahedra on the Freudenthal split of every cell, in three streaming passes over the nodes, one
// lane per node, z fastest:
//   k_surface_classify   one word per node: which of its seven edges carry a vertex, how many, and the triangles of its cell
//   (totals, two scans)  the exact 64-bit totals of the two counts, then their exclusive scans: where a node's vertices and a cell's
//                        triangles start
//   k_surface_emit       the vertices of the node's edges and the triangles of its cell, at those places
// A triangle names a vertex by the node that owns its edge and the edge's bit: scan[owner] + popcount(mask[owner] & (bit - 1)).  No
// atomics and no hashing anywhere: the output order is a pure function of the node values.  k_surface_normals turns the evaluator's
// gradient at the vertices into unit normals; k_surface_bounds is k_field_bbox over the particles of the selected fluids.
// Built like every file with -ffp-contract=off: every f32 operation of a vertex rounds once; `/` is the correctly rounded division.
#include "surface.h"
#include "sph_math.h"

#include <hipcub/hipcub.hpp>

namespace salva {

// ------------------------------------------------------------------------------------------------ the 6 x 16 cases
// Corner k = 4 ox + 2 oy + oz of a cell.  Tetrahedron t follows the permutation (a, b, c) of the axes, in lexicographic order:
// v0 = 0, v1 = v0 + e_a, v2 = v1 + e_b, v3 = 7.  An edge (v_i, v_j), i < j, is owned by v_i; its bit is (v_j - v_i) - 1.
struct alignas(8) SurfaceCase {
    uint8_t n;     // triangles: 0, 1 or 2
    uint8_t e[6];  // their corners: (owner corner k) << 3 | edge bit
    uint8_t pad;
};
struct SurfaceCases {
    SurfaceCase c[6][16];  // [tetrahedron][bit i: v_i is inside]
    uint8_t corner[6][4];
};
constexpr SurfaceCases make_surface_cases() {
    constexpr int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    SurfaceCases T{};
    for (int t = 0; t < 6; ++t) {
        int v[4] = {0, 0, 0, 7};
        v[1] = 4 >> perm[t][0];
        v[2] = v[1] | (4 >> perm[t][1]);
        for (int i = 0; i < 4; ++i) T.corner[t][i] = (uint8_t)v[i];
        for (int m = 1; m < 15; ++m) {
            int in[4] = {}, out[4] = {}, ni = 0, no = 0;
            for (int i = 0; i < 4; ++i) {
                if ((m >> i) & 1) in[ni++] = i; else out[no++] = i;
            }
            int tri[2][3][2] = {};  // triangles of tetrahedron edges (i, j)
            int ntri = 0;
            if (ni == 1 || no == 1) {  // one corner apart: (ab, ac, ad), b < c < d
                const int a = ni == 1 ? in[0] : out[0];
                const int* o = ni == 1 ? out : in;
                for (int k = 0; k < 3; ++k) { tri[0][k][0] = a; tri[0][k][1] = o[k]; }
                ntri = 1;
            } else {  // inside a < b, outside c < d: the quad (ac, ad, bd, bc) as (q0, q1, q2), (q0, q2, q3)
                const int q[4][2] = {{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}, {in[1], out[0]}};
                const int pick[2][3] = {{0, 1, 2}, {0, 2, 3}};
                for (int k = 0; k < 2; ++k)
                    for (int c = 0; c < 3; ++c) { tri[k][c][0] = q[pick[k][c]][0]; tri[k][c][1] = q[pick[k][c]][1]; }
                ntri = 2;
            }
            // from the inside corners' centroid to the outside corners' centroid, times ni * no
            int towards[3] = {};
            for (int a = 0; a < 3; ++a) {
                for (int k = 0; k < no; ++k) towards[a] += ni * ((v[out[k]] >> (2 - a)) & 1);
                for (int k = 0; k < ni; ++k) towards[a] -= no * ((v[in[k]] >> (2 - a)) & 1);
            }
            T.c[t][m].n = (uint8_t)ntri;
            for (int k = 0; k < ntri; ++k) {
                // the edge midpoints of the unit tetrahedron, times 2, stand in for the vertices
                int p[3][3] = {};
                for (int c = 0; c < 3; ++c)
                    for (int a = 0; a < 3; ++a) p[c][a] = ((v[tri[k][c][0]] >> (2 - a)) & 1) + ((v[tri[k][c][1]] >> (2 - a)) & 1);
                const int u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
                const int w[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
                const int s = (u[1] * w[2] - u[2] * w[1]) * towards[0] + (u[2] * w[0] - u[0] * w[2]) * towards[1] +
                              (u[0] * w[1] - u[1] * w[0]) * towards[2];
                const int order[3] = {0, s > 0 ? 1 : 2, s > 0 ? 2 : 1};  // the right-hand normal points to the outside corners
                for (int c = 0; c < 3; ++c) {
                    const int i = tri[k][order[c]][0], j = tri[k][order[c]][1];
                    const int lo = i < j ? i : j, hi = i < j ? j : i;
                    T.c[t][m].e[3 * k + c] = (uint8_t)((v[lo] << 3) | ((v[hi] - v[lo]) - 1));
                }
            }
        }
    }
    return T;
}
constexpr SurfaceCases SURFACE_CASES_HOST = make_surface_cases();
__constant__ SurfaceCases SURFACE_CASES = make_surface_cases();

// v1 and v2 of tetrahedron t, a nibble each (v0 = 0 and v3 = 7 always): immediates after unrolling
constexpr uint32_t SURFACE_V1 = 0x112244u, SURFACE_V2 = 0x353656u;
constexpr bool surface_cases_sound() {
    int cases = 0, triangles = 0;
    for (int t = 0; t < 6; ++t) {
        if (SURFACE_CASES_HOST.corner[t][0] != 0 || SURFACE_CASES_HOST.corner[t][3] != 7) return false;
        if (SURFACE_CASES_HOST.corner[t][1] != ((SURFACE_V1 >> (4 * t)) & 15u) || SURFACE_CASES_HOST.corner[t][2] != ((SURFACE_V2 >> (4 * t)) & 15u)) return false;
        for (int m = 0; m < 16; ++m) {
            const SurfaceCase& c = SURFACE_CASES_HOST.c[t][m];
            cases += c.n ? 1 : 0;
            triangles += c.n;
            for (int k = 0; k < 3 * c.n; ++k)
                if ((c.e[k] & 7) > 6 || ((c.e[k] >> 3) & ((c.e[k] & 7) + 1)) != 0) return false;  // owner + offset stays a corner
        }
    }
    return cases == 84 && triangles == 6 * (8 + 2 * 6);
}
static_assert(surface_cases_sound(), "6 x 14 non-trivial cases, 120 triangles, every edge inside its cell");
static_assert(sizeof(SurfaceCase) == 8, "one 64-bit load per case");

// ------------------------------------------------------------------------------------------------ classify
struct SurfaceNode {
    uint32_t ix, iy, iz;
    uint32_t sx, sy;  // index strides of x and y (z: 1)
};
__device__ __forceinline__ SurfaceNode surface_node(const SurfaceLattice& g, uint32_t i) {
    const uint32_t nz = g.dims[2], ny = g.dims[1];
    const uint32_t q = i / nz;
    return SurfaceNode{q / ny, q % ny, i % nz, ny * nz, nz};
}
// bit k: corner k (4 ox + 2 oy + oz) of node i's cell is in the lattice; bit 8 + k: it is inside (f >= iso)
__device__ __forceinline__ uint32_t surface_corners(const float* __restrict__ values, float iso, const SurfaceLattice& g, uint32_t i, const SurfaceNode& p,
                                                    float f0) {
    const bool hx = p.ix + 1u < g.dims[0], hy = p.iy + 1u < g.dims[1], hz = p.iz + 1u < g.dims[2];
    uint32_t bits = 1u | (f0 >= iso ? 0x100u : 0u);
#pragma unroll
    for (uint32_t k = 1; k < 8; ++k) {
        const bool ox = (k & 4u) != 0u, oy = (k & 2u) != 0u, oz = (k & 1u) != 0u;
        if ((!ox || hx) && (!oy || hy) && (!oz || hz)) {
            const float f = values[i + (ox ? p.sx : 0u) + (oy ? p.sy : 0u) + (oz ? 1u : 0u)];
            bits |= (1u << k) | (f >= iso ? 0x100u << k : 0u);
        }
    }
    return bits;
}
// bit i: corner v_i of tetrahedron t is inside
__device__ __forceinline__ uint32_t surface_tet_mask(uint32_t inside, uint32_t t) {
    const uint32_t v1 = (SURFACE_V1 >> (4u * t)) & 15u, v2 = (SURFACE_V2 >> (4u * t)) & 15u;
    return (inside & 1u) | (((inside >> v1) & 1u) << 1) | (((inside >> v2) & 1u) << 2) | (((inside >> 7) & 1u) << 3);
}

__global__ __launch_bounds__(BLOCK) void k_surface_classify(const float* __restrict__ values, float iso, SurfaceLattice g, uint32_t* __restrict__ word,
                                                            SurfaceTotals* __restrict__ totals) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= g.n) {
        if (i == g.n) word[i] = 0u;
        return;
    }
    const SurfaceNode p = surface_node(g, i);
    const float f0 = values[i];
    if (!isfinite(f0)) totals->nonfinite = 1u;  // (every lane that stores, stores the same word)
    const uint32_t bits = surface_corners(values, iso, g, i, p, f0);
    const uint32_t have = bits & 0xffu, inside = bits >> 8;
    // the edges to the corners that are there and on the other side of iso than the node itself
    const uint32_t mask = (((inside & 1u) ? ~inside : inside) & have & 0xfeu) >> 1;
    uint32_t nt = 0;
    if (have == 0xffu) {
#pragma unroll
        for (uint32_t t = 0; t < 6; ++t) {
            const uint32_t pc = __popc(surface_tet_mask(inside, t));
            nt += pc == 2u ? 2u : (pc == 0u || pc == 4u ? 0u : 1u);
        }
    }
    word[i] = mask | ((uint32_t)__popc(mask) << SURFACE_VCOUNT_SHIFT) | (nt << SURFACE_TCOUNT_SHIFT);
}
void launch_surface_classify(const float* values, float iso, const SurfaceLattice& g, uint32_t* word, SurfaceTotals* totals, hipStream_t st) {
    k_surface_classify<<<div_up((size_t)g.n + 1, BLOCK), BLOCK, 0, st>>>(values, iso, g, word, totals);
    SALVA_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ totals and scans
struct SurfacePair {
    unsigned long long v, t;
};
struct SurfacePairSum {
    __host__ __device__ SurfacePair operator()(const SurfacePair& a, const SurfacePair& b) const { return SurfacePair{a.v + b.v, a.t + b.t}; }
};
struct SurfacePairOf {
    __host__ __device__ SurfacePair operator()(uint32_t w) const { return SurfacePair{(w >> SURFACE_VCOUNT_SHIFT) & 7u, (w >> SURFACE_TCOUNT_SHIFT) & 15u}; }
};
struct SurfaceVCount {
    __host__ __device__ uint32_t operator()(uint32_t w) const { return (w >> SURFACE_VCOUNT_SHIFT) & 7u; }
};
struct SurfaceTCount {
    __host__ __device__ uint32_t operator()(uint32_t w) const { return (w >> SURFACE_TCOUNT_SHIFT) & 15u; }
};
using SurfacePairIt = hipcub::TransformInputIterator<SurfacePair, SurfacePairOf, const uint32_t*>;
using SurfaceVIt = hipcub::TransformInputIterator<uint32_t, SurfaceVCount, const uint32_t*>;
using SurfaceTIt = hipcub::TransformInputIterator<uint32_t, SurfaceTCount, const uint32_t*>;
static_assert(offsetof(SurfaceTotals, nv) == 0 && offsetof(SurfaceTotals, nt) == 8, "a SurfacePair leads a SurfaceTotals");

size_t surface_temp_bytes(uint32_t n) {
    size_t a = 0, b = 0, c = 0;
    (void)hipcub::DeviceReduce::Reduce(nullptr, a, SurfacePairIt(nullptr, SurfacePairOf{}), (SurfacePair*)nullptr, (int)n, SurfacePairSum{}, SurfacePair{0, 0});
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, SurfaceVIt(nullptr, SurfaceVCount{}), (uint32_t*)nullptr, (int)(n + 1u));
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, c, SurfaceTIt(nullptr, SurfaceTCount{}), (uint32_t*)nullptr, (int)(n + 1u));
    return std::max(a, std::max(b, c));
}
void launch_surface_totals(void* temp, size_t temp_bytes, const uint32_t* word, uint32_t n, SurfaceTotals* totals, hipStream_t st) {
    SALVA_HIP_CHECK(hipcub::DeviceReduce::Reduce(temp, temp_bytes, SurfacePairIt(word, SurfacePairOf{}), reinterpret_cast<SurfacePair*>(totals), (int)n,
                                                 SurfacePairSum{}, SurfacePair{0, 0}, st));
}
void launch_surface_scans(void* temp, size_t temp_bytes, const uint32_t* word, uint32_t n, uint32_t* voff, uint32_t* toff, hipStream_t st) {
    SALVA_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, SurfaceVIt(word, SurfaceVCount{}), voff, (int)(n + 1u), st));
    SALVA_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, SurfaceTIt(word, SurfaceTCount{}), toff, (int)(n + 1u), st));
}

// ------------------------------------------------------------------------------------------------ emit
// origin + (float)i * spacing, product and sum each rounded (field.hip field_node)
__device__ __forceinline__ float surface_coord(float origin, float spacing, uint32_t i) { return origin + opaque((float)i * spacing); }

__global__ __launch_bounds__(BLOCK) void k_surface_emit(const float* __restrict__ values, float iso, SurfaceLattice g, const uint32_t* __restrict__ word,
                                                        const uint32_t* __restrict__ voff, const uint32_t* __restrict__ toff, uint64_t nv, uint64_t nt,
                                                        float* __restrict__ vertices, uint32_t* __restrict__ triangles) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= g.n) return;
    const uint32_t w = word[i];
    if (!w) return;  // (most nodes: no vertex and no triangle)
    const SurfaceNode p = surface_node(g, i);
    const uint32_t mask = w & SURFACE_MASK_BITS;
    if (mask) {
        const float fa = values[i];
        const float pa[3] = {surface_coord(g.origin[0], g.spacing, p.ix), surface_coord(g.origin[1], g.spacing, p.iy),
                             surface_coord(g.origin[2], g.spacing, p.iz)};
        const float pb[3] = {surface_coord(g.origin[0], g.spacing, p.ix + 1u), surface_coord(g.origin[1], g.spacing, p.iy + 1u),
                             surface_coord(g.origin[2], g.spacing, p.iz + 1u)};
        uint64_t at = voff[i];
#pragma unroll
        for (uint32_t b = 0; b < 7; ++b) {
            if (!((mask >> b) & 1u)) continue;
            const uint32_t k = b + 1u;
            const bool ox = (k & 4u) != 0u, oy = (k & 2u) != 0u, oz = (k & 1u) != 0u;
            const float fb = values[i + (ox ? p.sx : 0u) + (oy ? p.sy : 0u) + (oz ? 1u : 0u)];
            const float t = (iso - fa) / (fb - fa);
            const float x = pa[0] + opaque(t * ((ox ? pb[0] : pa[0]) - pa[0]));
            const float y = pa[1] + opaque(t * ((oy ? pb[1] : pa[1]) - pa[1]));
            const float z = pa[2] + opaque(t * ((oz ? pb[2] : pa[2]) - pa[2]));
            if (at < nv) { vertices[3 * at] = x; vertices[3 * at + 1] = y; vertices[3 * at + 2] = z; }
            ++at;
        }
    }
    if (!((w >> SURFACE_TCOUNT_SHIFT) & 15u)) return;
    // (a node with triangles is the min corner of a cell: all eight corners are there)
    const uint32_t inside = surface_corners(values, iso, g, i, p, values[i]) >> 8;
    uint64_t at = toff[i];
#pragma unroll 1
    for (uint32_t t = 0; t < 6; ++t) {
        // (the case as one 64-bit word: byte 0 the count, bytes 1 .. 6 the corners)
        const uint64_t cs = *reinterpret_cast<const uint64_t*>(&SURFACE_CASES.c[t][surface_tet_mask(inside, t)]);
        const uint32_t ntri = (uint32_t)(cs & 0xffu);
        for (uint32_t k = 0; k < ntri; ++k) {
            uint32_t idx[3];
#pragma unroll
            for (uint32_t c = 0; c < 3; ++c) {
                const uint32_t e = (uint32_t)(cs >> (8u * (1u + 3u * k + c))) & 0xffu, corner = e >> 3, bit = e & 7u;
                const uint32_t owner = i + ((corner & 4u) ? p.sx : 0u) + ((corner & 2u) ? p.sy : 0u) + (corner & 1u);
                idx[c] = voff[owner] + (uint32_t)__popc(word[owner] & ((1u << bit) - 1u));
            }
            if (at < nt) { triangles[3 * at] = idx[0]; triangles[3 * at + 1] = idx[1]; triangles[3 * at + 2] = idx[2]; }
            ++at;
        }
    }
}
void launch_surface_emit(const float* values, float iso, const SurfaceLattice& g, const uint32_t* word, const uint32_t* voff, const uint32_t* toff,
                         uint64_t nv, uint64_t nt, float* vertices, uint32_t* triangles, hipStream_t st) {
    if (!g.n || !(nv || nt)) return;
    k_surface_emit<<<div_up(g.n, BLOCK), BLOCK, 0, st>>>(values, iso, g, word, voff, toff, nv, nt, vertices, triangles);
    SALVA_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ normals
__global__ __launch_bounds__(BLOCK) void k_surface_normals(float* __restrict__ g, uint64_t nv) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nv) return;
    const float gx = g[3 * i], gy = g[3 * i + 1], gz = g[3 * i + 2];
    // scaled by the largest component first, so that neither a tiny nor a huge gradient loses its direction in the squares
    const float m = fmaxf(fabsf(gx), fmaxf(fabsf(gy), fabsf(gz)));
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (m > 0.0f && isfinite(m)) {
        const float sx = gx / m, sy = gy / m, sz = gz / m;
        const float len = sqrtf(sx * sx + sy * sy + sz * sz);
        nx = -sx / len; ny = -sy / len; nz = -sz / len;
    }
    g[3 * i] = nx; g[3 * i + 1] = ny; g[3 * i + 2] = nz;
}
void launch_surface_normals(float* gradient_to_normals, uint64_t nv, hipStream_t st) {
    if (!nv) return;
    k_surface_normals<<<div_up(nv, BLOCK), BLOCK, 0, st>>>(gradient_to_normals, nv);
    SALVA_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ the fluids' box
__global__ __launch_bounds__(BLOCK) void k_surface_bounds(const float4* __restrict__ st_pos, const uint32_t* __restrict__ st_model, uint32_t n,
                                                          uint32_t mask, int32_t* __restrict__ box6, unsigned long long* __restrict__ nfinite) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    bool counted = false;
    if (i < n) {
        const uint32_t m = st_model[i];
        const float4 x = st_pos[i];
        if (m < 32u && ((mask >> m) & 1u) && isfinite(x.x) && isfinite(x.y) && isfinite(x.z)) {
            counted = true;
            const float c[3] = {x.x, x.y, x.z};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int32_t b = __float_as_int(c[a]);
                lo[a] = hi[a] = b ^ ((b >> 31) & 0x7fffffff);  // (field.h field_ordered)
            }
        }
    }
    // (every lane of the wave arrives: the reductions are wave-wide)
    const unsigned long long votes = __ballot(counted);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int32_t l = wave_min_i32(lo[a]), h = wave_max_i32(hi[a]);
        if ((threadIdx.x & (WAVE - 1)) == 0 && l <= h) { atomicMin(&box6[a], l); atomicMax(&box6[3 + a], h); }
    }
    if ((threadIdx.x & (WAVE - 1)) == 0 && votes) atomicAdd(nfinite, (unsigned long long)__popcll(votes));
}
void launch_surface_bounds(const float4* st_pos, const uint32_t* st_model, uint32_t n, uint32_t mask, int32_t* box6, unsigned long long* nfinite,
                           hipStream_t st) {
    if (!n) return;
    k_surface_bounds<<<div_up(n, BLOCK), BLOCK, 0, st>>>(st_pos, st_model, n, mask, box6, nfinite);
    SALVA_HIP_CHECK(hipGetLastError());
}

}  // namespace salva

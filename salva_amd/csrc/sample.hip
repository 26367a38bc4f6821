// sample.hip — sampling/ray_sampling.rs on the device: `shape_surface_ray_sample` / `shape_volume_ray_sample` for the analytic
// shapes of SalvaHipShape, the same loop for any other shape through host ray casts, and the two ways to use the samples without
// a host round trip (Fluid::add_particles of posed samples; a StaticSampling boundary).  DESIGN.md §13.
//
// The sampler's lattice has spacing s = 2 r and origin (aabb.mins - s) + s / 2; the lattice lines of an axis are origin, + s, + s ...
// while < aabb.maxs + s, accumulated in f32 on the host as the reference's `curr[k] += subdivision_size` does (:60-68).  Along every
// line of every axis one ray is cast from outside; its impacts are quantised to lattice indices (quantize_point :209-231,
// sample_segment :166-191) and the set of indices is the result.  Here the set is a bit lattice:
//   k_sample_mark    one thread per ray: the closed form of the cast for the shape, atomicOr of the quantised impacts
//   k_sample_count   popcount per word, followed by the exclusive scan the grid already uses (scan_u32)
//   k_sample_emit    one thread per word: its set bits, in bit order, to origin + float(q) * s — packed xyz or the float4 layout of
//                    the staging arrays, optionally posed (pose.h, the device function of k_boundary_pose)
// Bit order is lexicographic in (q_x, q_y, q_z); a row along z is padded to whole words.
// All arithmetic is f32, correctly rounded (`/`, sqrtf) and free of contraction, so that a numpy f32 reading reproduces it bit for bit.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "world.h"
#include "dcs.h"
#include "mesh.h"
#include "pose.h"
#include "raycast.h"

// (the Makefile's -ffp-contract=off already says so; the sampler's bit-for-bit specification must not depend on a build flag)
#pragma clang fp contract(off)

namespace salva {

void scan_u32(void* temp, size_t temp_bytes, const uint32_t* in, uint32_t* out, uint32_t n, hipStream_t s);  // grid.hip

struct SampleGrid {
    uint32_t nx, ny, nz, wz;   // lattice lines per axis; words per z row
    float ox, oy, oz, s;       // lattice origin and spacing
    const float *cx, *cy, *cz; // the lattice lines' coordinates
};

struct World::SampleLattice {
    SampleGrid g{};
    uint32_t nwords = 0;
    std::vector<float> coords[3];
};

namespace {

template <typename T>
__host__ __device__ __forceinline__ T sel3(int a, T x, T y, T z) { return a == 0 ? x : (a == 1 ? y : z); }

// Rust's `as u32`: saturating, NaN -> 0
__host__ __device__ __forceinline__ uint32_t sat_u32(float v) { return v > 0.0f ? (v >= 4294967296.0f ? 0xffffffffu : (uint32_t)v) : 0u; }

__host__ __device__ __forceinline__ uint32_t word_of(const SampleGrid& g, uint32_t qx, uint32_t qy, uint32_t qz) {
    return (qx * g.ny + qy) * g.wz + (qz >> 5);
}

// Where the ray along +axis through the transverse coordinates (cj, ck) — j = axis + 1, k = axis + 2 mod 3 — enters (a) and leaves
// (b) the shape; false = a miss.  The closed forms of DESIGN.md §13.
__device__ __forceinline__ bool cast_axis(const SalvaHipShape& sh, int axis, float cj, float ck, float& a, float& b) {
    const float p0 = sh.params[0], p1 = sh.params[1], p2 = sh.params[2];
    switch (sh.kind) {
        case SALVA_HIP_SHAPE_BALL: {
            const float d2 = (p0 * p0) - ((cj * cj) + (ck * ck));
            if (!(d2 > 0.0f)) return false;
            b = sqrtf(d2); a = -b;
            return true;
        }
        case SALVA_HIP_SHAPE_CUBOID: {
            const float hi = sel3(axis, p0, p1, p2), hj = sel3(axis, p1, p2, p0), hk = sel3(axis, p2, p0, p1);
            if (!(fabsf(cj) <= hj && fabsf(ck) <= hk)) return false;
            a = -hi; b = hi;
            return true;
        }
        case SALVA_HIP_SHAPE_CYLINDER: {  // axis y; p0 = half height, p1 = radius
            if (axis == 1) {              // (j, k) = (z, x)
                const float d2 = (p1 * p1) - ((ck * ck) + (cj * cj));
                if (!(d2 >= 0.0f)) return false;
                a = -p0; b = p0;
                return true;
            }
            const float cy = axis == 0 ? cj : ck, co = axis == 0 ? ck : cj;
            const float d2 = (p1 * p1) - (co * co);
            if (!(fabsf(cy) <= p0 && d2 > 0.0f)) return false;
            b = sqrtf(d2); a = -b;
            return true;
        }
        case SALVA_HIP_SHAPE_CAPSULE: {  // parry Capsule::new_y; p0 = half height of the segment, p1 = radius
            if (axis == 1) {
                const float d2 = (p1 * p1) - ((ck * ck) + (cj * cj));
                if (!(d2 > 0.0f)) return false;
                b = p0 + sqrtf(d2); a = -b;
                return true;
            }
            const float cy = axis == 0 ? cj : ck, co = axis == 0 ? ck : cj;
            const float dy = fmaxf(fabsf(cy) - p0, 0.0f);
            const float d2 = ((p1 * p1) - (dy * dy)) - (co * co);
            if (!(d2 > 0.0f)) return false;
            b = sqrtf(d2); a = -b;
            return true;
        }
        default: return false;
    }
}

__global__ __launch_bounds__(BLOCK) void k_sample_mark(SampleGrid g, SalvaHipShape shape, int volume, uint32_t* __restrict__ bits) {
    uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint64_t r0 = (uint64_t)g.ny * g.nz, r1 = (uint64_t)g.nz * g.nx, r2 = (uint64_t)g.nx * g.ny;
    int axis;
    if (t < r0) axis = 0;
    else if (t < r0 + r1) { axis = 1; t -= r0; }
    else if (t < r0 + r1 + r2) { axis = 2; t -= r0 + r1; }
    else return;
    // (j, k) = (axis + 1, axis + 2) mod 3
    const uint32_t ni = sel3(axis, g.nx, g.ny, g.nz), nj = sel3(axis, g.ny, g.nz, g.nx), nk = sel3(axis, g.nz, g.nx, g.ny);
    const float oi = sel3(axis, g.ox, g.oy, g.oz), oj = sel3(axis, g.oy, g.oz, g.ox), ok = sel3(axis, g.oz, g.ox, g.oy);
    const float* lj = sel3(axis, g.cy, g.cz, g.cx);
    const float* lk = sel3(axis, g.cz, g.cx, g.cy);
    const uint32_t aj = (uint32_t)(t / nk), ak = (uint32_t)(t % nk);  // aj < nj: t < nj * nk
    const float cj = lj[aj], ck = lk[ak];
    float a, b;
    if (!cast_axis(shape, axis, cj, ck, a, b)) return;
    const uint32_t qj = sat_u32(roundf((cj - oj) / g.s)), qk = sat_u32(roundf((ck - ok) / g.s));
    if (qj >= nj || qk >= nk) return;  // (outside the lattice: never written)
    // the reference casts again from the impact + s / 10: a chord shorter than that has no second impact
    const bool thin = (b - a) < g.s / 10.0f;
    const float fa = (a - oi) / g.s, fb = (b - oi) / g.s;
    uint32_t q0, q1;
    if (volume) {
        if (thin) return;
        q0 = sat_u32(roundf(fa)); q1 = sat_u32(roundf(fb));
        if (q0 >= ni) return;
        q1 = q1 < ni - 1u ? q1 : ni - 1u;
        if (q0 > q1) return;
    } else {
        q0 = sat_u32(ceilf(fa)); q1 = thin ? q0 : sat_u32(floorf(fb));
    }
    if (axis == 2) {  // the run lies along z: (x, y) = (qj, qk)
        const uint32_t row = (qj * g.ny + qk) * g.wz;
        if (volume) {
            for (uint32_t w = q0 >> 5; w <= (q1 >> 5); ++w) {
                const uint32_t lo = w == (q0 >> 5) ? (q0 & 31u) : 0u, hi = w == (q1 >> 5) ? (q1 & 31u) : 31u;
                const uint32_t mask = (0xffffffffu >> (31u - hi)) & (0xffffffffu << lo);
                atomicOr(&bits[row + w], mask);
            }
        } else {
            if (q0 < ni) atomicOr(&bits[row + (q0 >> 5)], 1u << (q0 & 31u));
            if (q1 < ni && q1 != q0) atomicOr(&bits[row + (q1 >> 5)], 1u << (q1 & 31u));
        }
        return;
    }
    // axis 0: (y, z) = (qj, qk), the run strides over x; axis 1: (z, x) = (qj, qk), the run strides over y
    const uint32_t qz = axis == 0 ? qk : qj, bit = 1u << (qz & 31u);
    const uint32_t base = axis == 0 ? word_of(g, 0u, qj, qz) : word_of(g, qk, 0u, qz);
    const uint32_t stride = axis == 0 ? g.ny * g.wz : g.wz;
    if (volume) {
        for (uint32_t q = q0; q <= q1; ++q) atomicOr(&bits[base + q * stride], bit);
    } else {
        if (q0 < ni) atomicOr(&bits[base + q0 * stride], bit);
        if (q1 < ni && q1 != q0) atomicOr(&bits[base + q1 * stride], bit);
    }
}

// The same for a triangle mesh: every accepted hit is one walk of the hierarchy (mesh.h mesh_next_hit), the loop around it is the host
// arm's (World::sample_host_shape) for one ray — toi = hit - origin, impact = origin + toi, the next origin = origin + (toi + s / 10),
// entry and exit alternating; a 65th accepted hit raises *err.
__device__ __forceinline__ void mark_bit(const SampleGrid& g, int axis, uint32_t qi, uint32_t qj, uint32_t qk, uint32_t* __restrict__ bits) {
    // axis 0: (x, y, z) = (qi, qj, qk); axis 1: (z, x) = (qj, qk); axis 2: (x, y) = (qj, qk)
    const uint32_t qx = sel3(axis, qi, qk, qj), qy = sel3(axis, qj, qi, qk), qz = sel3(axis, qk, qj, qi);
    atomicOr(&bits[word_of(g, qx, qy, qz)], 1u << (qz & 31u));
}

// One lattice ray of a shape that is cast at: `cast(axis, cj, ck, o)` is the toi of the ray along +axis through (cj, ck) from the
// coordinate o, +inf for a miss.
template <typename Cast>
__device__ __forceinline__ void mark_ray_hits(const SampleGrid& g, int volume, uint32_t* __restrict__ bits, uint32_t* __restrict__ err,
                                              const Cast& cast) {
    uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint64_t r0 = (uint64_t)g.ny * g.nz, r1 = (uint64_t)g.nz * g.nx, r2 = (uint64_t)g.nx * g.ny;
    int axis;
    if (t < r0) axis = 0;
    else if (t < r0 + r1) { axis = 1; t -= r0; }
    else if (t < r0 + r1 + r2) { axis = 2; t -= r0 + r1; }
    else return;
    const uint32_t ni = sel3(axis, g.nx, g.ny, g.nz), nj = sel3(axis, g.ny, g.nz, g.nx), nk = sel3(axis, g.nz, g.nx, g.ny);
    const float oi = sel3(axis, g.ox, g.oy, g.oz), oj = sel3(axis, g.oy, g.oz, g.ox), ok = sel3(axis, g.oz, g.ox, g.oy);
    const float* lj = sel3(axis, g.cy, g.cz, g.cx);
    const float* lk = sel3(axis, g.cz, g.cx, g.cy);
    const uint32_t aj = (uint32_t)(t / nk), ak = (uint32_t)(t % nk);  // aj < nj: t < nj * nk
    const float cj = lj[aj], ck = lk[ak];
    const uint32_t qj = sat_u32(roundf((cj - oj) / g.s)), qk = sat_u32(roundf((ck - ok) / g.s));
    if (qj >= nj || qk >= nk) return;  // (outside the lattice: never written)
    const float step = g.s / 10.0f;
    float o = oi, prev = 0.0f;
    bool entry = true, has_prev = false;
    for (int hits = 0;; ++hits) {
        const float toi = cast(axis, cj, ck, o);
        if (!(toi < __builtin_inff())) break;
        if (hits == MESH_MAX_HITS) { atomicOr(err, 1u); break; }
        const float impact = o + toi;
        if (!volume) {
            const float f = (impact - oi) / g.s;
            const uint32_t q = sat_u32(entry ? ceilf(f) : floorf(f));
            if (q < ni) mark_bit(g, axis, q, qj, qk, bits);
            entry = !entry;
        } else if (has_prev) {
            const uint32_t q0 = sat_u32(roundf((prev - oi) / g.s)), qe = sat_u32(roundf((impact - oi) / g.s));
            const uint32_t q1 = qe < ni - 1u ? qe : ni - 1u;
            for (uint32_t q = q0; q <= q1 && q < ni; ++q) mark_bit(g, axis, q, qj, qk, bits);
            has_prev = false;
        } else {
            prev = impact; has_prev = true;
        }
        o = o + (toi + step);
    }
}

__global__ __launch_bounds__(BLOCK) void k_sample_mesh_mark(SampleGrid g, MeshDev mesh, int volume, uint32_t* __restrict__ bits,
                                                            uint32_t* __restrict__ err) {
    mark_ray_hits(g, volume, bits, err, [&](int axis, float cj, float ck, float o) { return mesh_next_hit(mesh, axis, cj, ck, o) - o; });
}

// The same for a compound (raycast.h): every accepted hit is one walk over the parts.  The part index is wave-uniform
// and the table const __restrict__, so the parts' records come through the scalar cache as in k_dcs_compound_project.
__global__ __launch_bounds__(BLOCK) void k_compound_mark(SampleGrid g, const CompoundPartDev* __restrict__ parts, uint32_t nparts, int volume,
                                                         uint32_t* __restrict__ bits, uint32_t* __restrict__ err) {
    mark_ray_hits(g, volume, bits, err, [&](int axis, float cj, float ck, float o) {
        return compound_cast_ray<true>(parts, nparts, sel3(axis, o, ck, cj), sel3(axis, cj, o, ck), sel3(axis, ck, cj, o), axis == 0 ? 1.0f : 0.0f,
                                       axis == 1 ? 1.0f : 0.0f, axis == 2 ? 1.0f : 0.0f);
    });
}

// cnt[w] = set bits of word w; cnt[nwords] = 0, so that the exclusive scan over nwords + 1 entries ends in the total
__global__ __launch_bounds__(BLOCK) void k_sample_count(uint32_t nwords, const uint32_t* __restrict__ bits, uint32_t* __restrict__ cnt) {
    const uint32_t w = blockIdx.x * BLOCK + threadIdx.x;
    if (w <= nwords) cnt[w] = w < nwords ? (uint32_t)__popc(bits[w]) : 0u;
}

struct SampleEmit {
    float* xyz;        // packed [x, y, z] per sample, or
    float4* f4;        // (x, y, z, w4) per sample
    float w4;
    float4* vel;       // with f4: (vx, vy, vz, 0) per sample; may be null
    float vx, vy, vz;
    int posed;         // with f4: q * p + t (pose.h)
    float q[4], t[3];
};

__global__ __launch_bounds__(BLOCK) void k_sample_emit(SampleGrid g, uint32_t nwords, const uint32_t* __restrict__ bits,
                                                       const uint32_t* __restrict__ off, SampleEmit e) {
    const uint32_t w = blockIdx.x * BLOCK + threadIdx.x;
    if (w >= nwords) return;
    uint32_t m = bits[w];
    if (!m) return;
    uint32_t o = off[w];
    const uint32_t row = w / g.wz, wz = w - row * g.wz, qx = row / g.ny, qy = row - qx * g.ny;
    const float x = g.ox + ((float)qx * g.s), y = g.oy + ((float)qy * g.s);  // unquantize_points (:193-207)
    while (m) {
        const uint32_t b = (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1u;
        const float z = g.oz + ((float)(wz * 32u + b) * g.s);
        if (e.xyz) {
            e.xyz[3 * (size_t)o] = x; e.xyz[3 * (size_t)o + 1] = y; e.xyz[3 * (size_t)o + 2] = z;
        } else {
            float4 p = make_float4(x, y, z, e.w4);
            if (e.posed) pose_point(e.q[0], e.q[1], e.q[2], e.q[3], e.t[0], e.t[1], e.t[2], x, y, z, p.x, p.y, p.z);
            e.f4[o] = p;
            if (e.vel) e.vel[o] = make_float4(e.vx, e.vy, e.vz, 0.0f);
        }
        ++o;
    }
}

void check_sample_args(float particle_rad, int mode) {
    if (!(particle_rad > 0.0f) || !std::isfinite(particle_rad)) throw HipError(SALVA_HIP_E_INVALID, "the particle radius must be positive");
    if (mode != SALVA_HIP_SAMPLE_SURFACE && mode != SALVA_HIP_SAMPLE_VOLUME)
        throw HipError(SALVA_HIP_E_INVALID, "unknown sampling mode (SALVA_HIP_SAMPLE_SURFACE / SALVA_HIP_SAMPLE_VOLUME)");
}

// half extents of the shape's local AABB (`shape.compute_aabb(&Isometry::identity())`)
void shape_half_extents(const SalvaHipShape& shape, float ext[3]) {
    check_shape_params(shape, "shape parameters must be positive");
    switch (shape.kind) {
        case SALVA_HIP_SHAPE_BALL: ext[0] = ext[1] = ext[2] = shape.params[0]; break;
        case SALVA_HIP_SHAPE_CUBOID: ext[0] = shape.params[0]; ext[1] = shape.params[1]; ext[2] = shape.params[2]; break;
        case SALVA_HIP_SHAPE_CAPSULE: ext[0] = ext[2] = shape.params[1]; ext[1] = shape.params[0] + shape.params[1]; break;
        default: ext[0] = ext[2] = shape.params[1]; ext[1] = shape.params[0]; break;  // cylinder
    }
}

}  // namespace

// The lattice of a local AABB [mins, maxs] (surface_ray_sample :33-38): coordinates on the host, uploaded; the bit lattice cleared.
void World::sample_lattice(const float mins[3], const float maxs[3], float particle_rad, SampleLattice& L) {
    const float s = particle_rad * 2.0f;
    float origin[3];
    uint64_t nbits = 1;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(mins[a]) || !std::isfinite(maxs[a]) || !(mins[a] <= maxs[a]))
            throw HipError(SALVA_HIP_E_INVALID, "shape sampling: the shape's aabb is empty, infinite or NaN");
        const float lo = mins[a] - s, hi = maxs[a] + s;  // Aabb::loosened(subdivision_size)
        origin[a] = lo + s / 2.0f;
        std::vector<float>& c = L.coords[a];
        c.clear();
        for (float v = origin[a]; v < hi;) {
            // (indices travel through f32 quotients, exact up to 2^24; a spacing that vanishes against the coordinates never ends)
            if (c.size() >= (1u << 24)) throw HipError(SALVA_HIP_E_CAPACITY, "shape sampling: more than 2^24 lattice lines along one axis");
            c.push_back(v);
            const float nv = v + s;
            if (!(nv > v)) throw HipError(SALVA_HIP_E_CAPACITY, "shape sampling: the lattice spacing vanishes against the shape's extent");
            v = nv;
        }
        nbits *= (uint64_t)c.size();
        if (nbits > (1ull << 32)) throw HipError(SALVA_HIP_E_CAPACITY, "shape sampling: a lattice of more than 2^32 points");
    }
    SampleGrid& g = L.g;
    g.nx = (uint32_t)L.coords[0].size(); g.ny = (uint32_t)L.coords[1].size(); g.nz = (uint32_t)L.coords[2].size();
    g.wz = (g.nz + 31u) / 32u;
    g.ox = origin[0]; g.oy = origin[1]; g.oz = origin[2]; g.s = s;
    const uint64_t nwords = (uint64_t)g.nx * g.ny * g.wz;
    if (nwords >= (1ull << 31)) throw HipError(SALVA_HIP_E_CAPACITY, "shape sampling: a lattice of more than 2^31 words");
    L.nwords = (uint32_t)nwords;
    const size_t nc = (size_t)g.nx + g.ny + g.nz;
    smp_coords.ensure(nc, stream, false, 1.25f);
    smp_bits.ensure(std::max<size_t>(L.nwords, 1), stream, false, 1.25f);
    smp_cnt.ensure((size_t)L.nwords + 1, stream, false, 1.25f);
    smp_off.ensure((size_t)L.nwords + 1, stream, false, 1.25f);
    std::vector<float> all;
    all.reserve(nc);
    for (int a = 0; a < 3; ++a) all.insert(all.end(), L.coords[a].begin(), L.coords[a].end());
    SALVA_HIP_CHECK(hipMemcpyAsync(smp_coords.p, all.data(), nc * sizeof(float), hipMemcpyHostToDevice, stream));
    SALVA_HIP_CHECK(hipMemsetAsync(smp_bits.p, 0, (size_t)L.nwords * sizeof(uint32_t), stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));  // (`all` leaves scope)
    g.cx = smp_coords.p; g.cy = g.cx + g.nx; g.cz = g.cy + g.ny;
}

// The bit lattice of a geometry: one lattice, three mark kernels.  A built-in shape is marked in closed form over its
// own half extents.  A mesh or a compound (§17) is cast at hit by hit over the lattice of its local box — a
// compound's is the unloosened merge of the parts' boxes, parry's local AABB of a compound — and its error word is a ray with more
// than 64 accepted hits.
void World::sample_mark(const Geom& geom, float particle_rad, int mode, SampleLattice& L) {
    check_sample_args(particle_rad, mode);
    const int volume = mode == SALVA_HIP_SAMPLE_VOLUME ? 1 : 0;
    const SampleGrid& g = L.g;
    auto rays = [&] { return (uint64_t)g.ny * g.nz + (uint64_t)g.nz * g.nx + (uint64_t)g.nx * g.ny; };
    if (geom.kind != SALVA_HIP_SHAPE_MESH && geom.kind != SALVA_HIP_SHAPE_COMPOUND) {
        float ext[3], mins[3];
        shape_half_extents(geom.shape, ext);
        for (int a = 0; a < 3; ++a) mins[a] = -ext[a];
        sample_lattice(mins, ext, particle_rad, L);
        k_sample_mark<<<div_up(rays(), BLOCK), BLOCK, 0, stream>>>(g, geom.shape, volume, smp_bits.p);
        SALVA_HIP_CHECK(hipGetLastError());
        return;
    }
    sample_lattice(geom.mins(), geom.maxs(), particle_rad, L);
    smp_err.ensure(1);
    SALVA_HIP_CHECK(hipMemsetAsync(smp_err.p, 0, sizeof(uint32_t), stream));
    if (geom.mesh) k_sample_mesh_mark<<<div_up(rays(), BLOCK), BLOCK, 0, stream>>>(g, geom.mesh->dev(), volume, smp_bits.p, smp_err.p);
    else k_compound_mark<<<div_up(rays(), BLOCK), BLOCK, 0, stream>>>(g, geom.parts(), geom.nparts(), volume, smp_bits.p, smp_err.p);
    SALVA_HIP_CHECK(hipGetLastError());
    uint32_t err = 0;
    SALVA_HIP_CHECK(hipMemcpyAsync(&err, smp_err.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    if (err)
        throw HipError(SALVA_HIP_E_CAPACITY, geom.mesh ? "mesh sampling: a ray crosses the mesh more than 64 times"
                                                       : "compound sampling: a ray crosses the parts' boundaries more than 64 times");
}

// count + scan; returns the number of samples (smp_off then holds every word's first output index)
uint32_t World::sample_count(const SampleLattice& L) {
    const uint32_t n1 = L.nwords + 1u;
    k_sample_count<<<div_up(n1, BLOCK), BLOCK, 0, stream>>>(L.nwords, smp_bits.p, smp_cnt.p);
    SALVA_HIP_CHECK(hipGetLastError());
    const size_t tb = scan_temp_bytes(n1);
    ensure_cub_temp(tb);
    scan_u32(cub_temp.p, tb, smp_cnt.p, smp_off.p, n1, stream);
    uint32_t total = 0;
    SALVA_HIP_CHECK(hipMemcpyAsync(&total, smp_off.p + L.nwords, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    return total;
}

// the samples in local coordinates to the host, when `capacity` holds them all (the convention of particles_in_aabb)
int64_t World::sample_download(const SampleLattice& L, uint64_t capacity, float* out_xyz) {
    const uint32_t total = sample_count(L);
    if (!total || !out_xyz || capacity < total) return total;
    smp_out.ensure(3 * (size_t)total, stream, false, 1.25f);
    SampleEmit e{};
    e.xyz = smp_out.p;
    k_sample_emit<<<div_up(L.nwords, BLOCK), BLOCK, 0, stream>>>(L.g, L.nwords, smp_bits.p, smp_off.p, e);
    SALVA_HIP_CHECK(hipGetLastError());
    SALVA_HIP_CHECK(hipMemcpyAsync(out_xyz, smp_out.p, 3 * (size_t)total * sizeof(float), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    return total;
}

int64_t World::sample(const GeomArg& geom, float particle_rad, int mode, uint64_t capacity, float* out_xyz) {
    use_device();
    SampleLattice L;
    sample_mark(geom_of(geom), particle_rad, mode, L);
    return sample_download(L, capacity, out_xyz);
}

// Any other shape: the casts stay with the host.  The reference's loop (surface_ray_sample :40-53, volume_ray_sample :103-127) runs
// in rounds over all rays of an axis at once: cast the live rays, quantise the hits (entry and exit alternate), advance each origin
// by toi + s / 10, go on with the rays that hit.  A ray may cross the shape any number of times (concave shapes).
int64_t World::sample_host_shape(const SalvaHipHostRayShape& shape, float particle_rad, int mode, uint64_t capacity, float* out_xyz) {
    use_device();
    check_sample_args(particle_rad, mode);
    if (!shape.aabb || !shape.cast) throw HipError(SALVA_HIP_E_INVALID, "a host ray shape needs both callbacks");
    float mins[3], maxs[3];
    shape.aabb(shape.user, mins, maxs);
    SampleLattice L;
    sample_lattice(mins, maxs, particle_rad, L);
    const SampleGrid& g = L.g;
    const bool volume = mode == SALVA_HIP_SAMPLE_VOLUME;
    std::vector<uint32_t> bits((size_t)L.nwords, 0u);
    const uint32_t N[3] = {g.nx, g.ny, g.nz};
    const float O[3] = {g.ox, g.oy, g.oz};
    const float s = g.s, step = s / 10.0f;
    auto set_bit = [&](const uint32_t q[3]) {
        if (q[0] < N[0] && q[1] < N[1] && q[2] < N[2]) bits[word_of(g, q[0], q[1], q[2])] |= 1u << (q[2] & 31u);
    };
    struct Ray { uint32_t qj, qk; float prev; uint8_t entry, has_prev; };
    std::vector<Ray> rays;
    std::vector<float> origins, toi;
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        rays.clear(); origins.clear();
        for (uint32_t aj = 0; aj < N[j]; ++aj)
            for (uint32_t ak = 0; ak < N[k]; ++ak) {
                const float cj = L.coords[j][aj], ck = L.coords[k][ak];
                float o[3];
                o[i] = O[i]; o[j] = cj; o[k] = ck;
                origins.insert(origins.end(), o, o + 3);
                rays.push_back(Ray{sat_u32(roundf((cj - O[j]) / s)), sat_u32(roundf((ck - O[k]) / s)), 0.0f, 1, 0});
            }
        for (int round = 0; !rays.empty(); ++round) {
            if (round >= 64)
                throw HipError(SALVA_HIP_E_INVALID, "shape sampling: a ray still hits the host shape after 64 rounds (a cast that never misses?)");
            const uint32_t nr = (uint32_t)rays.size();
            toi.assign(nr, -1.0f);
            shape.cast(shape.user, nr, origins.data(), i, toi.data());
            uint32_t live = 0;
            for (uint32_t r = 0; r < nr; ++r) {
                const float t = toi[r];
                if (!(t >= 0.0f)) continue;  // negative or NaN: a miss, the ray is done
                Ray ray = rays[r];
                const float oi = origins[3 * r + i], impact = oi + t;
                uint32_t q[3];
                q[j] = ray.qj; q[k] = ray.qk;
                if (!volume) {
                    const float f = (impact - O[i]) / s;
                    q[i] = sat_u32(ray.entry ? ceilf(f) : floorf(f));
                    set_bit(q);
                    ray.entry ^= 1;
                } else if (ray.has_prev) {
                    const uint32_t q0 = sat_u32(roundf((ray.prev - O[i]) / s)), q1 = std::min(sat_u32(roundf((impact - O[i]) / s)), N[i] - 1u);
                    for (uint32_t v = q0; v <= q1 && v < N[i]; ++v) { q[i] = v; set_bit(q); }
                    ray.has_prev = 0;
                } else {
                    ray.prev = impact; ray.has_prev = 1;
                }
                rays[live] = ray;
                origins[3 * live] = origins[3 * r]; origins[3 * live + 1] = origins[3 * r + 1]; origins[3 * live + 2] = origins[3 * r + 2];
                origins[3 * live + i] = oi + (t + step);
                ++live;
            }
            rays.resize(live); origins.resize(3 * (size_t)live);
        }
    }
    if (L.nwords) SALVA_HIP_CHECK(hipMemcpyAsync(smp_bits.p, bits.data(), (size_t)L.nwords * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    return sample_download(L, capacity, out_xyz);  // (synchronises before `bits` leaves scope)
}

static const char* const kDecomposedSampling =
    "shape sampling does not edit a running decomposed world: sample with salva_hip_sample_shape and add the particles collectively "
    "with salva_hip_add_particles";

// Fluid::add_particles of the posed samples, one velocity for all: the positions go from the bit lattice straight into the staging
// array.
int64_t World::append_sampled(uint32_t slot, const SampleLattice& L, const float t[3], const float q[4], const float* vel_h) {
    const uint32_t total = sample_count(L);
    if (!total) return 0;
    const uint64_t at = append_particles(slot, total);
    const float r = prm.particle_radius;
    SampleEmit e{};
    e.f4 = st_pos.p + at;
    e.w4 = r * r * r * 6.4f;  // Fluid::particle_volume, as append_particles filled it
    e.posed = 1;
    for (int a = 0; a < 4; ++a) e.q[a] = q[a];
    for (int a = 0; a < 3; ++a) e.t[a] = t[a];
    if (vel_h) { e.vel = st_vel.p + at; e.vx = vel_h[0]; e.vy = vel_h[1]; e.vz = vel_h[2]; }
    k_sample_emit<<<div_up(L.nwords, BLOCK), BLOCK, 0, stream>>>(L.g, L.nwords, smp_bits.p, smp_off.p, e);
    SALVA_HIP_CHECK(hipGetLastError());
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    return total;
}

int64_t World::add_particles_sampled(uint32_t slot, const GeomArg& geom, const float t[3], const float q[4], int mode, const float* vel_h) {
    use_device();
    if (slot >= fluids.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot out of range");
    if (comm && dist_started) throw HipError(SALVA_HIP_E_INVALID, kDecomposedSampling);
    for (int a = 0; a < 4; ++a)
        if (!std::isfinite(q[a]) || (a < 3 && !std::isfinite(t[a]))) throw HipError(SALVA_HIP_E_INVALID, "non-finite pose");
    SampleLattice L;
    sample_mark(geom_of(geom), prm.particle_radius, mode, L);
    return append_sampled(slot, L, t, q, vel_h);
}

// salva_hip_set_boundary_sampling with the surface samples at the world's particle radius as the local points, kept on the device
int64_t World::boundary_from_sampled(uint32_t slot, const SampleLattice& L, uint32_t memberships, uint32_t filter) {
    const uint32_t total = sample_count(L);
    const std::function<void(float4*)> fill = [&](float4* dst) {
        SampleEmit e{};
        e.f4 = dst;  // (w = 0, as an uploaded boundary position carries it)
        k_sample_emit<<<div_up(L.nwords, BLOCK), BLOCK, 0, stream>>>(L.g, L.nwords, smp_bits.p, smp_off.p, e);
        SALVA_HIP_CHECK(hipGetLastError());
    };
    set_boundary_sampling(slot, total, nullptr, memberships, filter, &fill);
    return total;
}

int64_t World::set_boundary_sampling_from(uint32_t slot, const GeomArg& geom, uint32_t memberships, uint32_t filter) {
    use_device();
    if (slot > bounds.size()) throw HipError(SALVA_HIP_E_INVALID, "boundary slot out of range (slots are dense)");
    if (comm && dist_started) throw HipError(SALVA_HIP_E_INVALID, kDecomposedSampling);
    SampleLattice L;
    // (nothing keeps a mesh or a compound: a boundary sampled from it holds its points only)
    sample_mark(geom_of(geom), prm.particle_radius, SALVA_HIP_SAMPLE_SURFACE, L);
    return boundary_from_sampled(slot, L, memberships, filter);
}

}  // namespace salva

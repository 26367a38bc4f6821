// raycast.h — general-direction ray casts against the five kinds of part a compound holds (compound.h), and the walk over the parts
// that the ray sampler runs for a compound (sample.hip k_compound_mark; DESIGN.md §17 "Ray sampling").  One rule for every kind, this
// project's reading of parry 0.18's cast_local_ray with solid = false: the cast of o + t d (d of unit length up to rounding) at a part
// is the smallest t >= 0 at which the ray crosses the part's boundary — the entry when o is outside, the exit when it is inside — and
// +inf for a miss.  parry's Compound::cast_local_ray is the minimum over the parts of part.cast_ray(part_pos, ray, ..): here the ray
// is carried into the part's frame (quat_rot with the conjugate, on o - t_k and on d), cast there, and the smallest t over the parts
// in index order is the result; equal t from two parts is one hit.
//
// The four convex kinds are cast as intervals [t0, t1] = ray ∩ solid (empty: t0 = +inf, t1 = -inf), the crossing is t0 if t0 >= 0, else
// t1 if t1 >= 0, else a miss:
//   ball      the quadratic about the point of closest approach: tm = -(o.d) / (d.d), p = o + tm d, disc = r r - p.p > 0,
//             half = sqrt(disc / (d.d)), [tm - half, tm + half] (about tm, not about o: the error stays an ulp of the coordinates
//             however far away the origin is)
//   cuboid    slabs: per axis ((-h - o) / d, (h - o) / d) ordered, d = 0: |o| <= h or empty; the largest entry, the smallest exit
//   cylinder  (axis y) the side's quadratic in the (x, z) plane — the ball's, in two dimensions; a ray along y: r r - (ox ox + oz oz) > 0
//             or empty — intersected with the slab |y| <= hh: an entry through a cap is the slab's, through the side the quadratic's
//   capsule   (axis y) the hull of three intervals: that cylinder's and the balls' about (0, +-hh, 0)
// and for the cylinder and the capsule, which parry casts with GJK, these closed forms ARE the specification, as in §13.
//   mesh      the general-direction twin of mesh_next_hit (mesh.h): the stackless walk with a ray / box test, every triangle in a frame
//             sheared so that the ray runs along its dominant axis kz (the largest |d|, the lower index on a tie; kx = kz + 1, ky =
//             kz + 2 mod 3): Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]; a vertex v becomes A = v - o, X = A[kx] - Sx A[kz],
//             Y = A[ky] - Sy A[kz], Z = Sz A[kz].  The edge functions are mesh_edge's at (0, 0) — endpoints in vertex-index order, so
//             the two triangles of a shared edge compute the same number with opposite sign and a ray through an edge or a vertex
//             belongs to both — and a hit needs all three of one sign, a sum != 0 and (0, 0) within the box of (X, Y) of the three
//             vertices; t = (e0 Z0 + e1 Z1 + e2 Z2) / sum, clamped to [min Z, max Z].
// The two conditions that look redundant are what makes the pruning exact: X, Y and Z are monotone in the vertex's coordinates
// operation by operation, so a node's box gives bounds that hold for the COMPUTED X, Y, Z of every vertex inside it, and a node is
// left out only when every triangle in it would fail the box condition or could not give a t in [0, best).  The walk equals the pass over
// all triangles bit for bit (tests/compound_cast_check.hip).  A part is left out when the ray misses its loosened box (compound.h
// CompoundPartDev::lo / hi) within [0, best].
//
// f32, free of contraction, `/` and sqrtf correctly rounded: tests/compound_cast_reading.py reproduces every cast bit for bit.
#pragma once
#include "compound.h"

namespace salva {

#ifdef __HIPCC__
__host__ __device__ __forceinline__ float ray_dot(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    return ((ax * bx) + (ay * by)) + (az * bz);
}

// the first boundary crossing of an interval at t >= 0
__host__ __device__ __forceinline__ float ray_crossing(float t0, float t1) {
    return t0 >= 0.0f ? t0 : (t1 >= 0.0f ? t1 : __builtin_inff());
}

__host__ __device__ __forceinline__ void ray_ball(float ox, float oy, float oz, float dx, float dy, float dz, float r, float& t0, float& t1) {
#pragma clang fp contract(off)
    t0 = __builtin_inff(); t1 = -__builtin_inff();
    const float a = ray_dot(dx, dy, dz, dx, dy, dz), b = ray_dot(ox, oy, oz, dx, dy, dz);
    const float tm = (-b) / a;
    const float px = ox + (tm * dx), py = oy + (tm * dy), pz = oz + (tm * dz);
    const float disc = (r * r) - ray_dot(px, py, pz, px, py, pz);
    if (!(disc > 0.0f)) return;
    const float half = sqrtf(disc / a);
    t0 = tm - half; t1 = tm + half;
}

// one slab |x| <= h intersected into [t0, t1]; false: the ray runs beside it
__host__ __device__ __forceinline__ bool ray_slab(float o, float d, float h, float& t0, float& t1) {
#pragma clang fp contract(off)
    if (d == 0.0f) return fabsf(o) <= h;
    const float u = ((-h) - o) / d, v = (h - o) / d;
    t0 = fmaxf(t0, fminf(u, v)); t1 = fminf(t1, fmaxf(u, v));
    return true;
}

__host__ __device__ __forceinline__ void ray_cuboid(float ox, float oy, float oz, float dx, float dy, float dz, float hx, float hy, float hz,
                                                    float& t0, float& t1) {
    float a = -__builtin_inff(), b = __builtin_inff();
    const bool onx = ray_slab(ox, dx, hx, a, b), ony = ray_slab(oy, dy, hy, a, b), onz = ray_slab(oz, dz, hz, a, b);
    const bool hit = onx && ony && onz && a <= b;
    t0 = hit ? a : __builtin_inff(); t1 = hit ? b : -__builtin_inff();
}

__host__ __device__ __forceinline__ void ray_cylinder(float ox, float oy, float oz, float dx, float dy, float dz, float hh, float r, float& t0,
                                                      float& t1) {
#pragma clang fp contract(off)
    t0 = __builtin_inff(); t1 = -__builtin_inff();
    float s0 = -__builtin_inff(), s1 = __builtin_inff();
    const float a = (dx * dx) + (dz * dz);
    if (a > 0.0f) {
        const float b = (ox * dx) + (oz * dz);
        const float tm = (-b) / a;
        const float px = ox + (tm * dx), pz = oz + (tm * dz);
        const float disc = (r * r) - ((px * px) + (pz * pz));
        if (!(disc > 0.0f)) return;
        const float half = sqrtf(disc / a);
        s0 = tm - half; s1 = tm + half;
    } else if (!((r * r) - ((ox * ox) + (oz * oz)) > 0.0f)) {
        return;
    }
    if (!ray_slab(oy, dy, hh, s0, s1) || !(s0 <= s1)) return;
    t0 = s0; t1 = s1;
}

__host__ __device__ __forceinline__ void ray_capsule(float ox, float oy, float oz, float dx, float dy, float dz, float hh, float r, float& t0,
                                                     float& t1) {
#pragma clang fp contract(off)
    float a0, a1, b0, b1;
    ray_cylinder(ox, oy, oz, dx, dy, dz, hh, r, t0, t1);
    ray_ball(ox, oy - hh, oz, dx, dy, dz, r, a0, a1);
    ray_ball(ox, oy + hh, oz, dx, dy, dz, r, b0, b1);
    t0 = fminf(t0, fminf(a0, b0)); t1 = fmaxf(t1, fmaxf(a1, b1));
}

// a ball, a cuboid, a capsule or a cylinder in its own frame: `S` anything with `kind` and `p` (a compound's part)
template <typename S>
__host__ __device__ __forceinline__ float shape_cast_ray(const S& s, float ox, float oy, float oz, float dx, float dy, float dz) {
    float t0, t1;
    if (s.kind == SALVA_HIP_SHAPE_BALL) ray_ball(ox, oy, oz, dx, dy, dz, s.p[0], t0, t1);
    else if (s.kind == SALVA_HIP_SHAPE_CAPSULE) ray_capsule(ox, oy, oz, dx, dy, dz, s.p[0], s.p[1], t0, t1);
    else if (s.kind == SALVA_HIP_SHAPE_CYLINDER) ray_cylinder(ox, oy, oz, dx, dy, dz, s.p[0], s.p[1], t0, t1);
    else ray_cuboid(ox, oy, oz, dx, dy, dz, s.p[0], s.p[1], s.p[2], t0, t1);
    return ray_crossing(t0, t1);
}

// The smallest t in [0, best) at which the ray crosses a triangle of the mesh; `best` when there is none.
__host__ __device__ __forceinline__ float mesh_cast_ray(const MeshDev& m, float ox, float oy, float oz, float dx, float dy, float dz, float best) {
#pragma clang fp contract(off)
    const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
    const int kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    const float dk = mesh_sel3(kz, dx, dy, dz);
    const float Sx = mesh_sel3(kz, dy, dz, dx) / dk, Sy = mesh_sel3(kz, dz, dx, dy) / dk, Sz = 1.0f / dk;
    const float px = mesh_sel3(kz, oy, oz, ox), py = mesh_sel3(kz, oz, ox, oy), pz = mesh_sel3(kz, ox, oy, oz);
    uint32_t i = 0;
    while (i < m.nnodes) {
        const float4 a = m.nodes[2 * i], b = m.nodes[2 * i + 1];
        const uint32_t leaf = mesh_bits(b.w);
        const float zl = mesh_sel3(kz, a.x, a.y, a.z) - pz, zh = mesh_sel3(kz, b.x, b.y, b.z) - pz;
        const float u0 = Sx * zl, u1 = Sx * zh, v0 = Sy * zl, v1 = Sy * zh, w0 = Sz * zl, w1 = Sz * zh;
        const float Xl = (mesh_sel3(kz, a.y, a.z, a.x) - px) - fmaxf(u0, u1), Xh = (mesh_sel3(kz, b.y, b.z, b.x) - px) - fminf(u0, u1);
        const float Yl = (mesh_sel3(kz, a.z, a.x, a.y) - py) - fmaxf(v0, v1), Yh = (mesh_sel3(kz, b.z, b.x, b.y) - py) - fminf(v0, v1);
        const bool in = Xl <= 0.0f && Xh >= 0.0f && Yl <= 0.0f && Yh >= 0.0f && fmaxf(w0, w1) >= 0.0f && fminf(w0, w1) < best;
        if (in && leaf) {
            const uint32_t first = leaf >> 3, end = first + (leaf & 7u);
            for (uint32_t t = first; t < end; ++t) {
                const uint4 tr = m.tris[t];
                const float4 q0 = m.verts[tr.x], q1 = m.verts[tr.y], q2 = m.verts[tr.z];
                const float A0 = mesh_sel3(kz, q0.x, q0.y, q0.z) - pz, A1 = mesh_sel3(kz, q1.x, q1.y, q1.z) - pz, A2 = mesh_sel3(kz, q2.x, q2.y, q2.z) - pz;
                const float X0 = (mesh_sel3(kz, q0.y, q0.z, q0.x) - px) - (Sx * A0), Y0 = (mesh_sel3(kz, q0.z, q0.x, q0.y) - py) - (Sy * A0);
                const float X1 = (mesh_sel3(kz, q1.y, q1.z, q1.x) - px) - (Sx * A1), Y1 = (mesh_sel3(kz, q1.z, q1.x, q1.y) - py) - (Sy * A1);
                const float X2 = (mesh_sel3(kz, q2.y, q2.z, q2.x) - px) - (Sx * A2), Y2 = (mesh_sel3(kz, q2.z, q2.x, q2.y) - py) - (Sy * A2);
                const bool boxed = fminf(fminf(X0, X1), X2) <= 0.0f && fmaxf(fmaxf(X0, X1), X2) >= 0.0f && fminf(fminf(Y0, Y1), Y2) <= 0.0f &&
                                   fmaxf(fmaxf(Y0, Y1), Y2) >= 0.0f;
                // e_k: the edge opposite vertex k
                const float e0 = mesh_edge(tr.y, tr.z, X1, Y1, X2, Y2, 0.0f, 0.0f), e1 = mesh_edge(tr.z, tr.x, X2, Y2, X0, Y0, 0.0f, 0.0f),
                            e2 = mesh_edge(tr.x, tr.y, X0, Y0, X1, Y1, 0.0f, 0.0f);
                const float sum = (e0 + e1) + e2;
                const bool hit = ((e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) || (e0 <= 0.0f && e1 <= 0.0f && e2 <= 0.0f)) && sum != 0.0f && boxed;
                if (!hit) continue;
                const float Z0 = Sz * A0, Z1 = Sz * A1, Z2 = Sz * A2;
                const float h = (((e0 * Z0) + (e1 * Z1)) + (e2 * Z2)) / sum;
                const float tt = fminf(fmaxf(h, fminf(fminf(Z0, Z1), Z2)), fmaxf(fmaxf(Z0, Z1), Z2));
                if (tt >= 0.0f && tt < best) best = tt;
            }
        }
        i = (in && !leaf) ? i + 1u : mesh_bits(a.w);
    }
    return best;
}

// whether the ray meets the box [lo, hi] at some t in [0, best]
__host__ __device__ __forceinline__ bool ray_box_reach(const float lo[3], const float hi[3], float ox, float oy, float oz, float dx, float dy,
                                                       float dz, float best) {
#pragma clang fp contract(off)
    float t0 = 0.0f, t1 = best;
    bool on = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float o = a == 0 ? ox : (a == 1 ? oy : oz), d = a == 0 ? dx : (a == 1 ? dy : dz);
        if (d == 0.0f) {
            on = on && o >= lo[a] && o <= hi[a];
        } else {
            const float u = (lo[a] - o) / d, v = (hi[a] - o) / d;
            t0 = fmaxf(t0, fminf(u, v)); t1 = fminf(t1, fmaxf(u, v));
        }
    }
    return on && t0 <= t1;
}

// parry's Compound::cast_local_ray, solid = false, in the compound's frame (see the head of this file).  PRUNE: a part whose loosened
// box the ray misses within [0, best] is left out; the result is the walk over all parts bit for bit.
template <bool PRUNE>
__host__ __device__ __forceinline__ float compound_cast_ray(const CompoundPartDev* __restrict__ parts, uint32_t nparts, float ox, float oy,
                                                            float oz, float dx, float dy, float dz) {
#pragma clang fp contract(off)
    float best = __builtin_inff();
#pragma unroll 1
    for (uint32_t k = 0; k < nparts; ++k) {
        const CompoundPartDev& P = parts[k];
        if (PRUNE && !ray_box_reach(P.lo, P.hi, ox, oy, oz, dx, dy, dz, best)) continue;
        float lx, ly, lz, ex, ey, ez;
        quat_rot(-P.q[0], -P.q[1], -P.q[2], P.q[3], ox - P.t[0], oy - P.t[1], oz - P.t[2], lx, ly, lz);
        quat_rot(-P.q[0], -P.q[1], -P.q[2], P.q[3], dx, dy, dz, ex, ey, ez);
        if (P.kind == SALVA_HIP_SHAPE_MESH) {
            best = mesh_cast_ray(P.mesh, lx, ly, lz, ex, ey, ez, best);
        } else {
            const float t = shape_cast_ray(P, lx, ly, lz, ex, ey, ez);
            if (t < best) best = t;  // (strict: equal t from two parts is one hit)
        }
    }
    return best;
}
#endif  // __HIPCC__

}  // namespace salva

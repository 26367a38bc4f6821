// mesh.h — a device-resident triangle mesh (mesh.hip): vertices, triangles in the leaf order of a bounding volume hierarchy, the
// hierarchy in depth-first order with one skip index per node, and — for a closed, consistently wound mesh — the pseudo-normals of
// its faces, edges and vertices.  DESIGN.md §14.  The device functions below are the two pieces of geometry the ray sampler
// (sample.hip, k_sample_mesh_mark) and DynamicContactSampling (dcs.hip, k_dcs_project_mesh) need: the next hit of an axis-parallel
// ray and the closest point.  Both walk the hierarchy without a stack — next = hit ? i + 1 : skip[i] — and both give exactly what a
// pass over all triangles gives: a node is left out only when no triangle in its (loosened) box can change the answer.
#pragma once
#include <memory>
#include <vector>

#include "common.h"

namespace salva {

struct MeshDev {
    const float4* verts;      // (x, y, z, 0) per vertex
    const uint4* tris;        // leaf order: (i0, i1, i2, the triangle's index as the caller gave it)
    const float4* nodes;      // two per node: (box mins, skip index), (box maxs, leaf ? first << 3 | count : 0)
    uint32_t nnodes, oriented;
    const uint4* tri_edges;   // oriented meshes, leaf order: the mesh edge behind (i0 i1, i1 i2, i2 i0)
    const float4 *fn, *en, *vn;  // pseudo-normals: per triangle (leaf order), per mesh edge, per vertex
};

struct MeshRes {
    uint32_t nv = 0, nt = 0, nnodes = 0, flags = 0;
    float mins[3] = {0, 0, 0}, maxs[3] = {0, 0, 0};  // min / max over the vertices
    DevBuf<float4> verts, nodes, fn, en, vn;
    DevBuf<uint4> tris, tri_edges;
    MeshDev dev() const {
        return MeshDev{verts.p, tris.p, nodes.p, nnodes, (flags & 1u) ? 1u : 0u, tri_edges.p, fn.p, en.p, vn.p};
    }
};

// validates, builds the hierarchy (median split on the longest axis, leaves of at most 4 triangles) and the pseudo-normals (f64),
// uploads on `stream` and waits
std::shared_ptr<MeshRes> mesh_build(const float* vertices_xyz, uint32_t nv, const uint32_t* indices, uint32_t nt, uint32_t flags,
                                    hipStream_t stream);
// the host half of it: triangles in leaf order (`order[s]` = the caller's index of the triangle in slot s), nodes, `tris` as MeshDev reads them
void mesh_build_hierarchy(const float* vertices_xyz, uint32_t nv, const uint32_t* indices, uint32_t nt, std::vector<uint32_t>& order,
                          std::vector<float4>& nodes, std::vector<uint4>& tris);
// parry 0.18 HeightField's vertices and triangles
void heightfield_triangles(const float* heights, uint32_t nrows, uint32_t ncols, const float scale[3], std::vector<float>& vertices,
                           std::vector<uint32_t>& indices);

#ifdef __HIPCC__
constexpr int MESH_MAX_HITS = 64;  // accepted hits per ray (the host arm's bound on its rounds)

__host__ __device__ __forceinline__ uint32_t mesh_bits(float v) { return __builtin_bit_cast(uint32_t, v); }

template <typename T>
__host__ __device__ __forceinline__ T mesh_sel3(int a, T x, T y, T z) { return a == 0 ? x : (a == 1 ? y : z); }

// the edge function of c against a -> b in the (j, k) plane, the endpoints taken in the order of their vertex indices: the two
// triangles of a shared edge compute the same number with opposite sign
__host__ __device__ __forceinline__ float mesh_edge(uint32_t ia, uint32_t ib, float aj, float ak, float bj, float bk, float cj, float ck) {
#pragma clang fp contract(off)
    if (ia < ib) return ((bj - aj) * (ck - ak)) - ((bk - ak) * (cj - aj));
    return -(((aj - bj) * (ck - bk)) - ((ak - bk) * (cj - bj)));
}

// The smallest hit coordinate >= o of the ray along +axis through (cj, ck) — j = axis + 1, k = axis + 2 mod 3; +inf: none.
__host__ __device__ __forceinline__ float mesh_next_hit(const MeshDev& m, int axis, float cj, float ck, float o) {
#pragma clang fp contract(off)
    float best = __builtin_inff();
    uint32_t i = 0;
    while (i < m.nnodes) {
        const float4 a = m.nodes[2 * i], b = m.nodes[2 * i + 1];
        const uint32_t leaf = mesh_bits(b.w);
        const bool in = cj >= mesh_sel3(axis, a.y, a.z, a.x) && cj <= mesh_sel3(axis, b.y, b.z, b.x) && ck >= mesh_sel3(axis, a.z, a.x, a.y) &&
                        ck <= mesh_sel3(axis, b.z, b.x, b.y) && mesh_sel3(axis, b.x, b.y, b.z) >= o && mesh_sel3(axis, a.x, a.y, a.z) <= best;
        if (in && leaf) {
            const uint32_t first = leaf >> 3, end = first + (leaf & 7u);
            for (uint32_t t = first; t < end; ++t) {
                const uint4 tr = m.tris[t];
                const float4 v0 = m.verts[tr.x], v1 = m.verts[tr.y], v2 = m.verts[tr.z];
                const float j0 = mesh_sel3(axis, v0.y, v0.z, v0.x), k0 = mesh_sel3(axis, v0.z, v0.x, v0.y);
                const float j1 = mesh_sel3(axis, v1.y, v1.z, v1.x), k1 = mesh_sel3(axis, v1.z, v1.x, v1.y);
                const float j2 = mesh_sel3(axis, v2.y, v2.z, v2.x), k2 = mesh_sel3(axis, v2.z, v2.x, v2.y);
                // e_k: the edge opposite vertex k
                const float e0 = mesh_edge(tr.y, tr.z, j1, k1, j2, k2, cj, ck), e1 = mesh_edge(tr.z, tr.x, j2, k2, j0, k0, cj, ck),
                            e2 = mesh_edge(tr.x, tr.y, j0, k0, j1, k1, cj, ck);
                const float sum = (e0 + e1) + e2;
                const bool hit = ((e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) || (e0 <= 0.0f && e1 <= 0.0f && e2 <= 0.0f)) && sum != 0.0f;
                if (!hit) continue;
                const float x0 = mesh_sel3(axis, v0.x, v0.y, v0.z), x1 = mesh_sel3(axis, v1.x, v1.y, v1.z), x2 = mesh_sel3(axis, v2.x, v2.y, v2.z);
                const float h = (((e0 * x0) + (e1 * x1)) + (e2 * x2)) / sum;
                if (h >= o && h < best) best = h;
            }
        }
        i = (in && !leaf) ? i + 1u : mesh_bits(a.w);
    }
    return best;
}

__host__ __device__ __forceinline__ float mesh_dot(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    return ((ax * bx) + (ay * by)) + (az * bz);
}

// Ericson's ClosestPtPointTriangle (Real-Time Collision Detection §5.1.5), f32; `feat`: 0 1 2 = vertex a b c, 3 4 5 = edge ab ac bc,
// 6 = face
__host__ __device__ __forceinline__ void mesh_closest_on_triangle(float px, float py, float pz, const float4& a, const float4& b, const float4& c,
                                                         float& ox, float& oy, float& oz, uint32_t& feat) {
#pragma clang fp contract(off)
    const float abx = b.x - a.x, aby = b.y - a.y, abz = b.z - a.z, acx = c.x - a.x, acy = c.y - a.y, acz = c.z - a.z;
    const float apx = px - a.x, apy = py - a.y, apz = pz - a.z;
    const float d1 = mesh_dot(abx, aby, abz, apx, apy, apz), d2 = mesh_dot(acx, acy, acz, apx, apy, apz);
    if (d1 <= 0.0f && d2 <= 0.0f) { ox = a.x; oy = a.y; oz = a.z; feat = 0u; return; }
    const float bpx = px - b.x, bpy = py - b.y, bpz = pz - b.z;
    const float d3 = mesh_dot(abx, aby, abz, bpx, bpy, bpz), d4 = mesh_dot(acx, acy, acz, bpx, bpy, bpz);
    if (d3 >= 0.0f && d4 <= d3) { ox = b.x; oy = b.y; oz = b.z; feat = 1u; return; }
    const float vc = (d1 * d4) - (d3 * d2);
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        const float v = d1 / (d1 - d3);
        ox = a.x + (abx * v); oy = a.y + (aby * v); oz = a.z + (abz * v); feat = 3u;
        return;
    }
    const float cpx = px - c.x, cpy = py - c.y, cpz = pz - c.z;
    const float d5 = mesh_dot(abx, aby, abz, cpx, cpy, cpz), d6 = mesh_dot(acx, acy, acz, cpx, cpy, cpz);
    if (d6 >= 0.0f && d5 <= d6) { ox = c.x; oy = c.y; oz = c.z; feat = 2u; return; }
    const float vb = (d5 * d2) - (d1 * d6);
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        const float w = d2 / (d2 - d6);
        ox = a.x + (acx * w); oy = a.y + (acy * w); oz = a.z + (acz * w); feat = 4u;
        return;
    }
    const float va = (d3 * d6) - (d5 * d4);
    if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {
        const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        ox = b.x + ((c.x - b.x) * w); oy = b.y + ((c.y - b.y) * w); oz = b.z + ((c.z - b.z) * w); feat = 5u;
        return;
    }
    const float denom = 1.0f / ((va + vb) + vc);
    const float v = vb * denom, w = vc * denom;
    ox = (a.x + (abx * v)) + (acx * w); oy = (a.y + (aby * v)) + (acy * w); oz = (a.z + (abz * v)) + (acz * w); feat = 6u;
}

// The closest point of the mesh to p (smallest squared distance, ties to the lowest triangle index) and, for an oriented mesh,
// whether p lies inside: dot(p - closest, pseudo-normal of the closest feature) <= 0.
__host__ __device__ __forceinline__ void mesh_project_point(const MeshDev& m, float px, float py, float pz, float& ox, float& oy, float& oz, bool& inside) {
#pragma clang fp contract(off)
    float best = __builtin_inff();
    uint32_t best_tri = 0xffffffffu, best_slot = 0u, best_feat = 6u;
    ox = px; oy = py; oz = pz;
    uint32_t i = 0;
    while (i < m.nnodes) {
        const float4 a = m.nodes[2 * i], b = m.nodes[2 * i + 1];
        const uint32_t leaf = mesh_bits(b.w);
        const float dx = fmaxf(fmaxf(a.x - px, 0.0f), px - b.x), dy = fmaxf(fmaxf(a.y - py, 0.0f), py - b.y), dz = fmaxf(fmaxf(a.z - pz, 0.0f), pz - b.z);
        // (the factor keeps the comparison on the safe side of the rounding of both squared distances)
        const bool in = !((((dx * dx) + (dy * dy)) + (dz * dz)) * 0.999999f > best);
        if (in && leaf) {
            const uint32_t first = leaf >> 3, end = first + (leaf & 7u);
            for (uint32_t t = first; t < end; ++t) {
                const uint4 tr = m.tris[t];
                float cx, cy, cz;
                uint32_t feat;
                mesh_closest_on_triangle(px, py, pz, m.verts[tr.x], m.verts[tr.y], m.verts[tr.z], cx, cy, cz, feat);
                const float ex = px - cx, ey = py - cy, ez = pz - cz;
                const float d = mesh_dot(ex, ey, ez, ex, ey, ez);
                if (d < best || (d == best && tr.w < best_tri)) {
                    best = d; best_tri = tr.w; best_slot = t; best_feat = feat;
                    ox = cx; oy = cy; oz = cz;
                }
            }
        }
        i = (in && !leaf) ? i + 1u : mesh_bits(a.w);
    }
    inside = false;
    if (m.oriented && best_tri != 0xffffffffu) {
        float4 n;
        if (best_feat == 6u) {
            n = m.fn[best_slot];
        } else if (best_feat < 3u) {
            const uint4 tr = m.tris[best_slot];
            n = m.vn[mesh_sel3((int)best_feat, tr.x, tr.y, tr.z)];
        } else {
            const uint4 te = m.tri_edges[best_slot];  // (ab, bc, ca)
            n = m.en[best_feat == 3u ? te.x : (best_feat == 4u ? te.z : te.y)];
        }
        inside = mesh_dot(px - ox, py - oy, pz - oz, n.x, n.y, n.z) <= 0.0f;
    }
}
#endif  // __HIPCC__

}  // namespace salva

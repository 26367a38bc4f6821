// mesh.hip — the host side of a device-resident triangle mesh (mesh.h): validation, the bounding volume hierarchy,
// the pseudo-normals, parry's height field as triangles, and the world's mesh table.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <numeric>

#include "mesh.h"
#include "world.h"

namespace salva {

namespace {

struct Box { float lo[3], hi[3]; };

struct BvhBuilder {
    const std::vector<Box>& tb;           // per triangle
    const std::vector<float>& centroid;   // 3 per triangle
    std::vector<uint32_t> order;          // triangles, permuted in place into leaf order
    std::vector<float4> nodes;            // two per node (mesh.h)
    float margin;

    // the subtree over order[first, first + count), depth first; returns nothing: a node's skip index is the node count after it
    void build(uint32_t first, uint32_t count) {
        Box b{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
        for (uint32_t k = first; k < first + count; ++k)
            for (int a = 0; a < 3; ++a) {
                b.lo[a] = std::min(b.lo[a], tb[order[k]].lo[a]);
                b.hi[a] = std::max(b.hi[a], tb[order[k]].hi[a]);
            }
        const size_t me = nodes.size();
        nodes.push_back(make_float4(b.lo[0] - margin, b.lo[1] - margin, b.lo[2] - margin, 0.0f));
        nodes.push_back(make_float4(b.hi[0] + margin, b.hi[1] + margin, b.hi[2] + margin, 0.0f));
        if (count <= 4) {
            const uint32_t leaf = first << 3 | count;
            std::memcpy(&nodes[me + 1].w, &leaf, 4);
        } else {
            int axis = 0;
            for (int a = 1; a < 3; ++a)
                if (b.hi[a] - b.lo[a] > b.hi[axis] - b.lo[axis]) axis = a;
            const uint32_t half = count / 2;
            auto less = [&](uint32_t x, uint32_t y) {
                const float cx = centroid[3 * (size_t)x + axis], cy = centroid[3 * (size_t)y + axis];
                return cx < cy || (cx == cy && x < y);
            };
            std::nth_element(order.begin() + first, order.begin() + first + half, order.begin() + first + count, less);
            build(first, half);
            build(first + half, count - half);
        }
        const uint32_t skip = (uint32_t)(nodes.size() / 2);
        std::memcpy(&nodes[me].w, &skip, 4);
    }
};

template <typename T>
void upload(DevBuf<T>& d, const std::vector<T>& h, hipStream_t stream) {
    d.ensure(std::max<size_t>(h.size(), 1));
    if (!h.empty()) SALVA_HIP_CHECK(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, stream));
}

float4 as_f4(const double v[3]) { return make_float4((float)v[0], (float)v[1], (float)v[2], 0.0f); }

}  // namespace

// Median split (nth_element on the centroid, ties by triangle index) along the longest axis of the node's box, leaves of at most 4
// triangles, nodes depth first.  Boxes are loosened by 2^-18 of the largest coordinate (64 ulp of it): a closest point or a hit
// coordinate is a rounded combination of a triangle's vertices and may leave their exact box by an ulp or two.
void mesh_build_hierarchy(const float* v, uint32_t nv, const uint32_t* idx, uint32_t nt, std::vector<uint32_t>& order,
                          std::vector<float4>& nodes, std::vector<uint4>& tris) {
    float maxabs = 0.0f;
    for (size_t k = 0; k < 3 * (size_t)nv; ++k) maxabs = std::max(maxabs, std::fabs(v[k]));
    std::vector<Box> tb(nt);
    std::vector<float> centroid(3 * (size_t)nt);
    for (uint32_t t = 0; t < nt; ++t)
        for (int a = 0; a < 3; ++a) {
            const float x0 = v[3 * (size_t)idx[3 * (size_t)t] + a], x1 = v[3 * (size_t)idx[3 * (size_t)t + 1] + a], x2 = v[3 * (size_t)idx[3 * (size_t)t + 2] + a];
            tb[t].lo[a] = std::min(x0, std::min(x1, x2));
            tb[t].hi[a] = std::max(x0, std::max(x1, x2));
            centroid[3 * (size_t)t + a] = (float)(((double)x0 + x1 + x2) / 3.0);
        }
    BvhBuilder bb{tb, centroid, {}, {}, std::max(maxabs * 3.814697265625e-6f, 1e-30f)};
    bb.order.resize(nt);
    std::iota(bb.order.begin(), bb.order.end(), 0u);
    bb.nodes.reserve(4 * (size_t)nt / 3 + 8);
    bb.build(0, nt);
    tris.resize(nt);
    for (uint32_t s = 0; s < nt; ++s) {
        const uint32_t t = bb.order[s];
        tris[s] = make_uint4(idx[3 * (size_t)t], idx[3 * (size_t)t + 1], idx[3 * (size_t)t + 2], t);
    }
    order = std::move(bb.order);
    nodes = std::move(bb.nodes);
}

std::shared_ptr<MeshRes> mesh_build(const float* v, uint32_t nv, const uint32_t* idx, uint32_t nt, uint32_t flags, hipStream_t stream) {
    if (!v || !idx) throw HipError(SALVA_HIP_E_INVALID, "mesh: null vertices or indices");
    if (nt == 0 || nv == 0) throw HipError(SALVA_HIP_E_INVALID, "mesh: no triangles");
    if (nt >= (1u << 29)) throw HipError(SALVA_HIP_E_CAPACITY, "mesh: more than 2^29 triangles");
    if (flags & ~(uint32_t)SALVA_HIP_MESH_ORIENTED) throw HipError(SALVA_HIP_E_INVALID, "mesh: unknown flags");
    for (size_t k = 0; k < 3 * (size_t)nv; ++k)
        if (!std::isfinite(v[k])) throw HipError(SALVA_HIP_E_INVALID, "mesh: a vertex coordinate is infinite or NaN");
    for (size_t k = 0; k < 3 * (size_t)nt; ++k)
        if (idx[k] >= nv) throw HipError(SALVA_HIP_E_INVALID, "mesh: a triangle names a vertex past the end of the vertex array");

    auto m = std::make_shared<MeshRes>();
    m->nv = nv; m->nt = nt; m->flags = flags;
    for (int a = 0; a < 3; ++a) { m->mins[a] = INFINITY; m->maxs[a] = -INFINITY; }
    std::vector<float4> verts(nv);
    for (uint32_t k = 0; k < nv; ++k) {
        verts[k] = make_float4(v[3 * (size_t)k], v[3 * (size_t)k + 1], v[3 * (size_t)k + 2], 0.0f);
        for (int a = 0; a < 3; ++a) {
            const float c = v[3 * (size_t)k + a];
            m->mins[a] = std::min(m->mins[a], c); m->maxs[a] = std::max(m->maxs[a], c);
        }
    }

    // ---- the hierarchy
    std::vector<uint32_t> order;
    std::vector<float4> nodes;
    std::vector<uint4> tris;
    mesh_build_hierarchy(v, nv, idx, nt, order, nodes, tris);
    m->nnodes = (uint32_t)(nodes.size() / 2);
    upload(m->verts, verts, stream);
    upload(m->nodes, nodes, stream);
    upload(m->tris, tris, stream);

    // ---- pseudo-normals (Baerentzen & Aanaes 2005) in f64, stored as f32: the face normal; per mesh edge the sum of the unit
    // normals of the faces at it; per vertex the sum of the unit normals of the faces around it, each weighted by its angle there
    std::vector<float4> fn, en, vn;
    std::vector<uint4> tri_edges;
    if (flags & SALVA_HIP_MESH_ORIENTED) {
        std::vector<double> fnd(3 * (size_t)nt, 0.0), vnd(3 * (size_t)nv, 0.0), end_;
        std::map<std::pair<uint32_t, uint32_t>, uint32_t> edge_id;  // ids in the order the edges first appear, triangle by triangle
        std::vector<uint32_t> te(3 * (size_t)nt);
        for (uint32_t t = 0; t < nt; ++t) {
            const uint32_t i3[3] = {idx[3 * (size_t)t], idx[3 * (size_t)t + 1], idx[3 * (size_t)t + 2]};
            double p[3][3];
            for (int c = 0; c < 3; ++c)
                for (int a = 0; a < 3; ++a) p[c][a] = (double)v[3 * (size_t)i3[c] + a];
            double ab[3], ac[3], nrm[3];
            for (int a = 0; a < 3; ++a) { ab[a] = p[1][a] - p[0][a]; ac[a] = p[2][a] - p[0][a]; }
            nrm[0] = ab[1] * ac[2] - ab[2] * ac[1]; nrm[1] = ab[2] * ac[0] - ab[0] * ac[2]; nrm[2] = ab[0] * ac[1] - ab[1] * ac[0];
            const double len = std::sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
            for (int a = 0; a < 3; ++a) nrm[a] = len > 0.0 ? nrm[a] / len : 0.0;  // (a degenerate face adds nothing)
            for (int a = 0; a < 3; ++a) fnd[3 * (size_t)t + a] = nrm[a];
            for (int c = 0; c < 3; ++c) {
                const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                double e1[3], e2[3], cr[3];
                for (int a = 0; a < 3; ++a) { e1[a] = p[c1][a] - p[c][a]; e2[a] = p[c2][a] - p[c][a]; }
                cr[0] = e1[1] * e2[2] - e1[2] * e2[1]; cr[1] = e1[2] * e2[0] - e1[0] * e2[2]; cr[2] = e1[0] * e2[1] - e1[1] * e2[0];
                const double angle = std::atan2(std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]), e1[0] * e2[0] + e1[1] * e2[1] + e1[2] * e2[2]);
                for (int a = 0; a < 3; ++a) vnd[3 * (size_t)i3[c] + a] += angle * nrm[a];
                const std::pair<uint32_t, uint32_t> key(std::min(i3[c], i3[c1]), std::max(i3[c], i3[c1]));
                auto it = edge_id.find(key);
                if (it == edge_id.end()) {
                    it = edge_id.emplace(key, (uint32_t)(end_.size() / 3)).first;
                    end_.insert(end_.end(), {0.0, 0.0, 0.0});
                }
                te[3 * (size_t)t + c] = it->second;
                for (int a = 0; a < 3; ++a) end_[3 * (size_t)it->second + a] += nrm[a];
            }
        }
        fn.resize(nt); tri_edges.resize(nt);
        for (uint32_t s = 0; s < nt; ++s) {
            const uint32_t t = order[s];
            fn[s] = as_f4(&fnd[3 * (size_t)t]);
            tri_edges[s] = make_uint4(te[3 * (size_t)t], te[3 * (size_t)t + 1], te[3 * (size_t)t + 2], 0u);
        }
        vn.resize(nv);
        for (uint32_t k = 0; k < nv; ++k) vn[k] = as_f4(&vnd[3 * (size_t)k]);
        en.resize(end_.size() / 3);
        for (size_t k = 0; k < en.size(); ++k) en[k] = as_f4(&end_[3 * k]);
    }
    upload(m->fn, fn, stream); upload(m->en, en, stream); upload(m->vn, vn, stream); upload(m->tri_edges, tri_edges, stream);
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));  // (the host vectors leave scope)
    return m;
}

void heightfield_triangles(const float* heights, uint32_t nrows, uint32_t ncols, const float scale[3], std::vector<float>& vertices,
                           std::vector<uint32_t>& indices) {
    if (!heights || !scale) throw HipError(SALVA_HIP_E_INVALID, "height field: null argument");
    if (nrows < 2 || ncols < 2) throw HipError(SALVA_HIP_E_INVALID, "height field: at least 2 x 2 heights");
    if ((uint64_t)(nrows - 1) * (ncols - 1) * 2 >= (1ull << 29)) throw HipError(SALVA_HIP_E_CAPACITY, "height field: more than 2^29 triangles");
    vertices.resize(3 * (size_t)nrows * ncols);
    for (uint32_t i = 0; i < nrows; ++i)
        for (uint32_t j = 0; j < ncols; ++j) {
            float* p = &vertices[3 * ((size_t)i * ncols + j)];
            p[0] = ((float)j / (float)(ncols - 1) - 0.5f) * scale[0];
            p[1] = heights[(size_t)i * ncols + j] * scale[1];
            p[2] = ((float)i / (float)(nrows - 1) - 0.5f) * scale[2];
        }
    indices.clear();
    indices.reserve(6 * (size_t)(nrows - 1) * (ncols - 1));
    for (uint32_t i = 0; i + 1 < nrows; ++i)
        for (uint32_t j = 0; j + 1 < ncols; ++j) {
            const uint32_t p00 = i * ncols + j, p01 = p00 + 1, p10 = p00 + ncols, p11 = p10 + 1;
            indices.insert(indices.end(), {p00, p10, p11, p00, p11, p01});
        }
}

// ------------------------------------------------------------------------------------------------ the world's mesh table
uint32_t World::create_mesh(const float* vertices_xyz, uint32_t nv, const uint32_t* indices, uint32_t nt, uint32_t flags) {
    use_device();
    std::shared_ptr<MeshRes> m = mesh_build(vertices_xyz, nv, indices, nt, flags, stream);
    for (uint32_t k = 0; k < meshes.size(); ++k)
        if (!meshes[k]) { meshes[k] = m; return k; }
    meshes.push_back(m);
    return (uint32_t)meshes.size() - 1;
}

uint32_t World::create_heightfield(const float* heights, uint32_t nrows, uint32_t ncols, const float scale[3]) {
    std::vector<float> vertices;
    std::vector<uint32_t> indices;
    heightfield_triangles(heights, nrows, ncols, scale, vertices, indices);
    return create_mesh(vertices.data(), nrows * ncols, indices.data(), (uint32_t)(indices.size() / 3), 0u);  // never oriented
}

const std::shared_ptr<MeshRes>& World::mesh_at(uint32_t mesh) const {
    if (mesh >= meshes.size() || !meshes[mesh]) throw HipError(SALVA_HIP_E_INVALID, "no such mesh");
    return meshes[mesh];
}

void World::destroy_mesh(uint32_t mesh) {
    use_device();
    if (mesh_at(mesh).use_count() > 1)
        throw HipError(SALVA_HIP_E_INVALID, "the mesh is the collider of a dynamically sampled boundary (salva_hip_clear_boundary_sampling releases it) or a part of a compound (salva_hip_destroy_compound releases it), or the region of a sink (salva_hip_remove_sink releases it)");
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    meshes[mesh].reset();
}

}  // namespace salva

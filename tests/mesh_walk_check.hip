// mesh_walk_check.hip — a stand-alone host program (tests/test_mesh_walk_cpu.py builds and runs it, no GPU): the stackless walks of
// salva_amd/csrc/mesh.h over the hierarchy mesh_build_hierarchy makes, against the same per-triangle code run over ALL triangles (a
// flat list of one-triangle leaves with infinite boxes), bit for bit — casts along all three axes with the sampler's origin sequence,
// and closest points, on height fields and on random triangle soups.  Prints the number of differences; exit status 1 if any.
#include <cstdio>
#include <cstring>
#include <random>

#include "mesh.h"

using namespace salva;

struct HostMesh {
    std::vector<float4> verts, nodes;
    std::vector<uint4> tris;
    MeshDev dev() const { return MeshDev{verts.data(), tris.data(), nodes.data(), (uint32_t)(nodes.size() / 2), 0u, nullptr, nullptr, nullptr, nullptr}; }
};

static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int main() {
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    int bad = 0, deepest = 0;
    for (int trial = 0; trial < 6; ++trial) {
        std::vector<float> v;
        std::vector<uint32_t> idx;
        if (trial < 3) {
            const uint32_t n = trial == 0 ? 5 : (trial == 1 ? 9 : 41);
            std::vector<float> h(n * n);
            for (float& x : h) x = U(rng);
            const float scale[3] = {1.1f, 0.25f, 0.9f};
            heightfield_triangles(h.data(), n, n, scale, v, idx);
        } else {
            const uint32_t nv = 60 * trial, nt = 100 * trial;
            for (uint32_t k = 0; k < 3 * nv; ++k) v.push_back(U(rng) * 2.0f - 1.0f);
            for (uint32_t k = 0; k < 3 * nt; ++k) idx.push_back(rng() % nv);
        }
        const uint32_t nv = (uint32_t)(v.size() / 3), nt = (uint32_t)(idx.size() / 3);
        HostMesh m;
        for (uint32_t k = 0; k < nv; ++k) m.verts.push_back(make_float4(v[3 * k], v[3 * k + 1], v[3 * k + 2], 0.0f));
        std::vector<uint32_t> order;
        mesh_build_hierarchy(v.data(), nv, idx.data(), nt, order, m.nodes, m.tris);
        HostMesh flat = m;
        flat.nodes.clear();
        for (uint32_t t = 0; t < nt; ++t) {
            const uint32_t skip = t + 1, leaf = t << 3 | 1u;
            float fs, fl;
            std::memcpy(&fs, &skip, 4); std::memcpy(&fl, &leaf, 4);
            flat.nodes.push_back(make_float4(-INFINITY, -INFINITY, -INFINITY, fs));
            flat.nodes.push_back(make_float4(INFINITY, INFINITY, INFINITY, fl));
        }
        // shape of the hierarchy: every leaf holds 1..4 triangles, every skip index points forward, the leaves cover [0, nt) in order
        uint32_t covered = 0;
        const uint32_t nn = (uint32_t)(m.nodes.size() / 2);
        for (uint32_t i = 0; i < nn; ++i) {
            const uint32_t skip = mesh_bits(m.nodes[2 * i].w), leaf = mesh_bits(m.nodes[2 * i + 1].w);
            if (skip <= i || skip > nn) ++bad;
            if (leaf) {
                if ((leaf >> 3) != covered || (leaf & 7u) == 0 || (leaf & 7u) > 4 || skip != i + 1) ++bad;
                covered += leaf & 7u;
            }
        }
        if (covered != nt) ++bad;
        int depth = 0;
        for (uint32_t k = nn; k > 1; k >>= 1) ++depth;
        deepest = depth > deepest ? depth : deepest;
        const MeshDev a = m.dev(), b = flat.dev();
        for (int r = 0; r < 6000; ++r) {
            const int axis = r % 3;
            const float cj = U(rng) * 2.4f - 1.2f, ck = U(rng) * 2.4f - 1.2f;
            float o = -3.0f;
            for (int hits = 0; hits < 70; ++hits) {
                const float ha = mesh_next_hit(a, axis, cj, ck, o), hb = mesh_next_hit(b, axis, cj, ck, o);
                if (!same(ha, hb) && bad++ < 10) printf("cast differs: trial %d axis %d (%g, %g) from %g: %g against %g\n", trial, axis, cj, ck, o, ha, hb);
                if (!(hb < INFINITY)) break;
                o = o + ((hb - o) + 0.004f);
            }
            float p[3] = {U(rng) * 3.0f - 1.5f, U(rng) * 3.0f - 1.5f, U(rng) * 3.0f - 1.5f};
            if (r % 4 == 0) {  // next to a vertex: many triangles at nearly the same distance
                const float4 q = m.verts[rng() % nv];
                p[0] = q.x + (U(rng) - 0.5f) * 1e-3f; p[1] = q.y + (U(rng) - 0.5f) * 1e-3f; p[2] = q.z;
            }
            float ax, ay, az, bx, by, bz;
            bool ia, ib;
            mesh_project_point(a, p[0], p[1], p[2], ax, ay, az, ia);
            mesh_project_point(b, p[0], p[1], p[2], bx, by, bz, ib);
            if (!(same(ax, bx) && same(ay, by) && same(az, bz)) && bad++ < 10) printf("projection differs: trial %d at (%g, %g, %g)\n", trial, p[0], p[1], p[2]);
        }
    }
    printf("deepest hierarchy: %d levels; differences: %d\n", deepest, bad);
    return bad != 0;
}

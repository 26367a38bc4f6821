// compound_walk_check.hip — a stand-alone host program (tests/test_compound_cpu.py builds and runs it, no GPU): the walk over a
// compound's parts of salva_amd/csrc/compound.h with its box pruning against the same walk over ALL parts, bit for bit, on the table
// the library's own compound_build_table makes — a compound whose parts lie far apart, so that most parts are left out for most
// points, and one whose parts overlap.  Prints how many parts the walk left out behind the winner and the number of
// differences; exit status 1 if any, or if nothing was left out.
#include <cstdio>
#include <cstring>
#include <random>

#include "compound.h"

using namespace salva;

static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static SalvaHipCompoundPart part(int kind, float p0, float p1, float p2, float tx, float ty, float tz, float ax, float ay, float az) {
    SalvaHipCompoundPart c{};
    c.kind = kind;
    c.params[0] = p0; c.params[1] = p1; c.params[2] = p2;
    c.translation[0] = tx; c.translation[1] = ty; c.translation[2] = tz;
    const float ang = std::sqrt(ax * ax + ay * ay + az * az);
    const float s = ang > 0.0f ? std::sin(0.5f * ang) / ang : 0.0f;
    c.rotation_ijkw[0] = ax * s; c.rotation_ijkw[1] = ay * s; c.rotation_ijkw[2] = az * s; c.rotation_ijkw[3] = std::cos(0.5f * ang);
    return c;
}

int main() {
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    int bad = 0;
    long visits = 0, pruned = 0;
    for (int trial = 0; trial < 2; ++trial) {
        const float spread = trial == 0 ? 0.45f : 0.05f;  // far apart / overlapping
        std::vector<SalvaHipCompoundPart> parts = {
            part(SALVA_HIP_SHAPE_BALL, 0.06f, 0, 0, -spread, 0, 0, 0, 0, 0),
            part(SALVA_HIP_SHAPE_CUBOID, 0.05f, 0.07f, 0.04f, 0, 0.9f * spread, 0, 0.3f, 0.2f, -0.4f),
            part(SALVA_HIP_SHAPE_CAPSULE, 0.06f, 0.04f, 0, spread, 0, 0.1f, 0, 0, 1.2f),
            part(SALVA_HIP_SHAPE_CYLINDER, 0.05f, 0.06f, 0, 0, -0.9f * spread, -0.1f, 0.7f, 0, 0.1f),
            part(SALVA_HIP_SHAPE_BALL, 0.05f, 0, 0, 0.05f, 0, spread, 0, 0, 0),
            part(SALVA_HIP_SHAPE_BALL, 0.05f, 0, 0, 0.05f, 0, spread, 0, 0, 0),  // (a twin: every point ties between the two)
        };
        std::vector<CompoundPartDev> table;
        float mins[3], maxs[3];
        compound_build_table(parts.data(), (uint32_t)parts.size(), std::vector<const MeshRes*>(parts.size(), nullptr), table, mins, maxs);
        for (int r = 0; r < 40000; ++r) {
            float p[3];
            for (int a = 0; a < 3; ++a) p[a] = mins[a] - 0.2f + U(rng) * (maxs[a] - mins[a] + 0.4f);
            if (r % 5 == 0) {  // near a part's centre: deep inside it
                const CompoundPartDev& P = table[rng() % table.size()];
                for (int a = 0; a < 3; ++a) p[a] = P.t[a] + (U(rng) - 0.5f) * 0.02f;
            }
            float ax, ay, az, bx, by, bz;
            bool ia, ib;
            compound_project_local<true>(table.data(), (uint32_t)table.size(), p[0], p[1], p[2], ax, ay, az, ia);
            compound_project_local<false>(table.data(), (uint32_t)table.size(), p[0], p[1], p[2], bx, by, bz, ib);
            if (!(same(ax, bx) && same(ay, by) && same(az, bz) && ia == ib) && bad++ < 10)
                printf("projection differs: trial %d at (%g, %g, %g): (%g, %g, %g) %d against (%g, %g, %g) %d\n", trial, p[0], p[1], p[2], ax, ay, az,
                       (int)ia, bx, by, bz, (int)ib);
            // The skips the walk certainly took: the winner is the first part whose own projection is the result; from there on `best`
            // is final, so every later part whose box test fails against it was left out by compound_project_local<true>.
            uint32_t winner = (uint32_t)table.size();
            for (uint32_t k = 0; k < table.size() && winner == table.size(); ++k) {
                float cx, cy, cz;
                bool ik;
                compound_project_local<false>(table.data() + k, 1u, p[0], p[1], p[2], cx, cy, cz, ik);
                if (same(cx, bx) && same(cy, by) && same(cz, bz)) winner = k;
            }
            if (winner == table.size()) { ++bad; continue; }
            const float dx = p[0] - bx, dy = p[1] - by, dz = p[2] - bz, best = ((dx * dx) + (dy * dy)) + (dz * dz);
            for (uint32_t k = 0; k < table.size(); ++k) {
                ++visits;
                if (k > winner && compound_box_d2(table[k], p[0], p[1], p[2]) * 0.999999f > best) ++pruned;
            }
        }
    }
    printf("part visits: %ld, of them left out behind the winner: %ld; differences: %d\n", visits, pruned, bad);
    return bad != 0 || pruned == 0;
}

// compound_host_arm.hip — the host arm's two callbacks for a compound collider, in C++ (tools/coupling_bench.py --shape compound
// --host): what a rapier user's binding does per step for a parry `Compound` when the library has no device code for it.  The
// geometry is the library's own walk (salva_amd/csrc/compound.h is `__host__ __device__`) run on the host, one point after the other.
//   hipcc -O3 -std=c++17 -fPIC -shared -ffp-contract=off -I salva_amd/csrc tools/compound_host_arm.hip -o tools/libcompound_host_arm.so \
//         -L salva_amd/csrc -lsalva_hip -Wl,-rpath,'$ORIGIN/../salva_amd/csrc'
#include <vector>

#include "compound.h"

using namespace salva;

struct Arm {
    std::vector<CompoundPartDev> table;
    float mins[3], maxs[3];
    DcsParams pose{};
};

extern "C" void* arm_create(const SalvaHipCompoundPart* parts, uint32_t nparts, const float* translation, const float* rotation_ijkw) {
    Arm* a = new Arm();
    compound_build_table(parts, nparts, std::vector<const MeshRes*>(nparts, nullptr), a->table, a->mins, a->maxs);
    for (int k = 0; k < 3; ++k) a->pose.t[k] = translation[k];
    for (int k = 0; k < 4; ++k) a->pose.q[k] = rotation_ijkw[k];
    return a;
}
extern "C" void arm_destroy(void* user) { delete static_cast<Arm*>(user); }
extern "C" void arm_aabb(void* user, float* mins, float* maxs) {
    const Arm* a = static_cast<const Arm*>(user);
    aabb_transform_by(a->mins, a->maxs, a->pose.t, a->pose.q, mins, maxs);
}
extern "C" void arm_project(void* user, uint32_t n, const float* pts, float* proj, uint8_t* inside) {
    const Arm* a = static_cast<const Arm*>(user);
    for (uint32_t i = 0; i < n; ++i) {
        bool in;
        dcs_project_compound_world(a->table.data(), (uint32_t)a->table.size(), a->pose, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], proj[3 * i],
                                   proj[3 * i + 1], proj[3 * i + 2], in);
        inside[i] = in ? 1 : 0;
    }
}

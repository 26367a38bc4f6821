// compound_ray_arm.hip — the two callbacks of salva_hip_sample_host_shape for a compound, in C++ (tools/compound_sampling_bench.py): what
// a binding did to ray-sample a parry `Compound` before salva_hip_sample_compound.  The casts are the library's own
// (salva_amd/csrc/raycast.h is `__host__ __device__`) run on the host, one ray after the other; the box is the unloosened merge of the
// parts' boxes, as compound_build_table leaves it.
//   hipcc -O3 -std=c++17 -fPIC -shared -ffp-contract=off -I salva_amd/csrc tools/compound_ray_arm.hip -o tools/libcompound_ray_arm.so \
//         -L salva_amd/csrc -lsalva_hip -Wl,-rpath,'$ORIGIN/../salva_amd/csrc'
#include <vector>

#include "raycast.h"

using namespace salva;

struct RayArm {
    std::vector<CompoundPartDev> table;
    float mins[3], maxs[3];
};

extern "C" void* ray_arm_create(const SalvaHipCompoundPart* parts, uint32_t nparts) {
    RayArm* a = new RayArm();
    compound_build_table(parts, nparts, std::vector<const MeshRes*>(nparts, nullptr), a->table, a->mins, a->maxs);
    return a;
}
extern "C" void ray_arm_destroy(void* user) { delete static_cast<RayArm*>(user); }
extern "C" void ray_arm_aabb(void* user, float* mins, float* maxs) {
    const RayArm* a = static_cast<const RayArm*>(user);
    for (int k = 0; k < 3; ++k) { mins[k] = a->mins[k]; maxs[k] = a->maxs[k]; }
}
extern "C" void ray_arm_cast(void* user, uint32_t n, const float* origins, int32_t axis, float* toi) {
    const RayArm* a = static_cast<const RayArm*>(user);
    const float d[3] = {axis == 0 ? 1.0f : 0.0f, axis == 1 ? 1.0f : 0.0f, axis == 2 ? 1.0f : 0.0f};
    for (uint32_t i = 0; i < n; ++i) {
        const float t = compound_cast_ray<true>(a->table.data(), (uint32_t)a->table.size(), origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], d[0],
                                                d[1], d[2]);
        toi[i] = t < INFINITY ? t : -1.0f;
    }
}

// diffuse.h — the potentials of diffuse particles: spray, foam and bubbles (diffuse.hip; include/salva_hip.h "Diffuse particles";
// DESIGN.md §24).  Per particle of the selected fluids the number of its neighbours within h, the trapped-air and wave-crest sums of
// Ihmsen et al. 2012 over them, the surface normal from the gradient of the colour field and the kinetic energy.  Two passes walk one
// table of cells of width h built by the field evaluator's own keys, scan and order kernels (field.h): the second needs the normals
// the first leaves.
#pragma once
#include "field.h"

namespace salva {

enum : uint32_t { DIFFUSE_WANT_COUNT = 1, DIFFUSE_WANT_TRAPPED = 2, DIFFUSE_WANT_NORMAL = 4, DIFFUSE_WANT_CREST = 8, DIFFUSE_WANT_ENERGY = 16 };

struct DiffuseParams {  // SalvaHipDiffuse, validated
    float surface_min, crest_cos;
    float ta_lo, ta_hi, wc_lo, wc_hi, en_lo, en_hi, k_ta, k_wc;
    uint32_t max_per_particle, n_spray, n_bubble;
    float k_b, k_d, life_lo, life_hi;
    uint32_t seed, has_kill_box;
    float kill_lo[3], kill_hi[3], gravity[3];
};
// what the passes leave per host-order row v — zeros where the row has no part in the call —: a[v] = (trapped air, energy, wave crest,
// the count's bits), normal[v] = (n, n != 0 ? 1 : 0); and normal_sorted[p], the same record of sorted row p, for the second pass
struct DiffuseRows {
    float4 *a, *normal, *normal_sorted;
};

// One lane per sorted row of the table g (cells of width h; rows[p]: the host-order row behind sorted row p; cand.rec1 may be null
// when `want` is the count alone).
// Pass 1: count, trapped air, the normal and the energy of the outputs in `want`; the normal also when the crest is wanted.
void launch_diffuse_sums(uint32_t n, const FieldGrid& g, const FieldCandidates& cand, const uint32_t* rows, const SphConsts& c, const DiffuseParams& prm,
                         uint32_t want, const DiffuseRows& out, hipStream_t st);
// Pass 2: the wave crest, from the normals pass 1 wrote in sorted order
void launch_diffuse_crest(uint32_t n, const FieldGrid& g, const FieldCandidates& cand, const uint32_t* rows, const SphConsts& c, const DiffuseParams& prm,
                          const DiffuseRows& out, hipStream_t st);
// host-order rows -> the packed rows of salva_hip_diffuse_potentials (any output may be null)
void launch_diffuse_pack(uint32_t n, const uint32_t* st_model, const RowPack& pk, const DiffuseRows& in, float* trapped_air, float* wave_crest,
                         float* energy, float* normal, uint32_t* count, hipStream_t st);

// ---- the diffuse set: pos[i] = (x, lifetime), vel[i] = (v, the kind's bits), id[i]; in the order of creation
struct DiffuseSetDev {
    float4 *pos, *vel;
    uint32_t* id;
};
// what an update counts on the device: the survivors, by kind and in all, the removed, the emitted and the dropped
struct DiffuseCounters {
    uint32_t kept, kinds[4], dissolved, killed, emitted, dropped;
};
// who emits: the fluid's slot, the index within it and the draws are the random numbers' counters
struct DiffuseEmit {
    RowPack pk;
    uint32_t total;     // rows of the selected fluids
    uint32_t seed, updates, first_id, capacity;
    float radius, dt;
};

// n particles from packed xyz (and lifetimes, or `life` for all) behind the set's first `at`: kind 3, ids first_id ...
void launch_diffuse_add(uint32_t n, const float* pos, const float* vel, const float* lifetimes, float life, uint32_t at, uint32_t first_id,
                        const DiffuseSetDev& set, hipStream_t st);
// the set's rows as the caller's arrays (any may be null)
void launch_diffuse_get(uint32_t n, const DiffuseSetDev& set, float* pos, float* vel, float* life, uint32_t* kind, uint32_t* id, hipStream_t st);
// the positions as packed xyz: the points of the field evaluator
void launch_diffuse_set_points(uint32_t n, const DiffuseSetDev& set, float* pts, hipStream_t st);
// a. and the decisions of b.: fv / fc = the evaluator's velocity and count at the particles; keep[i] = 1 for a survivor
void launch_diffuse_advect(uint32_t n, const DiffuseSetDev& set, const float* fv, const uint32_t* fc, const DiffuseParams& prm, float dt,
                           uint32_t* keep, DiffuseCounters* counters, hipStream_t st);
// b.: after the exclusive scan of keep into off, the survivors in their order
void launch_diffuse_compact(uint32_t n, const uint32_t* keep, const uint32_t* off, const DiffuseSetDev& src, const DiffuseSetDev& dst,
                            DiffuseCounters* counters, hipStream_t st);
// c.: cnt[r] = the particles row r emits (r: the packed row of the potentials call)
void launch_diffuse_rate(uint32_t n, const float4* st_pos, const float4* st_vel, const uint32_t* st_model, const DiffuseRows& rows,
                         const DiffuseParams& prm, const DiffuseEmit& em, uint32_t* cnt, hipStream_t st);
// c.: after the exclusive scan of cnt into off, the new particles behind counters->kept
void launch_diffuse_emit(uint32_t n, const float4* st_pos, const float4* st_vel, const uint32_t* st_model, const DiffuseParams& prm,
                         const DiffuseEmit& em, const uint32_t* cnt, const uint32_t* off, const DiffuseSetDev& set, DiffuseCounters* counters,
                         hipStream_t st);

}  // namespace salva

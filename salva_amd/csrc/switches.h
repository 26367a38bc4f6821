// switches.h — the environment switches of a World: read once, when the world is constructed (Switches::from_env, world.hip), and never
// changed afterwards; World holds them as `const Switches sw`.  This is the authoritative list (INTEGRATION.md §4 and the build notes of
// DESIGN.md repeat the names).
// Read elsewhere, because they are not a World's: SALVA_HIP_CELL_TABLE_GIB (dims_from_bbox, world.hip), SALVA_HIP_SORT_DEFAULT_DIGITS
// (grid.hip), SALVA_HIP_P3_PAD (pairs.h), SALVA_HIP_DIST_TRACE (also the transports of comm.hip), SALVA_HIP_PEER_TIMEOUT_S
// (comm_peer.hip); and in kernel-development builds the variant probe's own SALVA_HIP_PIPE_WAVES / SALVA_HIP_TILE_TIMING /
// SALVA_HIP_VARIANT_VERBOSE (diag/world_diag.hip).
#pragma once
#include <cstdint>

namespace salva {

struct Switches {
    // Speculative sizing is OFF unless asked for (SALVA_HIP_SPECULATE=1; SALVA_HIP_NO_SPECULATION=1 overrides it).  Measured on the
    // bench scene (10^6 particles): it removes two ~20 us host round trips from a ~0.9 ms free-fall step (-2 %), but a failed
    // prediction costs a whole extra step, and at the impact — where the halo and the lists grow for a dozen steps in a row — two
    // passes in twenty were discarded, 2.25 ms per step against 1.88 ms without speculation.  Kept as an option for steady flows.
    bool spec_off = true;
    bool spec_tight = false;       // SALVA_HIP_SPEC_TIGHT: no margin on the predicted totals — the tests' way to force misses
    bool defer_off = false;        // SALVA_HIP_NO_DEFER_LISTS: check the list capacity in the middle of the step
    bool spec_apply_off = false;   // SALVA_HIP_NO_SPEC_APPLY (A/B, tests)
    bool spec_dist_off = false;    // SALVA_HIP_NO_SPEC_DIST=1 (A/B, tests)
    bool overlap_exchange = true;  // SALVA_HIP_NO_OVERLAP=1 turns it off (diagnostics)
    bool chain_off = false;        // SALVA_HIP_NO_CHAIN=1 (A/B, tests)
    bool pre_off = false;          // SALVA_HIP_NO_PREGRID=1 (A/B, tests)
    bool no_publish = false;       // SALVA_HIP_NO_PUBLISH (diagnostics: A/B of the solves' publication against the copy + wait)
    bool split_off = false;        // SALVA_HIP_NO_SPLIT=1: no splitting of over-full tiles (device_types.h StepCtx::split_s)
    uint32_t split_forced = 0;     // SALVA_HIP_SPLIT_S=k: split at k halo particles whatever the statistics say (tests)
    bool classes_off = false, classes_forced = false, light_on = false;  // SALVA_HIP_NO_CLASSES=1 / SALVA_HIP_CLASSES=1 / SALVA_HIP_LIGHT=1 (the light class: opt-in, it lost)
    bool ref_off = false, ref_forced = false;  // SALVA_HIP_FULL_HALO=1 (A/B: stage the full box) / SALVA_HIP_REF_HALO=1 (in every step: tests)
    bool ref_tight = false;        // SALVA_HIP_REF_TIGHT=1 (tests): cut the launches for LESS than the previous step's kept maxima — every such pass misses
    bool compact_halo = false;     // SALVA_HIP_COMPACT_HALO: compact rows in the halo slot tables whatever fixed-stride rows would cost (tests)
    bool no_planes = false;        // SALVA_HIP_NO_PLANES=1 (A/B): keep the 32-byte-per-slot evaluate kernels
    bool no_fused_div = false;     // SALVA_HIP_NO_FUSED_DIV=1 (A/B): the first divergence evaluate stays a pass of its own
    bool two_mass_off = false;     // SALVA_HIP_NO_TWO_MASS=1 (A/B, tests): such a world keeps the general kernels
    uint32_t max_masses = 2;       // SALVA_HIP_MAX_MASSES=3 / 4: opt-in — on the one 10^6-particle scene it was measured on (four columns,
                                   // tools/r06/multi_mass_probe.py) the general kernels are 8-10 % faster than the segments of three and four masses
    bool fold_off = false;         // SALVA_HIP_NO_FOLD=1: the fluid grid is never folded (device_types.h TileGrid)
    uint32_t fold_forced = 0;      // SALVA_HIP_FOLD_CELLS=P: every axis longer than P cells is folded to exactly P (tests)
    int sort_mode = -1;            // SALVA_HIP_RADIX_SORT: 1 = always the radix sort + k_cell_start, 0 = always the counting sort by cell, unset = by size
    uint32_t ds_level = 0;         // SALVA_HIP_DS_LEVEL (tests: pairs.h pick_ds*); the constructor hands it to TileLds::ds_level
    // SALVA_HIP_LIST_CAP0 (tests: force an overflow): the initial ELL capacity, which also counts as checked, so that the very first
    // step takes the deferred path.  The constructor hands list_cap0 to cap_ff when trust_cap0 says it was given.
    bool trust_cap0 = false;
    uint32_t list_cap0 = 0;
    bool dcs_batch_off = false;    // SALVA_HIP_NO_DCS_BATCH=1 (A/B, tests): every DynamicContactSampling collider takes the per-collider path
    uint32_t dcsb_cap0 = 0;        // SALVA_HIP_DCSB_CAP0=k (tests: force a repeat): the first capacity of the batched pass's record buffer
    int field_arm = 0;             // SALVA_HIP_FIELD_ARM=points|lattice (tests, measurements): the arm every lattice evaluation takes
    bool tile_trace = false;       // SALVA_HIP_TILE_TRACE=1: one line of tile statistics per step on stderr
    bool dist_trace = false;       // SALVA_HIP_DIST_TRACE: one line per decomposed divergence solve whose applies ran beside the all-reduce
#ifdef SALVA_HIP_DIAG
    int sched_mode = 0;            // SALVA_HIP_SCHED: 1 = run diag/sched.hip after the list build
    bool tile_threads_set = false; // SALVA_HIP_TILE_THREADS: the workgroup size of the tile kernels, whatever size_pass would choose
    uint32_t tile_threads = 0;
    bool no_pipeline = false;      // SALVA_HIP_NO_PIPELINE: the persistent pipeline kernels (pipe.h) stay off
    uint32_t pipe_waves = 0;       // SALVA_HIP_PIPE_WAVES: their waves per workgroup (0: one per slice of the fullest tile, at least four)
    bool tile_timing = false;      // SALVA_HIP_TILE_TIMING: salva_hip_time_pred_density prints the per-tile phase report first
#endif
    static Switches from_env();
};

}  // namespace salva

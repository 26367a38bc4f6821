// field.h — SPH fields at places that are not particles (field.hip): the evaluator's own cell table over the box of
// a query, the particles of the selected fluids sorted into it "by cell, then by host index", and the two kernels that sum over them —
// one lane per point (k_field_points) and one workgroup per brick of 8 x 8 x 8 lattice nodes (k_field_lattice).
#pragma once
#include "common.h"
#include "sph_math.h"
#include "../../include/salva_hip.h"

namespace salva {

constexpr uint32_t FIELD_MAX_SLOTS = 32;          // fluids per world (tile.h MAX_MODELS)
constexpr uint64_t FIELD_MAX_CELLS = 1ull << 27;  // cells of one query's own table
constexpr uint32_t FIELD_DROPPED = 0xffffffffu;   // the key of a particle outside the query's box, of another fluid or not finite
constexpr uint32_t FIELD_BRICK = 8;               // nodes per axis of a brick
constexpr uint32_t FIELD_BRICK_THREADS = FIELD_BRICK * FIELD_BRICK * FIELD_BRICK;
constexpr uint32_t FIELD_CHUNK = 512;             // candidates a brick stages at a time: two float4 each, 16 KiB of LDS

enum : uint32_t { FIELD_WANT_DENSITY = 1, FIELD_WANT_FRACTION = 2, FIELD_WANT_VELOCITY = 4, FIELD_WANT_GRADIENT = 8, FIELD_WANT_COUNT = 16 };

// cells o + [0, d) per axis, width h; cell (x, y, z) has the linear index (x d[1] + y) d[2] + z: ascending index = x slowest, z fastest
struct FieldGrid {
    int o[3];
    uint32_t d[3];
    uint32_t ncells;
    float h;
};
// the selected fluids and the rest density of each
struct FieldFluids {
    uint32_t mask;
    float density0[FIELD_MAX_SLOTS];
};
// where the sums are wanted: `pts` (packed xyz, npoints of them), or with pts == nullptr the nodes of a lattice, node (ix, iy, iz)
// at origin + (float)i * spacing per axis and at index (ix ny + iy) nz + iz
struct FieldQuery {
    const float* pts;
    uint64_t npoints;
    float origin[3];
    float spacing;
    uint32_t dims[3];
};
struct FieldOutDev {  // a null pointer: not written
    float *density, *fraction, *velocity, *gradient;
    uint32_t* count;
};
// the sorted candidates: rec0 = (x, y, z, m), rec1 = (vx, vy, vz, V) (nullptr when neither velocity nor fraction is wanted), and
// cells[c] .. cells[c + 1] the rows of cell c
struct FieldCandidates {
    const uint32_t* cells;
    const float4* rec0;
    const float4* rec1;
};
// where the rows of the selected fluids go in a packed output: fluid s has its len[s] host rows at first[s] and its output rows at
// base[s] (selected fluids only)
struct RowPack {
    uint32_t mask;
    uint32_t first[FIELD_MAX_SLOTS], len[FIELD_MAX_SLOTS], base[FIELD_MAX_SLOTS];
};

// box6 = {min x, y, z, max x, y, z} of the finite points among `pts`, as ordered integers (field_ordered / field_unordered);
// the caller has set it to {INT32_MAX x 3, INT32_MIN x 3}
void launch_field_bbox(const float* pts, uint64_t npoints, int32_t* box6, hipStream_t st);
inline int32_t field_ordered(float f) { int32_t i; __builtin_memcpy(&i, &f, 4); return i ^ ((i >> 31) & 0x7fffffff); }
inline float field_unordered(int32_t i) { i ^= (i >> 31) & 0x7fffffff; float f; __builtin_memcpy(&f, &i, 4); return f; }
// keys[i] = the cell of row i in g, or FIELD_DROPPED; rank[i] = its place among the rows of its cell in the order the atomics were
// served; cells[c] = rows of cell c (zeroed by the caller, g.ncells + 1 words)
void launch_field_keys(const float4* st_pos, const uint32_t* st_model, uint32_t n, const FieldFluids& f, const FieldGrid& g, uint32_t* keys,
                       uint32_t* rank, uint32_t* cells, hipStream_t st);
// after the exclusive scan of `cells` in place: the kept rows by cell, then by host index, gathered into rec0 / rec1 (rec1 may be null);
// rows (may be null): the host-order row behind each sorted row
void launch_field_sort(const float4* st_pos, const float4* st_vel, const uint32_t* st_model, uint32_t n, const FieldFluids& f, const FieldGrid& g,
                       const uint32_t* keys, const uint32_t* rank, const uint32_t* cells, uint32_t* keys_sorted, uint32_t* idx_tmp, float4* rec0,
                       float4* rec1, uint32_t* rows, hipStream_t st);
void launch_field_points(const FieldQuery& q, const FieldGrid& g, const FieldCandidates& cand, const SphConsts& c, const FieldOutDev& out,
                         hipStream_t st);
void launch_field_lattice(const FieldQuery& q, const FieldGrid& g, const FieldCandidates& cand, const SphConsts& c, const FieldOutDev& out,
                          hipStream_t st);

}  // namespace salva

// fluidcast.h — rays cast at the fluid's particles, each a sphere of radius R (fluidcast.hip, world_cast.hip): the first
// hit with its particle and normal, and the thickness of fluid along the ray.  The contract is include/salva_hip.h's ("Rays cast at the
// fluid"); the candidates are the field evaluator's sorted table over the box B of the call (field.h) plus the host-order row of every
// sorted row, and the walk of a ray through that table is the one kernel of fluidcast.hip.
#pragma once
#include "field.h"

namespace salva {

constexpr uint32_t CAST_MAX_AXIS_CELLS = 1u << 16;  // cells per axis of a cast's own table
constexpr uint32_t CAST_NONE = 0xffffffffu;         // fluid and index of a miss
constexpr uint32_t CAST_TILE = 8;                   // a wave of a camera call takes a tile of 8 x 8 pixels

// the rays of a call: a list (origins / directions, packed xyz, in the caller's order), or with origins == nullptr the pixels of a camera
struct CastRays {
    const float* origins;
    const float* directions;
    uint64_t nrays;
    float cam_o[3], cam_f[3], cam_r[3], cam_u[3];
    uint32_t width, height;
};
// R and tmax; the box B (closed) a particle must lie in, G = B grown by R, and the walk's margin eps (fluidcast.hip)
struct CastParams {
    float radius, tmax;
    float blo[3], bhi[3], glo[3], ghi[3];
    float eps;
};
// the sorted candidates of field.h and the host-order row of each; first[s] = the first host-order row of fluid s
struct CastTable {
    const uint32_t* cells;
    const float4* rec0;
    const uint32_t* rows;
    const uint32_t* st_model;
    uint32_t first[FIELD_MAX_SLOTS];
};
struct CastOutDev {  // a null pointer: not written
    float* t;
    uint32_t *fluid, *index;
    float *normal, *thickness;
    uint32_t* tested;  // salva_hip_count_ray_candidates: exact casts made per ray (the counting instances; every other pointer null)
};

// eps of a box G: 2^-19 (the largest |coordinate| of G + the sum of its extents), in f32, every operation rounded once
float cast_eps(const float glo[3], const float ghi[3]);
// hit: t / fluid / index / normal are wanted; thick: thickness is.  At least one of them.  With out.tested: exactly one of them, and
// the walk of that call is counted.
void launch_fluid_cast(const CastRays& rays, const CastParams& p, const FieldGrid& g, const CastTable& tab, const CastOutDev& out, bool hit,
                       bool thick, hipStream_t st);
// every ray of a call without a qualifying particle: a miss
void launch_fluid_cast_miss(uint64_t nrays, const CastOutDev& out, hipStream_t st);

}  // namespace salva

// anisotropy.h — anisotropic kernels for the fluid's surface (anisotropy.hip; include/salva_hip.h "Anisotropic kernels"; DESIGN.md
// §23): per particle the moments of its neighbourhood of radius 2h, from them a smoothed centre and a 3 x 3 metric G, and the fields
// of §20 summed with q = |G (x - centre)| instead of |x - x_j| / h.  Both passes walk tables of cells of width 2h built by the field
// evaluator's own keys, scan and order kernels (field.h).
#pragma once
#include "field.h"

namespace salva {

struct AnisoParams {  // SalvaHipAnisotropy, validated
    float lambda, k_r, k_s, k_n;
    uint32_t n_eps;
};
// what the moments pass leaves per host-order row v: centre[v] = (c, V) — NaN where the row has no part in the call —,
// m0[v] = (Gxx, Gxy, Gxz, Gyy), m1[v] = (Gyz, Gzz, det G m, det G V), count[v]
struct AnisoRows {
    float4 *centre, *m0, *m1;
    uint32_t* count;
};
struct AnisoOutDev {  // a null pointer: not written
    float *density, *fraction, *gradient;
};

// One lane per sorted row of the table g (cells of width 2h over the raw positions; rows[p]: the host-order row behind sorted row p).
// A row in one of the outermost `ring` cell layers of g is a neighbour only — its own neighbourhood is not complete in g — and gets
// nothing written.
void launch_aniso_moments(uint32_t n, const FieldGrid& g, const FieldCandidates& cand, const uint32_t* rows, const float4* st_pos, uint32_t ring,
                          const AnisoParams& prm, float h, const AnisoRows& out, hipStream_t st);
// the metric records of the sorted rows of a table built on the centres
void launch_aniso_gather(uint32_t n, const uint32_t* cells, uint32_t ncells, const uint32_t* rows, const AnisoRows& in, float4* g0, float4* g1,
                         hipStream_t st);
// One lane per place of q; g, cand: the table over the centres; g0, g1: the metric records beside cand.rec0.  c: SphConsts of h = 1 with
// the world's kernel kinds.
void launch_aniso_points(const FieldQuery& q, const FieldGrid& g, const FieldCandidates& cand, const float4* g0, const float4* g1, const SphConsts& c,
                         const AnisoOutDev& out, hipStream_t st);
// host-order rows -> the packed rows of salva_hip_compute_anisotropy (any output may be null)
void launch_aniso_pack(uint32_t n, const float4* st_pos, const uint32_t* st_model, const RowPack& pk, const AnisoRows& in, float* centres,
                       float* metric, uint32_t* count, hipStream_t st);

}  // namespace salva

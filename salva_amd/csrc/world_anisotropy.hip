// world_anisotropy.hip — anisotropic kernels for the fluid's surface (salva_hip_compute_anisotropy, salva_hip_evaluate_fields_anisotropic /
// _lattice, salva_hip_extract_surface_anisotropic): what the parameters must be, the two tables of cells of width 2h —
// one on the raw positions for the moments, one on the centres for the sums, both built by the field evaluator's table code
// (world_field.hip field_table) —, and the buffers of the caller.  Nothing here writes anything a step reads.
#include "world.h"

#include <cmath>
#include <cstring>

namespace salva {

static_assert(sizeof(SalvaHipAnisotropy) == SALVA_HIP_ANISOTROPY_BYTES, "SalvaHipAnisotropy: the header's size constant is what the mirrors check");

AnisoParams World::aniso_params(const SalvaHipAnisotropy* p, const char* what) const {
    const std::string w(what);
    if (!p) throw HipError(SALVA_HIP_E_INVALID, w + ": null params");
    if (p->struct_size != SALVA_HIP_ANISOTROPY_BYTES || p->version != SALVA_HIP_ANISOTROPY_VERSION)
        throw HipError(SALVA_HIP_E_INVALID, w + ": params with a struct_size / version other than this library's");
    if (!(p->lambda >= 0.0f && p->lambda <= 1.0f)) throw HipError(SALVA_HIP_E_INVALID, w + ": lambda must lie in [0, 1]");
    if (!(std::isfinite(p->k_r) && p->k_r >= 1.0f)) throw HipError(SALVA_HIP_E_INVALID, w + ": k_r must be finite and >= 1");
    if (!(std::isfinite(p->k_s) && p->k_s > 0.0f)) throw HipError(SALVA_HIP_E_INVALID, w + ": k_s must be finite and > 0");
    if (!(p->k_n >= SALVA_HIP_ANISOTROPY_S_LO && p->k_n <= SALVA_HIP_ANISOTROPY_S_HI))
        throw HipError(SALVA_HIP_E_INVALID, w + ": k_n must lie in [S_LO, S_HI]");
    return AnisoParams{p->lambda, p->k_r, p->k_s, p->k_n, p->n_eps};
}

// The moments pass over the table on the raw positions: the cells [lo, hi] touches and `grow` more on every side; the rows of the
// outermost `ring` layers are neighbours only.  Every other row of the staging arrays is left with a NaN centre and zeros.
AnisoRows World::aniso_moments(const FieldFluids& f, const AnisoParams& prm, const float lo[3], const float hi[3], int grow, uint32_t ring) {
    const size_t rows = n ? n : 1;
    ani.centre.ensure(rows, stream, false, 1.1f); ani.m0.ensure(rows, stream, false, 1.1f); ani.m1.ensure(rows, stream, false, 1.1f);
    ani.count.ensure(rows, stream, false, 1.1f);
    const AnisoRows r{ani.centre.p, ani.m0.p, ani.m1.p, ani.count.p};
    SALVA_HIP_CHECK(hipMemsetAsync(r.centre, 0xff, rows * sizeof(float4), stream));  // (all bits set: NaN)
    SALVA_HIP_CHECK(hipMemsetAsync(r.m0, 0, rows * sizeof(float4), stream));
    SALVA_HIP_CHECK(hipMemsetAsync(r.m1, 0, rows * sizeof(float4), stream));
    SALVA_HIP_CHECK(hipMemsetAsync(r.count, 0, rows * sizeof(uint32_t), stream));
    if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) return r;  // (no finite particle)
    FieldGrid g{};
    const FieldCandidates cand = field_table(f, st_pos.p, sc.h + sc.h, grow, lo, hi, false, g, true,
                                             "anisotropic kernels: the box exceeds 2^27 cells of width 2h: split the query");
    launch_aniso_moments(n, g, cand, fld.rows.p, st_pos.p, ring, prm, sc.h, r, stream);
    return r;
}

void World::compute_anisotropy(uint32_t fluid_mask, const SalvaHipAnisotropy* params, uint32_t flags, const SalvaHipAnisotropyOut* out,
                               uint64_t* nrows) {
    const char* what = "salva_hip_compute_anisotropy";
    *nrows = 0;
    const FieldFluids f = field_begin(fluid_mask, 0, what);
    if (flags & ~(uint32_t)SALVA_HIP_ANISOTROPY_OUT_ON_DEVICE) throw HipError(SALVA_HIP_E_INVALID, std::string(what) + ": unknown flag");
    const AnisoParams prm = aniso_params(params, what);
    uint64_t total = 0;
    const RowPack pk = rows_pack(f, total);
    if (!fill_wanted(total, nrows, out, what, "rows")) return;
    if (!total || !(out->centres || out->metric || out->count)) return;
    float lo[3], hi[3];
    uint64_t nfinite = 0;
    get_fluid_bounds(f.mask, lo, hi, &nfinite);
    const AnisoRows r = aniso_moments(f, prm, lo, hi, 1, 0);
    QueryOut o{{{out->centres, 3 * total}, {out->metric, 6 * total}, {out->count, total}}};
    query_place(o, (flags & SALVA_HIP_ANISOTROPY_OUT_ON_DEVICE) != 0u);
    launch_aniso_pack(n, st_pos.p, st_model.p, pk, r, o.f32(0), o.f32(1), o.u32(2), stream);
    query_finish(o);
}

// m places, their box (box_empty: none of them is finite — everything is zero), the caller's buffers (world_field.hip field_run)
void World::aniso_run(const FieldFluids& f, const AnisoParams& prm, const FieldQuery& q, const float lo[3], const float hi[3], bool box_empty, uint64_t m,
                      uint32_t flags, const SalvaHipAnisoFieldOut& out) {
    QueryOut o{{{out.density, m}, {out.fraction, m}, {out.gradient, 3 * m}}};
    query_place(o, (flags & SALVA_HIP_FIELD_OUT_ON_DEVICE) != 0u);
    if (!o.any()) return;
    if (box_empty) {
        query_zero(o);
    } else {
        // What can matter to a place in [lo, hi]: a centre within 2h of it, whose particle lies within 2h of the centre and whose
        // neighbours lie within 2h of the particle — three cells of width 2h, of which the outermost layer holds neighbours only.
        const AnisoRows r = aniso_moments(f, prm, lo, hi, 3, 1);
        FieldGrid g{};
        // (this table's row map overwrites the first's, behind the moments pass on the stream)
        const FieldCandidates cand = field_table(f, r.centre, sc.h + sc.h, 1, lo, hi, false, g, true,
                                                 "anisotropic kernels: the box exceeds 2^27 cells of width 2h: split the query");
        const size_t rows = n ? n : 1;
        ani.g0.ensure(rows, stream, false, 1.1f); ani.g1.ensure(rows, stream, false, 1.1f);
        launch_aniso_gather(n, cand.cells, g.ncells, fld.rows.p, r, ani.g0.p, ani.g1.p, stream);
        SphConsts unit = make_sph_consts(1.0f);  // P and P' are the world's kernels at h = 1
        unit.kd = sc.kd; unit.kg = sc.kg;
        launch_aniso_points(q, g, cand, ani.g0.p, ani.g1.p, unit, AnisoOutDev{o.f32(0), o.f32(1), o.f32(2)}, stream);
    }
    query_finish(o);
}

void World::evaluate_aniso_points(const FieldFluids& f, const AnisoParams& prm, uint64_t npoints, const float* points_xyz, uint32_t flags,
                                  const SalvaHipAnisoFieldOut& out, const char* what) {
    if (npoints == 0) return;
    float lo[3], hi[3];
    const FieldQuery q = field_points_query(npoints, points_xyz, flags, lo, hi, what);
    aniso_run(f, prm, q, lo, hi, !(lo[0] <= hi[0]), npoints, flags, out);
    if (!(flags & SALVA_HIP_FIELD_POINTS_ON_DEVICE)) SALVA_HIP_CHECK(hipStreamSynchronize(stream));
}

void World::evaluate_aniso_lattice(const FieldFluids& f, const AnisoParams& prm, const float origin[3], float spacing, const uint32_t dims[3],
                                   uint32_t flags, const SalvaHipAnisoFieldOut& out, const char* what) {
    float lo[3], hi[3];
    bool box_empty = false;
    const FieldQuery q = field_lattice_query(origin, spacing, dims, lo, hi, box_empty, what);
    aniso_run(f, prm, q, lo, hi, box_empty, q.npoints, flags, out);
}

void World::evaluate_fields_anisotropic(uint32_t fluid_mask, const SalvaHipAnisotropy* params, uint64_t npoints, const float* points_xyz, uint32_t flags,
                                        const SalvaHipAnisoFieldOut& out) {
    const char* what = "salva_hip_evaluate_fields_anisotropic";
    const FieldFluids f = field_begin(fluid_mask, flags, what);
    evaluate_aniso_points(f, aniso_params(params, what), npoints, points_xyz, flags, out, what);
}

void World::evaluate_fields_anisotropic_lattice(uint32_t fluid_mask, const SalvaHipAnisotropy* params, const float origin[3], float spacing,
                                                const uint32_t dims[3], uint32_t flags, const SalvaHipAnisoFieldOut& out) {
    const char* what = "salva_hip_evaluate_fields_anisotropic_lattice";
    const FieldFluids f = field_begin(fluid_mask, flags, what);
    evaluate_aniso_lattice(f, aniso_params(params, what), origin, spacing, dims, flags, out, what);
}

}  // namespace salva

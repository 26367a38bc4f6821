// world_surface.hip — the iso-surface of a field as a triangle mesh (salva_hip_extract_surface / _from_values, salva_hip_get_fluid_bounds;
// DESIGN.md §21): what a call must be, where the node values come from (the field evaluator's lattice call into scratch, or the caller's
// lattice), the passes of surface.hip with the one read-back that decides the capacity outcome, the evaluator's points path on the
// vertices for normals and velocities, and the buffers of the caller.  Nothing here writes anything a step reads.
#include "world.h"

#include <cmath>
#include <cstring>

namespace salva {

static void surface_check_out(const SalvaHipSurfaceOut* out, bool attributes, const std::string& w) {
    if (!out) return;
    if (!out->vertices || !out->triangles) throw HipError(SALVA_HIP_E_INVALID, w + ": out without vertices or triangles");
    if (!attributes && (out->normals || out->velocities))
        throw HipError(SALVA_HIP_E_INVALID, w + ": normals and velocities must be NULL: a supplied lattice has no particles behind it");
}

SurfaceLattice World::surface_lattice(float iso, const float origin[3], float spacing, const uint32_t dims[3], const char* what) const {
    const std::string w(what);
    if (!std::isfinite(iso)) throw HipError(SALVA_HIP_E_INVALID, w + ": iso must be finite");
    if (!(std::isfinite(spacing) && spacing > 0.0f)) throw HipError(SALVA_HIP_E_INVALID, w + ": spacing must be finite and > 0");
    if (dims[0] < 2 || dims[1] < 2 || dims[2] < 2) throw HipError(SALVA_HIP_E_INVALID, w + ": every dimension must be at least 2");
    const uint64_t xy = (uint64_t)dims[0] * dims[1];
    if (xy > SURFACE_MAX_NODES || xy * dims[2] > SURFACE_MAX_NODES)
        throw HipError(SALVA_HIP_E_CAPACITY, w + ": 2^31 - 1 nodes or more: split the lattice");
    SurfaceLattice g{};
    for (int a = 0; a < 3; ++a) { g.origin[a] = origin[a]; g.dims[a] = dims[a]; }
    g.spacing = spacing;
    g.n = (uint32_t)(xy * dims[2]);
    return g;
}

// d_values: the n node values in device memory.  fluid_mask: whose gradient and velocity the vertices get (where `out` asks).
void World::surface_run(const float* d_values, float iso, const SurfaceLattice& g, uint32_t fluid_mask, bool on_device, const SalvaHipSurfaceOut* out,
                        uint64_t counts[2], const char* what, const AnisoParams* aniso) {
    const std::string w(what);
    const size_t tb = surface_temp_bytes(g.n);
    srf.word.ensure((size_t)g.n + 1, stream, false, 1.1f);
    srf.totals.ensure(1);
    srf.temp.ensure(tb ? tb : 1);
    SALVA_HIP_CHECK(hipMemsetAsync(srf.totals.p, 0, sizeof(SurfaceTotals), stream));
    launch_surface_classify(d_values, iso, g, srf.word.p, srf.totals.p, stream);
    launch_surface_totals(srf.temp.p, tb, srf.word.p, g.n, srf.totals.p, stream);
    // the one read-back: the two totals and the flag
    SurfaceTotals tot{};
    SALVA_HIP_CHECK(hipMemcpyAsync(&tot, srf.totals.p, sizeof(tot), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    if (tot.nonfinite) throw HipError(SALVA_HIP_E_INVALID, w + ": a node value is not finite");
    const uint64_t nv = tot.nv, nt = tot.nt;
    counts[0] = nv; counts[1] = nt;
    if (nv >= (1ull << 32) || 3 * nt >= (1ull << 32))
        throw HipError(SALVA_HIP_E_CAPACITY, w + ": the mesh has 2^32 vertices or triangle indices or more: split the lattice");
    if (!out) return;
    if (out->vertex_capacity < nv || out->triangle_capacity < nt)
        throw HipError(SALVA_HIP_E_CAPACITY, w + ": the mesh has " + std::to_string(nv) + " vertices and " + std::to_string(nt) +
                                                 " triangles: more than the capacities of out");
    if (!nv && !nt) return;
    // all four at once, before the first kernel: the queries at the vertices below write to device memory and place nothing
    QueryOut o{{{out->vertices, 3 * nv}, {out->normals, 3 * nv}, {out->velocities, 3 * nv}, {out->triangles, 3 * nt}}};
    query_place(o, on_device);
    float *const d_vertices = o.f32(0), *const d_normals = o.f32(1), *const d_velocities = o.f32(2);
    srf.voff.ensure((size_t)g.n + 1, stream, false, 1.1f);
    srf.toff.ensure((size_t)g.n + 1, stream, false, 1.1f);
    launch_surface_scans(srf.temp.p, tb, srf.word.p, g.n, srf.voff.p, srf.toff.p, stream);
    launch_surface_emit(d_values, iso, g, srf.word.p, srf.voff.p, srf.toff.p, nv, nt, d_vertices, o.u32(3), stream);
    if ((d_normals || d_velocities) && nv) {
        // the evaluator's own sums at the vertices, through its points path: the gradient lands where the normals go
        SalvaHipFieldOut fo{};
        fo.gradient = aniso ? nullptr : d_normals;
        fo.velocity = d_velocities;
        const uint32_t there = SALVA_HIP_FIELD_POINTS_ON_DEVICE | SALVA_HIP_FIELD_OUT_ON_DEVICE;
        if (fo.gradient || fo.velocity) evaluate_fields(fluid_mask, nv, d_vertices, there, fo);
        if (aniso && d_normals) {  // (the surface of the anisotropic fields: their gradient)
            SalvaHipAnisoFieldOut ao{};
            ao.gradient = d_normals;
            evaluate_aniso_points(field_begin(fluid_mask, there, what), *aniso, nv, d_vertices, there, ao, what);
        }
        if (d_normals) launch_surface_normals(d_normals, nv, stream);
    }
    query_finish(o);  // (an output of no words is not copied)
}

void World::extract_surface(uint32_t fluid_mask, uint32_t field, float iso, const float origin[3], float spacing, const uint32_t dims[3], uint32_t flags,
                            const SalvaHipSurfaceOut* out, uint64_t counts[2]) {
    const char* what = "salva_hip_extract_surface";
    counts[0] = counts[1] = 0;
    if (flags & ~(uint32_t)SALVA_HIP_SURFACE_OUT_ON_DEVICE) throw HipError(SALVA_HIP_E_INVALID, std::string(what) + ": unknown flag");
    if (field != SALVA_HIP_SURFACE_DENSITY && field != SALVA_HIP_SURFACE_FRACTION) throw HipError(SALVA_HIP_E_INVALID, std::string(what) + ": unknown field");
    const FieldFluids f = field_begin(fluid_mask, 0, what);
    const SurfaceLattice g = surface_lattice(iso, origin, spacing, dims, what);
    surface_check_out(out, true, what);
    // the node values: the evaluator's lattice call, arm switch and all, into scratch
    srf.values.ensure(g.n, stream, false, 1.1f);
    SalvaHipFieldOut fo{};
    (field == SALVA_HIP_SURFACE_DENSITY ? fo.density : fo.fraction) = srf.values.p;
    evaluate_fields_lattice(f.mask, origin, spacing, dims, SALVA_HIP_FIELD_OUT_ON_DEVICE, fo);
    surface_run(srf.values.p, iso, g, f.mask, (flags & SALVA_HIP_SURFACE_OUT_ON_DEVICE) != 0u, out, counts, what);
}

// the same with the anisotropic kernels of world_anisotropy.hip behind the node values and the normals
void World::extract_surface_anisotropic(uint32_t fluid_mask, const SalvaHipAnisotropy* params, uint32_t field, float iso, const float origin[3],
                                        float spacing, const uint32_t dims[3], uint32_t flags, const SalvaHipSurfaceOut* out, uint64_t counts[2]) {
    const char* what = "salva_hip_extract_surface_anisotropic";
    counts[0] = counts[1] = 0;
    if (flags & ~(uint32_t)SALVA_HIP_SURFACE_OUT_ON_DEVICE) throw HipError(SALVA_HIP_E_INVALID, std::string(what) + ": unknown flag");
    if (field != SALVA_HIP_SURFACE_DENSITY && field != SALVA_HIP_SURFACE_FRACTION) throw HipError(SALVA_HIP_E_INVALID, std::string(what) + ": unknown field");
    const FieldFluids f = field_begin(fluid_mask, 0, what);
    const AnisoParams prm = aniso_params(params, what);
    const SurfaceLattice g = surface_lattice(iso, origin, spacing, dims, what);
    surface_check_out(out, true, what);
    srf.values.ensure(g.n, stream, false, 1.1f);
    SalvaHipAnisoFieldOut fo{};
    (field == SALVA_HIP_SURFACE_DENSITY ? fo.density : fo.fraction) = srf.values.p;
    evaluate_aniso_lattice(f, prm, origin, spacing, dims, SALVA_HIP_FIELD_OUT_ON_DEVICE, fo, what);
    surface_run(srf.values.p, iso, g, f.mask, (flags & SALVA_HIP_SURFACE_OUT_ON_DEVICE) != 0u, out, counts, what, &prm);
}

void World::extract_surface_from_values(const float* values, float iso, const float origin[3], float spacing, const uint32_t dims[3], uint32_t flags,
                                        const SalvaHipSurfaceOut* out, uint64_t counts[2]) {
    const char* what = "salva_hip_extract_surface_from_values";
    counts[0] = counts[1] = 0;
    use_device();
    if (in_force_cb || in_dforce_cb || in_coupling_cb) throw HipError(SALVA_HIP_E_INVALID, std::string(what) + ": not available inside a callback of a step");
    if (flags & ~(uint32_t)(SALVA_HIP_SURFACE_VALUES_ON_DEVICE | SALVA_HIP_SURFACE_OUT_ON_DEVICE))
        throw HipError(SALVA_HIP_E_INVALID, std::string(what) + ": unknown flag");
    const SurfaceLattice g = surface_lattice(iso, origin, spacing, dims, what);
    surface_check_out(out, false, what);
    const float* d_values = values;
    if (!(flags & SALVA_HIP_SURFACE_VALUES_ON_DEVICE)) {
        srf.values.ensure(g.n, stream, false, 1.1f);
        SALVA_HIP_CHECK(hipMemcpyAsync(srf.values.p, values, (size_t)g.n * sizeof(float), hipMemcpyHostToDevice, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
        d_values = srf.values.p;
    }
    surface_run(d_values, iso, g, 0u, (flags & SALVA_HIP_SURFACE_OUT_ON_DEVICE) != 0u, out, counts, what);
}

void World::get_fluid_bounds(uint32_t fluid_mask, float lo[3], float hi[3], uint64_t* nfinite) {
    const FieldFluids f = field_begin(fluid_mask, 0, "salva_hip_get_fluid_bounds");
    // six ordered integers and, behind them, the 64-bit count
    struct { int32_t box[6]; unsigned long long count; } host = {{INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN}, 0ull};
    static_assert(sizeof(host) == 32 && offsetof(decltype(host), count) == 24, "box and count, packed");
    srf.box.ensure(8);
    SALVA_HIP_CHECK(hipMemcpyAsync(srf.box.p, &host, sizeof(host), hipMemcpyHostToDevice, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));  // (`host` is pageable and on this frame)
    launch_surface_bounds(st_pos.p, st_model.p, n, f.mask, srf.box.p, reinterpret_cast<unsigned long long*>(srf.box.p + 6), stream);
    SALVA_HIP_CHECK(hipMemcpyAsync(&host, srf.box.p, sizeof(host), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    for (int a = 0; a < 3; ++a) {
        const bool any = host.box[a] <= host.box[3 + a];
        lo[a] = any ? field_unordered(host.box[a]) : INFINITY;
        hi[a] = any ? field_unordered(host.box[3 + a]) : -INFINITY;
    }
    *nfinite = host.count;
}

}  // namespace salva

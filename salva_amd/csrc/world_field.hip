// world_field.hip — SPH fields at points and on a lattice (salva_hip_evaluate_fields / _lattice): what a query must
// be, the box of the query and the evaluator's own grid over it, the buffers of the caller (host memory goes through the transfer
// helpers), and which of the two kernels of field.hip a lattice takes.  Nothing here writes anything a step reads.
#include "world.h"
#include "dcs.h"

#include <cmath>
#include <cstring>

namespace salva {

void scan_u32(void* temp, size_t temp_bytes, const uint32_t* in, uint32_t* out, uint32_t n, hipStream_t s);  // grid.hip

// The dispatch of a lattice: the brick kernel at spacing <= FIELD_CROSSOVER * h, one lane per node above.  MEASURED
// (tools/field_bench.py, profiles/field_bench.json): on the MI355X at 10^6 particles the lane-per-node kernel is the
// faster one at every spacing tried, r included (2.90 against 3.43 ms for five fields on 7 x 10^6 nodes), so the crossover is 0 and
// the brick kernel runs only where SALVA_HIP_FIELD_ARM=lattice asks for it.
constexpr float FIELD_CROSSOVER = 0.0f;

FieldFluids World::field_begin(uint32_t fluid_mask, uint32_t flags, const char* what) {
    use_device();
    const std::string w(what);
    if (comm) throw HipError(SALVA_HIP_E_INVALID, w + ": not available in a decomposed world (salva_hip_set_domain): host-order arrays are not maintained there");
    if (in_force_cb || in_dforce_cb || in_coupling_cb) throw HipError(SALVA_HIP_E_INVALID, w + ": not available inside a callback of a step");
    if (flags & ~(uint32_t)(SALVA_HIP_FIELD_POINTS_ON_DEVICE | SALVA_HIP_FIELD_OUT_ON_DEVICE)) throw HipError(SALVA_HIP_E_INVALID, w + ": unknown flag");
    FieldFluids f{};
    for (uint32_t s = 0; s < fluids.size() && s < FIELD_MAX_SLOTS; ++s) {
        f.density0[s] = fluids[s].density0;
        if ((fluid_mask >> s) & 1u) f.mask |= 1u << s;
    }
    if (!f.mask) throw HipError(SALVA_HIP_E_INVALID, w + ": fluid_mask selects no existing fluid");
    ensure_staging_current();
    return f;
}

// The evaluator's grid over [lo, hi] grown by h — one cell more on every side of the cells the box touches — and the selected
// particles inside it, sorted by cell, then by host index (rows: fld.rows gets the host-order row of each, for the ray casts)
FieldCandidates World::field_candidates(const FieldFluids& f, const float lo[3], const float hi[3], bool second, FieldGrid& g, bool rows) {
    return field_table(f, st_pos.p, sc.h, 1, lo, hi, second, g, rows, "field evaluation: the box of the query exceeds 2^27 cells of width h: split the query");
}

// The same table with its knobs out in the open: the rows of `pos` ((x, y, z, V) in host order: the staging positions, or the centres
// of world_anisotropy.hip) in cells of `width`, over the cells [lo, hi] touches and `grow` more on every side
FieldCandidates World::field_table(const FieldFluids& f, const float4* pos, float width, int grow, const float lo[3], const float hi[3], bool second,
                                   FieldGrid& g, bool rows_out, const char* too_large) {
    int clo[3], chi[3];
    cell_range(lo, hi, width, clo, chi);
    uint64_t ncells = 1;
    for (int a = 0; a < 3; ++a) {
        const uint64_t d = (uint64_t)((int64_t)chi[a] - (int64_t)clo[a] + 1 + 2 * grow);
        g.o[a] = clo[a] - grow;
        g.d[a] = (uint32_t)std::min<uint64_t>(d, 0xffffffffull);
        ncells = d > FIELD_MAX_CELLS || ncells * d > FIELD_MAX_CELLS ? FIELD_MAX_CELLS + 1 : ncells * d;
    }
    if (ncells > FIELD_MAX_CELLS) throw HipError(SALVA_HIP_E_CAPACITY, too_large);
    g.ncells = (uint32_t)ncells;
    g.h = width;
    const size_t rows = n ? n : 1;
    fld.keys.ensure(rows, stream, false, 1.1f); fld.rank.ensure(rows, stream, false, 1.1f);
    fld.keys_sorted.ensure(rows, stream, false, 1.1f); fld.idx_tmp.ensure(rows, stream, false, 1.1f);
    fld.rec0.ensure(rows, stream, false, 1.1f);
    if (second) fld.rec1.ensure(rows, stream, false, 1.1f);
    if (rows_out) fld.rows.ensure(rows, stream, false, 1.1f);
    fld.cells.ensure((size_t)g.ncells + 1, stream, false, 1.1f);
    const size_t tb = scan_temp_bytes(g.ncells + 1u);
    fld.temp.ensure(tb ? tb : 1);
    SALVA_HIP_CHECK(hipMemsetAsync(fld.cells.p, 0, ((size_t)g.ncells + 1) * sizeof(uint32_t), stream));
    launch_field_keys(pos, st_model.p, n, f, g, fld.keys.p, fld.rank.p, fld.cells.p, stream);
    scan_u32(fld.temp.p, tb, fld.cells.p, fld.cells.p, g.ncells + 1u, stream);
    launch_field_sort(pos, st_vel.p, st_model.p, n, f, g, fld.keys.p, fld.rank.p, fld.cells.p, fld.keys_sorted.p, fld.idx_tmp.p, fld.rec0.p,
                      second ? fld.rec1.p : nullptr, rows_out ? fld.rows.p : nullptr, stream);
    return FieldCandidates{fld.cells.p, fld.rec0.p, second ? fld.rec1.p : nullptr};
}

RowPack World::rows_pack(const FieldFluids& f, uint64_t& total) const {
    RowPack pk{};
    pk.mask = f.mask;
    total = 0;
    for (uint32_t s = 0; s < fluids.size() && s < FIELD_MAX_SLOTS; ++s) {
        if (!((f.mask >> s) & 1u)) continue;
        const SlotSpan sp = fluid_span(s);
        pk.first[s] = (uint32_t)sp.off;
        pk.len[s] = (uint32_t)sp.n;
        pk.base[s] = (uint32_t)total;
        total += sp.n;
    }
    return pk;
}

// m places, their box (box_empty: none of them is finite — everything is zero), the caller's buffers
void World::field_run(const FieldFluids& f, const FieldQuery& q, const float lo[3], const float hi[3], bool box_empty, uint64_t m, uint32_t flags,
                      const SalvaHipFieldOut& out, bool brick_arm) {
    QueryOut o{{{out.density, m}, {out.fraction, m}, {out.velocity, 3 * m}, {out.gradient, 3 * m}, {out.count, m}}};
    query_place(o, (flags & SALVA_HIP_FIELD_OUT_ON_DEVICE) != 0u);
    if (!o.any()) return;
    if (box_empty) {
        query_zero(o);
    } else {
        const bool second = out.fraction || out.velocity;
        FieldGrid g{};
        const FieldCandidates cand = field_candidates(f, lo, hi, second, g);
        const FieldOutDev od{o.f32(0), o.f32(1), o.f32(2), o.f32(3), o.u32(4)};
        SphConsts c = sc;
        if (brick_arm) launch_field_lattice(q, g, cand, c, od, stream);
        else launch_field_points(q, g, cand, c, od, stream);
    }
    query_finish(o);
}

// npoints > 0 places of the caller's: where the kernels read them, and the box of the finite ones (lo > hi: none is finite)
FieldQuery World::field_points_query(uint64_t npoints, const float* points_xyz, uint32_t flags, float lo[3], float hi[3], const char* what) {
    const std::string w(what);
    if (!points_xyz) throw HipError(SALVA_HIP_E_INVALID, w + ": null points");
    if (npoints > (1ull << 32)) throw HipError(SALVA_HIP_E_CAPACITY, w + ": more than 2^32 points: split the query");
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    FieldQuery q{};
    q.npoints = npoints;
    if (flags & SALVA_HIP_FIELD_POINTS_ON_DEVICE) {
        // the box of the finite points, reduced where they are
        q.pts = points_xyz;
        fld.box.ensure(6);
        const int32_t init[6] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN};
        int32_t got[6];
        SALVA_HIP_CHECK(hipMemcpyAsync(fld.box.p, init, sizeof(init), hipMemcpyHostToDevice, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));  // (`init` is pageable and on this frame)
        launch_field_bbox(q.pts, npoints, fld.box.p, stream);
        SALVA_HIP_CHECK(hipMemcpyAsync(got, fld.box.p, sizeof(got), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
        for (int a = 0; a < 3; ++a)
            if (got[a] <= got[3 + a]) { lo[a] = field_unordered(got[a]); hi[a] = field_unordered(got[3 + a]); }
    } else {
        for (uint64_t i = 0; i < npoints; ++i) {
            const float* p = points_xyz + 3 * i;
            if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]); }
        }
        q.pts = stage_floats(points_xyz, 3 * npoints);  // (scratch_f: free again once the kernels of the call have run — every path waits)
    }
    return q;
}

void World::evaluate_fields(uint32_t fluid_mask, uint64_t npoints, const float* points_xyz, uint32_t flags, const SalvaHipFieldOut& out) {
    const FieldFluids f = field_begin(fluid_mask, flags, "salva_hip_evaluate_fields");
    if (npoints == 0) return;
    float lo[3], hi[3];
    const FieldQuery q = field_points_query(npoints, points_xyz, flags, lo, hi, "salva_hip_evaluate_fields");
    const bool box_empty = !(lo[0] <= hi[0]);
    field_run(f, q, lo, hi, box_empty, npoints, flags, out, false);
    if (!(flags & SALVA_HIP_FIELD_POINTS_ON_DEVICE)) SALVA_HIP_CHECK(hipStreamSynchronize(stream));
}

// the nodes of a lattice, their box, and whether no node is finite
FieldQuery World::field_lattice_query(const float origin[3], float spacing, const uint32_t dims[3], float lo[3], float hi[3], bool& box_empty,
                                      const char* what) {
    const std::string w(what);
    if (!(std::isfinite(spacing) && spacing > 0.0f)) throw HipError(SALVA_HIP_E_INVALID, w + ": spacing must be finite and > 0");
    if (!dims[0] || !dims[1] || !dims[2]) throw HipError(SALVA_HIP_E_INVALID, w + ": every dimension must be at least 1");
    const uint64_t xy = (uint64_t)dims[0] * dims[1];
    if (xy > (1ull << 32) || xy * dims[2] > (1ull << 32)) throw HipError(SALVA_HIP_E_CAPACITY, w + ": more than 2^32 nodes: split the query");
    const uint64_t m = xy * dims[2];
    FieldQuery q{};
    q.npoints = m;
    q.spacing = spacing;
    box_empty = false;
    for (int a = 0; a < 3; ++a) {
        q.origin[a] = origin[a]; q.dims[a] = dims[a];
        // the first and the last node of the axis, as the kernels compute them
        volatile float step = (float)(dims[a] - 1u) * spacing;
        lo[a] = origin[a]; hi[a] = origin[a] + step;
        if (!std::isfinite(origin[a])) box_empty = true;  // no node is finite
    }
    if (!box_empty)
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(hi[a])) throw HipError(SALVA_HIP_E_CAPACITY, w + ": the lattice leaves the range of f32: split the query");
    return q;
}

void World::evaluate_fields_lattice(uint32_t fluid_mask, const float origin[3], float spacing, const uint32_t dims[3], uint32_t flags,
                                    const SalvaHipFieldOut& out) {
    const FieldFluids f = field_begin(fluid_mask, flags, "salva_hip_evaluate_fields_lattice");
    float lo[3], hi[3];
    bool box_empty = false;
    const FieldQuery q = field_lattice_query(origin, spacing, dims, lo, hi, box_empty, "salva_hip_evaluate_fields_lattice");
    const uint64_t m = q.npoints;
    const bool brick_arm = sw.field_arm == 2 || (sw.field_arm == 0 && FIELD_CROSSOVER > 0.0f && spacing <= FIELD_CROSSOVER * sc.h);
    field_run(f, q, lo, hi, box_empty, m, flags, out, brick_arm);
}

}  // namespace salva

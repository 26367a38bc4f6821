// world_diffuse.hip — diffuse particles.  The potentials (salva_hip_diffuse_potentials): what the parameters must be,
// the table of cells of width h over the fluids' box — built by the field evaluator's table code (world_field.hip field_table) —, the
// two passes over it and the buffers of the caller.  The sets (salva_hip_create_diffuse ... salva_hip_update_diffuse): their arrays, and
// an update as advect - remove - emit on that one table.  Nothing here writes anything a step reads.
#include "world.h"

#include <cmath>
#include <cstring>

namespace salva {

void scan_u32(void* temp, size_t temp_bytes, const uint32_t* in, uint32_t* out, uint32_t n, hipStream_t s);  // grid.hip

static_assert(sizeof(SalvaHipDiffuseStats) == SALVA_HIP_DIFFUSE_STATS_BYTES, "SalvaHipDiffuseStats: the header's size constant");
static_assert(sizeof(SalvaHipDiffuse) == SALVA_HIP_DIFFUSE_BYTES, "SalvaHipDiffuse: the header's size constant is what the mirrors check");

DiffuseParams World::diffuse_params(const SalvaHipDiffuse* p, const char* what) const {
    const std::string w(what);
    auto refuse = [&](const char* why) { throw HipError(SALVA_HIP_E_INVALID, w + ": " + why); };
    if (!p) refuse("null params");
    if (p->struct_size != SALVA_HIP_DIFFUSE_BYTES || p->version != SALVA_HIP_DIFFUSE_VERSION)
        refuse("params with a struct_size / version other than this library's");
    if (!(std::isfinite(p->surface_min) && p->surface_min >= 0.0f)) refuse("surface_min must be finite and >= 0");
    if (!(p->crest_cos >= -1.0f && p->crest_cos <= 1.0f)) refuse("crest_cos must lie in [-1, 1]");
    const float range[3][2] = {{p->ta_lo, p->ta_hi}, {p->wc_lo, p->wc_hi}, {p->en_lo, p->en_hi}};
    for (const auto& r : range)
        if (!(r[0] >= 0.0f && r[0] < r[1] && std::isfinite(r[1]))) refuse("a clamp range needs 0 <= lo < hi, finite");
    if (!(std::isfinite(p->k_ta) && p->k_ta >= 0.0f && std::isfinite(p->k_wc) && p->k_wc >= 0.0f)) refuse("k_ta and k_wc must be finite and >= 0");
    if (p->max_per_particle > SALVA_HIP_DIFFUSE_MAX_PER_PARTICLE) refuse("max_per_particle above SALVA_HIP_DIFFUSE_MAX_PER_PARTICLE");
    if (p->n_spray > p->n_bubble) refuse("n_spray must not exceed n_bubble");
    if (!std::isfinite(p->k_b)) refuse("k_b must be finite");
    if (!(p->k_d >= 0.0f && p->k_d <= 1.0f)) refuse("k_d must lie in [0, 1]");
    if (!(p->life_lo >= 0.0f && p->life_lo <= p->life_hi && std::isfinite(p->life_hi))) refuse("lifetimes need 0 <= lo <= hi, finite");
    if (p->has_kill_box > 1u) refuse("has_kill_box must be 0 or 1");
    DiffuseParams d{p->surface_min, p->crest_cos, p->ta_lo, p->ta_hi, p->wc_lo, p->wc_hi, p->en_lo, p->en_hi, p->k_ta, p->k_wc, p->max_per_particle,
                    p->n_spray, p->n_bubble, p->k_b, p->k_d, p->life_lo, p->life_hi, p->seed, p->has_kill_box, {}, {}, {}};
    for (int a = 0; a < 3; ++a) {
        if (std::isnan(p->kill_lo[a]) || std::isnan(p->kill_hi[a])) refuse("a NaN in the kill box");
        if (p->has_kill_box && !(p->kill_lo[a] <= p->kill_hi[a])) refuse("kill_lo must not exceed kill_hi");
        if (!std::isfinite(p->gravity[a])) refuse("gravity must be finite");
        d.kill_lo[a] = p->kill_lo[a]; d.kill_hi[a] = p->kill_hi[a]; d.gravity[a] = p->gravity[a];
    }
    return d;
}

// the rows the passes write, zeroed: every row of the staging arrays that has no part in a call keeps zeros
DiffuseRows World::diffuse_rows() {
    const size_t rows = n ? n : 1;
    dif.a.ensure(rows, stream, false, 1.1f); dif.normal.ensure(rows, stream, false, 1.1f); dif.normal_sorted.ensure(rows, stream, false, 1.1f);
    const DiffuseRows r{dif.a.p, dif.normal.p, dif.normal_sorted.p};
    SALVA_HIP_CHECK(hipMemsetAsync(r.a, 0, rows * sizeof(float4), stream));
    SALVA_HIP_CHECK(hipMemsetAsync(r.normal, 0, rows * sizeof(float4), stream));
    SALVA_HIP_CHECK(hipMemsetAsync(r.normal_sorted, 0, rows * sizeof(float4), stream));
    return r;
}
// the table over the fluids' own box; false: no particle is finite (second: with the (v, V) records)
bool World::diffuse_table(const FieldFluids& f, FieldGrid& g, FieldCandidates& cand, bool second) {
    float lo[3], hi[3];
    uint64_t nfinite = 0;
    get_fluid_bounds(f.mask, lo, hi, &nfinite);
    if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) return false;
    cand = field_table(f, st_pos.p, sc.h, 1, lo, hi, second, g, true, "diffuse particles: the fluids' box exceeds 2^27 cells of width h");
    return true;
}
// the two passes
DiffuseRows World::diffuse_sums(const FieldFluids& f, const DiffuseParams& prm, uint32_t want) {
    const DiffuseRows r = diffuse_rows();
    FieldGrid g{};
    FieldCandidates cand{};
    if (!diffuse_table(f, g, cand, (want & ~(uint32_t)DIFFUSE_WANT_COUNT) != 0u)) return r;  // ((v, V): every output but the count reads it)
    launch_diffuse_sums(n, g, cand, fld.rows.p, sc, prm, want, r, stream);
    if (want & DIFFUSE_WANT_CREST) launch_diffuse_crest(n, g, cand, fld.rows.p, sc, prm, r, stream);
    return r;
}

void World::diffuse_potentials(uint32_t fluid_mask, const SalvaHipDiffuse* params, uint32_t flags, const SalvaHipDiffusePotentialsOut* out,
                               uint64_t* nrows) {
    const char* what = "salva_hip_diffuse_potentials";
    *nrows = 0;
    const FieldFluids f = field_begin(fluid_mask, 0, what);
    if (flags & ~(uint32_t)SALVA_HIP_DIFFUSE_OUT_ON_DEVICE) throw HipError(SALVA_HIP_E_INVALID, std::string(what) + ": unknown flag");
    const DiffuseParams prm = diffuse_params(params, what);
    uint64_t total = 0;
    const RowPack pk = rows_pack(f, total);
    if (!fill_wanted(total, nrows, out, what, "rows")) return;
    const uint32_t want = (out->count ? DIFFUSE_WANT_COUNT : 0u) | (out->trapped_air ? DIFFUSE_WANT_TRAPPED : 0u) |
                          (out->normal ? DIFFUSE_WANT_NORMAL : 0u) | (out->wave_crest ? DIFFUSE_WANT_CREST : 0u) |
                          (out->energy ? DIFFUSE_WANT_ENERGY : 0u);
    if (!total || !want) return;
    const DiffuseRows r = diffuse_sums(f, prm, want);
    QueryOut o{{{out->trapped_air, total}, {out->wave_crest, total}, {out->energy, total}, {out->normal, 3 * total}, {out->count, total}}};
    query_place(o, (flags & SALVA_HIP_DIFFUSE_OUT_ON_DEVICE) != 0u);
    launch_diffuse_pack(n, st_model.p, pk, r, o.f32(0), o.f32(1), o.f32(2), o.f32(3), o.u32(4), stream);
    query_finish(o);
}

// ------------------------------------------------------------------------------------------------ the sets
World::DiffuseSet& World::diffuse_set(uint32_t set, const char* what) {
    if (set >= diffuse_sets.size() || !diffuse_sets[set] || !diffuse_sets[set]->live)
        throw HipError(SALVA_HIP_E_INVALID, std::string(what) + ": no such diffuse set (never created, or destroyed)");
    return *diffuse_sets[set];
}

uint32_t World::create_diffuse(uint64_t capacity) {
    use_device();
    if (capacity == 0 || capacity > 0x7fffffffull) throw HipError(SALVA_HIP_E_INVALID, "salva_hip_create_diffuse: capacity must lie in [1, 2^31 - 1]");
    auto s = std::make_unique<DiffuseSet>();
    s->live = true;
    s->capacity = (uint32_t)capacity;
    for (int k = 0; k < 2; ++k) { s->pos[k].ensure(capacity); s->vel[k].ensure(capacity); s->id[k].ensure(capacity); }
    diffuse_sets.push_back(std::move(s));
    return (uint32_t)diffuse_sets.size() - 1u;
}

void World::destroy_diffuse(uint32_t set) {
    use_device();
    diffuse_set(set, "salva_hip_destroy_diffuse");
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    diffuse_sets[set].reset();
}

void World::clear_diffuse(uint32_t set) {
    DiffuseSet& s = diffuse_set(set, "salva_hip_clear_diffuse");
    s.count = 0;
    s.stats.count = 0;
    for (uint64_t& k : s.stats.kinds) k = 0;
}

void World::add_diffuse(uint32_t set, uint64_t count, const float* positions, const float* velocities, const float* lifetimes, uint32_t flags) {
    const char* what = "salva_hip_add_diffuse";
    use_device();
    DiffuseSet& s = diffuse_set(set, what);
    if (flags & ~(uint32_t)SALVA_HIP_DIFFUSE_IN_ON_DEVICE) throw HipError(SALVA_HIP_E_INVALID, std::string(what) + ": unknown flag");
    if (count == 0) return;
    if (!positions || !velocities) throw HipError(SALVA_HIP_E_INVALID, std::string(what) + ": null positions or velocities");
    if (count > (uint64_t)(s.capacity - s.count))
        throw HipError(SALVA_HIP_E_CAPACITY, std::string(what) + ": " + std::to_string(count) + " particles: more than the room left in the set");
    const uint32_t m = (uint32_t)count;
    const float *d_pos = positions, *d_vel = velocities, *d_life = lifetimes;
    if (!(flags & SALVA_HIP_DIFFUSE_IN_ON_DEVICE)) {
        dif.in.ensure(7 * (size_t)m, stream, false, 1.1f);
        SALVA_HIP_CHECK(hipMemcpyAsync(dif.in.p, positions, 3 * (size_t)m * sizeof(float), hipMemcpyHostToDevice, stream));
        SALVA_HIP_CHECK(hipMemcpyAsync(dif.in.p + 3 * (size_t)m, velocities, 3 * (size_t)m * sizeof(float), hipMemcpyHostToDevice, stream));
        if (lifetimes) SALVA_HIP_CHECK(hipMemcpyAsync(dif.in.p + 6 * (size_t)m, lifetimes, (size_t)m * sizeof(float), hipMemcpyHostToDevice, stream));
        d_pos = dif.in.p; d_vel = dif.in.p + 3 * (size_t)m; d_life = lifetimes ? dif.in.p + 6 * (size_t)m : nullptr;
    }
    SalvaHipDiffuse def;
    salva_hip_default_diffuse(&def);
    launch_diffuse_add(m, d_pos, d_vel, d_life, def.life_hi, s.count, s.next_id, s.dev(s.cur), stream);
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));  // (the caller's buffers are free again)
    s.count += m;
    s.next_id += m;
    s.stats.count = s.count;
    s.stats.kinds[SALVA_HIP_DIFFUSE_NEW] += m;
}

void World::get_diffuse(uint32_t set, uint32_t flags, const SalvaHipDiffuseOut* out, uint64_t* count) {
    const char* what = "salva_hip_get_diffuse";
    use_device();
    *count = 0;
    DiffuseSet& s = diffuse_set(set, what);
    if (flags & ~(uint32_t)SALVA_HIP_DIFFUSE_OUT_ON_DEVICE) throw HipError(SALVA_HIP_E_INVALID, std::string(what) + ": unknown flag");
    const uint64_t total = s.count;
    if (!fill_wanted(total, count, out, what, "particles")) return;
    if (!total || !(out->positions || out->velocities || out->lifetime || out->kind || out->id)) return;
    QueryOut o{{{out->positions, 3 * total}, {out->velocities, 3 * total}, {out->lifetime, total}, {out->kind, total}, {out->id, total}}};
    query_place(o, (flags & SALVA_HIP_DIFFUSE_OUT_ON_DEVICE) != 0u);
    launch_diffuse_get((uint32_t)total, s.dev(s.cur), o.f32(0), o.f32(1), o.f32(2), o.u32(3), o.u32(4), stream);
    query_finish(o);
}

void World::get_diffuse_stats(uint32_t set, SalvaHipDiffuseStats* stats) { *stats = diffuse_set(set, "salva_hip_get_diffuse_stats").stats; }

void World::update_diffuse(uint32_t set, uint32_t fluid_mask, const SalvaHipDiffuse* params, float dt) {
    const char* what = "salva_hip_update_diffuse";
    const FieldFluids f = field_begin(fluid_mask, 0, what);
    DiffuseSet& s = diffuse_set(set, what);
    const DiffuseParams prm = diffuse_params(params, what);
    if (!(std::isfinite(dt) && dt >= 0.0f)) throw HipError(SALVA_HIP_E_INVALID, std::string(what) + ": dt must be finite and >= 0");
    uint64_t total = 0;
    const RowPack pk = rows_pack(f, total);
    // one table serves the evaluator at the diffuse particles and both passes of the potentials: the fluid does not change in between
    const DiffuseRows rows = diffuse_rows();
    FieldGrid g{};
    FieldCandidates cand{};
    const bool table = diffuse_table(f, g, cand, true);
    dif.counters.ensure(1);
    SALVA_HIP_CHECK(hipMemsetAsync(dif.counters.p, 0, sizeof(DiffuseCounters), stream));
    const uint32_t m = s.count;
    if (m) {
        // a. advect and age
        dif.pts.ensure(3 * (size_t)m, stream, false, 1.1f); dif.fv.ensure(3 * (size_t)m, stream, false, 1.1f);
        dif.fc.ensure(m, stream, false, 1.1f); dif.keep.ensure(m, stream, false, 1.1f); dif.keep_off.ensure(m, stream, false, 1.1f);
        if (table) {
            launch_diffuse_set_points(m, s.dev(s.cur), dif.pts.p, stream);
            FieldQuery q{};
            q.pts = dif.pts.p;
            q.npoints = m;
            launch_field_points(q, g, cand, sc, FieldOutDev{nullptr, nullptr, dif.fv.p, nullptr, dif.fc.p}, stream);
        } else {
            SALVA_HIP_CHECK(hipMemsetAsync(dif.fv.p, 0, 3 * (size_t)m * sizeof(float), stream));
            SALVA_HIP_CHECK(hipMemsetAsync(dif.fc.p, 0, (size_t)m * sizeof(uint32_t), stream));
        }
        launch_diffuse_advect(m, s.dev(s.cur), dif.fv.p, dif.fc.p, prm, dt, dif.keep.p, dif.counters.p, stream);
        // b. remove, stably
        const size_t tb = scan_temp_bytes(m);
        dif.temp.ensure(tb ? tb : 1);
        scan_u32(dif.temp.p, tb, dif.keep.p, dif.keep_off.p, m, stream);
        launch_diffuse_compact(m, dif.keep.p, dif.keep_off.p, s.dev(s.cur), s.dev(s.cur ^ 1u), dif.counters.p, stream);
        s.cur ^= 1u;
    }
    // c. emit
    if (table && total) {
        launch_diffuse_sums(n, g, cand, fld.rows.p, sc, prm, DIFFUSE_WANT_TRAPPED | DIFFUSE_WANT_CREST | DIFFUSE_WANT_ENERGY, rows, stream);
        launch_diffuse_crest(n, g, cand, fld.rows.p, sc, prm, rows, stream);
        DiffuseEmit em{};
        em.pk = pk;
        em.total = (uint32_t)total;
        em.seed = prm.seed; em.updates = s.updates; em.first_id = s.next_id; em.capacity = s.capacity;
        em.radius = this->prm.particle_radius; em.dt = dt;
        dif.cnt.ensure(total, stream, false, 1.1f); dif.cnt_off.ensure(total, stream, false, 1.1f);
        launch_diffuse_rate(n, st_pos.p, st_vel.p, st_model.p, rows, prm, em, dif.cnt.p, stream);
        const size_t tb = scan_temp_bytes((uint32_t)total);
        dif.temp.ensure(tb ? tb : 1);
        scan_u32(dif.temp.p, tb, dif.cnt.p, dif.cnt_off.p, (uint32_t)total, stream);
        launch_diffuse_emit(n, st_pos.p, st_vel.p, st_model.p, prm, em, dif.cnt.p, dif.cnt_off.p, s.dev(s.cur), dif.counters.p, stream);
    }
    // the one wait: what the update counted
    DiffuseCounters c{};
    SALVA_HIP_CHECK(hipMemcpyAsync(&c, dif.counters.p, sizeof(c), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    s.count = c.kept + c.emitted;
    s.next_id += c.emitted;
    s.updates += 1u;
    SalvaHipDiffuseStats& st = s.stats;
    st.count = s.count;
    for (int k = 0; k < 4; ++k) st.kinds[k] = c.kinds[k];
    st.emitted = c.emitted; st.dissolved = c.dissolved; st.killed = c.killed; st.dropped = c.dropped;
    st.total_emitted += c.emitted; st.total_dissolved += c.dissolved; st.total_killed += c.killed; st.total_dropped += c.dropped;
}

}  // namespace salva

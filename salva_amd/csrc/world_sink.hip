// world_sink.hip — deleting particles by region (salva_hip_delete_particles_in_region) and the sinks a step applies by itself
// (DESIGN.md §18): what a region must be, which rows its predicate walks, the one small read that says how many rows go, and the
// hand-over to the editor of the host-order arrays (World::apply_keep_flags, world_objects.hip).  The kernels are sink.hip.
#include "world.h"
#include "dcs.h"

#include <cmath>
#include <cstring>

namespace salva {

World::RegionRes World::resolve_region(const SalvaHipRegion& g) const {
    if (g.struct_size != SALVA_HIP_REGION_BYTES || g.version != SALVA_HIP_REGION_VERSION)
        throw HipError(SALVA_HIP_E_INVALID, "region: struct_size / version are not this library's SalvaHipRegion (SALVA_HIP_REGION_BYTES, SALVA_HIP_REGION_VERSION)");
    if (g.flags & ~(uint32_t)SALVA_HIP_REGION_INVERT) throw HipError(SALVA_HIP_E_INVALID, "region: unknown flag (only SALVA_HIP_REGION_INVERT)");
    if (g.kind < SALVA_HIP_REGION_HALFSPACE || g.kind > SALVA_HIP_REGION_COMPOUND) throw HipError(SALVA_HIP_E_INVALID, "region: unknown kind");
    if (!(std::isfinite(g.margin) && g.margin >= 0.0f)) throw HipError(SALVA_HIP_E_INVALID, "region: the margin must be finite and >= 0");
    RegionRes r;
    SinkRegionDev& d = r.dev;
    d.kind = g.kind; d.invert = (g.flags & SALVA_HIP_REGION_INVERT) ? 1u : 0u; d.margin = g.margin;
    d.q[3] = 1.0f;
    if (g.kind == SALVA_HIP_REGION_HALFSPACE) {
        float nn = 0.0f;
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(g.point[a]) || !std::isfinite(g.normal[a])) throw HipError(SALVA_HIP_E_INVALID, "region: non-finite point or normal of a half-space");
            nn += g.normal[a] * g.normal[a];
            d.a[a] = g.point[a]; d.b[a] = g.normal[a];
        }
        if (fabsf(nn - 1.0f) > 1.0e-3f) throw HipError(SALVA_HIP_E_INVALID, "region: the normal of a half-space must be a unit vector");
        return r;
    }
    if (g.kind == SALVA_HIP_REGION_AABB) {
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(g.mins[a]) || !std::isfinite(g.maxs[a])) throw HipError(SALVA_HIP_E_INVALID, "region: non-finite box");
            if (!(g.mins[a] <= g.maxs[a])) throw HipError(SALVA_HIP_E_INVALID, "region: mins > maxs");
            d.a[a] = g.mins[a]; d.b[a] = g.maxs[a];
        }
        return r;
    }
    // a posed geometry, checked in the order of the shape query (World::particles_in, world_query.hip)
    if (g.kind == SALVA_HIP_REGION_SHAPE) shape_param_count(g.shape.kind);
    r.geom = g.kind == SALVA_HIP_REGION_SHAPE ? geom_of(g.shape)
                                              : geom_of(g.kind == SALVA_HIP_REGION_MESH ? SALVA_HIP_SHAPE_MESH : SALVA_HIP_SHAPE_COMPOUND, g.handle);
    check_solid(r.geom, "region");
    check_pose(g.translation, g.rotation_ijkw, "region");
    if (g.kind == SALVA_HIP_REGION_SHAPE) {
        check_shape_params(g.shape, "region: radius / half extents must be positive and finite");
        d.shape_kind = g.shape.kind;
        for (int a = 0; a < 3; ++a) d.p[a] = g.shape.params[a];
    }
    for (int a = 0; a < 3; ++a) d.t[a] = g.translation[a];
    for (int a = 0; a < 4; ++a) d.q[a] = g.rotation_ijkw[a];
    return r;
}

// Tests the positions as they are against `count` regions, applied in order to the same positions, and removes what they select:
// region k takes what it selects of fluid slots[k] among the rows the regions before it left, and deleted[k] says how many those are.
// The predicates first walk the particles where they lie — the sorted working set after a step, the host-order arrays otherwise — into
// one flag array, and the per-region, per-fluid counts come back in ONE small read, whatever `count` is: an edit that selects nothing
// ends there, having written scratch only.  Otherwise the host-order arrays are brought up to date, the predicates write the flags
// again in their order, and the editor finishes.  deleted_mask (one region only): the bytes of the rows [sp.off, sp.off + sp.n).
uint64_t World::delete_in_regions(uint32_t count, const RegionRes* const* rs, const uint32_t* slots, uint64_t* deleted, uint8_t* deleted_mask,
                                  SlotSpan sp) {
    for (uint32_t k = 0; k < count; ++k) deleted[k] = 0;
    if (n == 0 || count == 0) return 0;
    sink_keep.ensure(n, stream, false, 1.1f);
    sink_deleted.ensure((size_t)count * SINK_MAX_SLOTS);
    const size_t words = (size_t)count * SINK_MAX_SLOTS;
    auto enqueue = [&](const float4* pos, const uint32_t* mdl, bool tally) {
        for (uint32_t k = 0; k < count; ++k) {
            const RegionRes& r = *rs[k];
            const Geom& g = r.geom;
            const MeshDev mesh = g.mesh ? g.mesh->dev() : MeshDev{};
            launch_sink_predicate(SinkSrc{pos, mdl, n, slots[k], k ? 1u : 0u}, r.dev, g.mesh ? &mesh : nullptr, g.parts(), g.nparts(), sink_keep.p,
                                  tally ? sink_deleted.p + (size_t)k * SINK_MAX_SLOTS : nullptr, stream);
        }
    };
    const bool on_sorted = !staging_current && sorted_valid;
    SALVA_HIP_CHECK(hipMemsetAsync(sink_deleted.p, 0, words * sizeof(uint32_t), stream));
    if (on_sorted) enqueue(posm[cur].p, model[cur].p, true);
    else enqueue(st_pos.p, st_model.p, true);
    uint32_t per_slot[SINK_MAX_SLOTS] = {};
    uint64_t total = 0;
    {   // the one small read
        const uint32_t* h = reinterpret_cast<const uint32_t*>(sink_stage.acquire(words * sizeof(uint32_t)));
        SALVA_HIP_CHECK(hipMemcpyAsync(const_cast<uint32_t*>(h), sink_deleted.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
        for (uint32_t k = 0; k < count; ++k)
            for (uint32_t s = 0; s < SINK_MAX_SLOTS; ++s) { deleted[k] += h[(size_t)k * SINK_MAX_SLOTS + s]; per_slot[s] += h[(size_t)k * SINK_MAX_SLOTS + s]; }
    }
    for (uint32_t k = 0; k < count; ++k) total += deleted[k];
    if (total == 0) {
        if (deleted_mask) memset(deleted_mask, 0, (size_t)sp.n);
        return 0;
    }
    if (on_sorted) {
        // the flags again, in host order: the same positions in another order select the same rows, so the counts stand (and the
        // compaction writes no row beyond the room cut from them, whatever the flags say)
        ensure_staging_current();
        enqueue(st_pos.p, st_model.p, false);
    }
    if (deleted_mask && sp.n) {  // (on the world's stream, behind the predicates that wrote the flags; the stream does not block the null stream)
        SALVA_HIP_CHECK(hipMemcpyAsync(deleted_mask, sink_keep.p + sp.off, (size_t)sp.n, hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
        for (uint64_t k = 0; k < sp.n; ++k) deleted_mask[k] = deleted_mask[k] ? 0 : 1;
    }
    apply_keep_flags(sink_keep.p, per_slot);
    return total;
}

int64_t World::delete_particles_in_region(const SalvaHipRegion& region, uint32_t slot, uint8_t* deleted_mask) {
    use_device();
    if (comm && dist_started) throw HipError(SALVA_HIP_E_INVALID, "host indices do not exist in a running multi-GPU world: delete by global id (salva_hip_delete_owned)");
    SlotSpan sp{n, 0};
    if (slot != SALVA_HIP_ALL_FLUIDS) sp = fluid_span(slot);
    const RegionRes r = resolve_region(region);
    const RegionRes* rp = &r;
    uint64_t deleted = 0;
    return (int64_t)delete_in_regions(1, &rp, &slot, &deleted, deleted_mask, sp);
}

// ------------------------------------------------------------------------------------------------ sinks
World::Sink& World::sink_at(uint32_t sink) {
    if (sink >= sinks.size() || !sinks[sink].live) throw HipError(SALVA_HIP_E_INVALID, "no such sink");
    return sinks[sink];
}
uint32_t World::add_sink(const SalvaHipRegion& region, uint32_t slot) {
    use_device();
    if (comm) throw HipError(SALVA_HIP_E_INVALID, "sinks are not available in a decomposed world (salva_hip_set_domain): delete by global id (salva_hip_delete_owned)");
    if (slot != SALVA_HIP_ALL_FLUIDS) fluid_span(slot);
    Sink s;
    s.live = true; s.res = resolve_region(region); s.slot = slot;
    uint32_t h = 0;
    while (h < sinks.size() && sinks[h].live) ++h;
    if (h == sinks.size()) sinks.emplace_back();
    sinks[h] = std::move(s);
    return h;
}
void World::remove_sink(uint32_t sink) {
    sink_at(sink);
    sinks[sink] = Sink{};
}
void World::set_sink_pose(uint32_t sink, const float t[3], const float q[4]) {
    Sink& s = sink_at(sink);
    if (s.res.dev.kind < SALVA_HIP_REGION_SHAPE) throw HipError(SALVA_HIP_E_INVALID, "a half-space or box sink has no pose");
    check_pose(t, q, "region");
    for (int a = 0; a < 3; ++a) s.res.dev.t[a] = t[a];
    for (int a = 0; a < 4; ++a) s.res.dev.q[a] = q[a];
}
void World::get_sink_stats(uint32_t sink, uint64_t out[2]) const {
    if (sink >= sinks.size() || !sinks[sink].live) throw HipError(SALVA_HIP_E_INVALID, "no such sink");
    out[0] = sinks[sink].last; out[1] = sinks[sink].total;
}
// remove_fluid is a swap-remove (world_objects.hip): the sinks of the removed fluid go with it, those of the fluid that takes its
// slot follow it there
void World::sinks_after_remove_fluid(uint32_t slot, uint32_t last) {
    for (Sink& s : sinks) {
        if (!s.live || s.slot == SALVA_HIP_ALL_FLUIDS) continue;
        if (s.slot == slot) s = Sink{};
        else if (s.slot == last) s.slot = slot;
    }
}
// the start of a step (World::step): every sink, in handle order, on the positions at step entry — one edit, one host wait
void World::apply_sinks() {
    std::vector<Sink*> live;
    for (Sink& s : sinks)
        if (s.live) live.push_back(&s);
    if (live.empty()) return;
    if (comm) throw HipError(SALVA_HIP_E_INVALID, "sinks are not available in a decomposed world (salva_hip_set_domain): remove them (salva_hip_remove_sink)");
    std::vector<const RegionRes*> rs;
    std::vector<uint32_t> slots;
    std::vector<uint64_t> deleted(live.size(), 0);
    for (Sink* s : live) {
        s->last = 0;
        if (s->slot != SALVA_HIP_ALL_FLUIDS) fluid_span(s->slot);
        rs.push_back(&s->res);
        slots.push_back(s->slot);
    }
    delete_in_regions((uint32_t)live.size(), rs.data(), slots.data(), deleted.data(), nullptr, SlotSpan{0, 0});
    for (size_t k = 0; k < live.size(); ++k) { live[k]->last = deleted[k]; live[k]->total += deleted[k]; }
}

}  // namespace salva

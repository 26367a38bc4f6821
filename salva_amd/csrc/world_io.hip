// world_io.hip — the read-backs and their write counterparts: host-order downloads (synchronous and asynchronous), the per-fluid
// fields, the local view, the contact exports, the host force callback's state and accelerations, Becker2009Elasticity's state.
// Host <-> device traffic happens only in set_* / get_*; the edits of the host-order arrays are world_objects.hip.
#include "world.h"

#include <algorithm>
#include <cstring>

namespace salva {

__global__ void k_unpack_xyz(uint32_t n, const float4* __restrict__ src, float* __restrict__ dst) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 s = src[i];
    dst[3 * i] = s.x; dst[3 * i + 1] = s.y; dst[3 * i + 2] = s.z;
}
__global__ void k_unpack_w(uint32_t n, const float4* __restrict__ src, float* __restrict__ dst) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) dst[i] = src[i].w;
}

// ------------------------------------------------------------------------------------------------ device -> host
// float4 rows -> packed xyz / their w / plain floats, into `out`.  Each waits for the stream: scratch_f is free again, and `out`
// is written, when it returns.
void World::download_f32(const float* src, uint64_t count, float* out) {
    SALVA_HIP_CHECK(hipMemcpyAsync(out, src, count * sizeof(float), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
}
// the outputs of a device query (world.h QueryOut)
void World::query_place(QueryOut& q, bool on_device) {
    q.on_device = on_device;
    uint64_t total = 0;
    for (const auto& e : q.o) total += e.host ? e.words : 0;
    if (!on_device) query_out.ensure(total ? total : 1, stream, false, 1.1f);
    uint64_t at = 0;
    for (auto& e : q.o) {
        if (!e.host) continue;
        e.dev = on_device ? static_cast<float*>(e.host) : query_out.p + at;
        at += e.words;
    }
}
void World::query_zero(const QueryOut& q) {
    for (const auto& e : q.o)
        if (e.dev) SALVA_HIP_CHECK(hipMemsetAsync(e.dev, 0, e.words * sizeof(float), stream));
}
void World::query_finish(const QueryOut& q) {
    if (q.on_device) {
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
        return;
    }
    for (const auto& e : q.o)
        if (e.dev && e.words) download_f32(e.dev, e.words, static_cast<float*>(e.host));
}
void World::download_xyz(const float4* src, uint64_t count, float* out) {
    scratch_f.ensure(3 * count, stream, false, 1.1f);
    k_unpack_xyz<<<nblk(count), BLOCK, 0, stream>>>((uint32_t)count, src, scratch_f.p);
    download_f32(scratch_f.p, 3 * count, out);
}
void World::download_w(const float4* src, uint64_t count, float* out) {
    scratch_f.ensure(count, stream, false, 1.1f);
    k_unpack_w<<<nblk(count), BLOCK, 0, stream>>>((uint32_t)count, src, scratch_f.p);
    download_f32(scratch_f.p, count, out);
}

// ------------------------------------------------------------------------------------------------ fluids, host order
void World::get_fluid(uint32_t slot, float* pos, float* vel_out) {
    use_device();
    const SlotSpan sp = fluid_span(slot);
    if (sp.n == 0) return;
    ensure_staging_current();
    if (pos) download_xyz(st_pos.p + sp.off, sp.n, pos);
    if (vel_out) download_xyz(st_vel.p + sp.off, sp.n, vel_out);
}

// ---- asynchronous read-back.  The reference's users read fluid.positions / velocities after every step
// (integrations/rapier/testbed_plugin.rs:361-367); the synchronous salva_hip_get_fluid costs 0.6 ms per step at 10^6 particles
// (un-sort into the staging arrays, unpack, copy, stream synchronisation, per array, serial with the step: 1.91 against 1.31 ms per
// step over the bench protocol, tools/pcie_probe.py — round 3's "5.57 ms" compared different steps of the scene).  Here: two scatter kernels on the main stream write (x, y, z) in host order straight from the sorted
// working set (~10 us), the copy stream takes them out behind an event while the main stream already runs the next step, and
// the host collects them with salva_hip_wait_download.  A destination in pinned memory (salva_hip_host_alloc / _register) is
// written by the DMA engine directly; a pageable one goes through the library's pinned buffers and one memcpy in the wait.
__global__ void k_scatter_xyz(uint32_t n, const uint32_t* __restrict__ perm, uint32_t off, uint32_t nn, const float4* __restrict__ src,
                              float* __restrict__ dst) {
    const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n) return;
    const uint32_t h = perm[s] - off;
    if (h >= nn) return;  // (another fluid's particle)
    const float4 v = src[s];
    dst[3 * (size_t)h] = v.x; dst[3 * (size_t)h + 1] = v.y; dst[3 * (size_t)h + 2] = v.z;
}
static bool host_pointer_is_pinned(const void* p) {
    hipPointerAttribute_t a{};
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }  // (plain malloc'ed memory is unknown to the runtime)
    return a.type == hipMemoryTypeHost;
}
void World::get_fluid_async(uint32_t slot, float* pos, float* vel_out) {
    use_device();
    const SlotSpan sp = fluid_span(slot);
    if (comm && dist_started) throw HipError(SALVA_HIP_E_INVALID, "host-order fluid arrays are not maintained in a multi-GPU run: use salva_hip_get_owned");
    wait_download();  // one download in flight
    const uint64_t nn = sp.n, off = sp.off;
    if (nn == 0 || (!pos && !vel_out)) return;
    if (!dl_stream) {
        SALVA_HIP_CHECK(hipStreamCreateWithFlags(&dl_stream, hipStreamNonBlocking));
        SALVA_HIP_CHECK(hipEventCreateWithFlags(&ev_dl_ready, hipEventDisableTiming));
        SALVA_HIP_CHECK(hipEventCreateWithFlags(&ev_dl_done, hipEventDisableTiming));
    }
    const size_t bytes = 3 * nn * sizeof(float);
    float* dsts[2] = {pos, vel_out};
    const float4* sorted_src[2] = {posm[cur].p, vel[cur].p};
    const float4* staged_src[2] = {st_pos.p + off, st_vel.p + off};
    const bool from_sorted = sorted_valid && !staging_current;
    for (int a = 0; a < 2; ++a) {
        if (!dsts[a]) continue;
        dl_dev[a].ensure(3 * nn, stream, false, 1.1f);
        if (from_sorted) k_scatter_xyz<<<nblk(n), BLOCK, 0, stream>>>(n, perm[cur].p, (uint32_t)off, (uint32_t)nn, sorted_src[a], dl_dev[a].p);
        else k_unpack_xyz<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, staged_src[a], dl_dev[a].p);
    }
    SALVA_HIP_CHECK(hipGetLastError());
    SALVA_HIP_CHECK(hipEventRecord(ev_dl_ready, stream));
    SALVA_HIP_CHECK(hipStreamWaitEvent(dl_stream, ev_dl_ready, 0));
    dl = PendingDownload{};
    dl.bytes = bytes;
    for (int a = 0; a < 2; ++a) {
        if (!dsts[a]) continue;
        dl.dst[a] = dsts[a];
        dl.staged[a] = !host_pointer_is_pinned(dsts[a]);
        float* target = dsts[a];
        if (dl.staged[a]) {
            if (h_dl_cap[a] < bytes) {
                if (h_dl[a]) SALVA_HIP_CHECK(hipHostFree(h_dl[a]));
                h_dl[a] = nullptr; h_dl_cap[a] = 0;
                const size_t cap = bytes + bytes / 8;
                SALVA_HIP_CHECK(hipHostMalloc((void**)&h_dl[a], cap, hipHostMallocDefault));
                h_dl_cap[a] = cap;
            }
            target = h_dl[a];
        }
        SALVA_HIP_CHECK(hipMemcpyAsync(target, dl_dev[a].p, bytes, hipMemcpyDeviceToHost, dl_stream));
    }
    SALVA_HIP_CHECK(hipEventRecord(ev_dl_done, dl_stream));
    dl.active = true;
}
void World::wait_download() {
    if (!dl.active) return;
    use_device();
    dl.active = false;
    SALVA_HIP_CHECK(hipEventSynchronize(ev_dl_done));
    for (int a = 0; a < 2; ++a)
        if (dl.dst[a] && dl.staged[a]) memcpy(dl.dst[a], h_dl[a], dl.bytes);
}

// A field is a component of one array: of a host-order array (brought up to date first), or of the step's scratch in sorted order
// (un-sorted through `perm`; valid only right after a step).
void World::get_fluid_field(uint32_t slot, int field, float* out) {
    use_device();
    const SlotSpan sp = fluid_span(slot);
    if (!out) throw HipError(SALVA_HIP_E_INVALID, "null output");
    if (comm && dist_started) throw HipError(SALVA_HIP_E_INVALID, "per-fluid host-order access is not available in a multi-GPU run: use salva_hip_get_owned");
    const uint64_t nn = sp.n, off = sp.off;
    if (nn == 0) return;
    enum Part { XYZ, W, F32, U32_AS_F32, SORTED_XYZ };  // (SORTED_XYZ: the xyz of a float4 array in sorted order)
    struct Source { const void* array; Part part; bool staged; };
    Source src{nullptr, F32, false};
    switch (field) {
        case SALVA_HIP_FIELD_VELOCITY_CHANGE: src = {st_dv.p, XYZ, true}; break;
        case SALVA_HIP_FIELD_PRESSURE: src = {st_dv.p, W, true}; break;
        case SALVA_HIP_FIELD_VOLUME: src = {st_pos.p, W, true}; break;
        case SALVA_HIP_FIELD_ACCELERATION: src = {st_acc.p, XYZ, true}; break;
        case SALVA_HIP_FIELD_DENSITY: src = {rho.p, F32, false}; break;
        case SALVA_HIP_FIELD_ALPHA: src = {alpha.p, F32, false}; break;
        case SALVA_HIP_FIELD_NUM_FLUID_CONTACTS: src = {nff.p, U32_AS_F32, false}; break;
        case SALVA_HIP_FIELD_NUM_BOUNDARY_CONTACTS: src = {nfb.p, U32_AS_F32, false}; break;
        case SALVA_HIP_FIELD_VORTICITY: {
            bool has = false;
            for (const SalvaHipForceDesc& d : fluids[slot].forces) has |= d.kind == SALVA_HIP_FORCE_VORTICITY_CONFINEMENT;
            if (!has) throw HipError(SALVA_HIP_E_INVALID, "SALVA_HIP_FIELD_VORTICITY: the fluid has no VorticityConfinement entry");
            src = {vort_omega.p, SORTED_XYZ, false};
            break;
        }
        default: break;
    }
    scratch_f.ensure(std::max<size_t>(3 * nn, n), stream, false, 1.1f);  // (one size for every field)
    if (src.staged) {
        if (field == SALVA_HIP_FIELD_ACCELERATION) {
            // not part of the working set; zero after every step (integrate_and_clear_accelerations) unless the host set them
            if (!acc_user) { memset(out, 0, 3 * nn * sizeof(float)); return; }
        } else {
            ensure_staging_current();
        }
        const float4* rows = static_cast<const float4*>(src.array) + off;
        if (src.part == XYZ) download_xyz(rows, nn, out);
        else download_w(rows, nn, out);
        return;
    }
    if (!sorted_valid || !have_last_ctx)
        throw HipError(SALVA_HIP_E_INVALID, "solver scratch fields are only available right after a step");
    if (field == SALVA_HIP_FIELD_NUM_BOUNDARY_CONTACTS && nb == 0) { memset(out, 0, nn * sizeof(float)); return; }
    if (field == SALVA_HIP_FIELD_VORTICITY && (!fluids[slot].vort_fresh || vort_omega.cap < n))  // (the entry was set after the last step's forces ran)
        throw HipError(SALVA_HIP_E_INVALID, "solver scratch fields are only available right after a step");
    if (!src.array) throw HipError(SALVA_HIP_E_INVALID, "unknown field");
    if (src.part == SORTED_XYZ) {
        scratch_f4.ensure(n);
        launch_unsort_f4(n, perm[cur].p, static_cast<const float4*>(src.array), scratch_f4.p, stream);
        download_xyz(scratch_f4.p + off, nn, out);
        return;
    }
    if (src.part == F32) launch_unsort_f32(n, perm[cur].p, static_cast<const float*>(src.array), scratch_f.p, stream);
    else launch_unsort_u32_as_f32(n, perm[cur].p, static_cast<const uint32_t*>(src.array), scratch_f.p, stream);
    download_f32(scratch_f.p + off, nn, out);
}

// checkpoint restore: the two pieces of solver state that live next to the fluid arrays (velocity_changes, IISPH pressures)
void World::set_fluid_field(uint32_t slot, int field, const float* data) {
    use_device();
    const SlotSpan sp = fluid_span(slot);
    if (!data) throw HipError(SALVA_HIP_E_INVALID, "null data");
    if (field != SALVA_HIP_FIELD_VELOCITY_CHANGE && field != SALVA_HIP_FIELD_PRESSURE)
        throw HipError(SALVA_HIP_E_INVALID, "only velocity_changes and pressures can be set");
    if (sp.n == 0) return;
    ensure_staging_current();
    if (field == SALVA_HIP_FIELD_VELOCITY_CHANGE) upload_xyz(data, st_dv.p + sp.off, sp.n, true);
    else upload_w(data, st_dv.p + sp.off, sp.n);
    order_invalidated(false);  // (the objects are what they were: the per-model tables stay)
}

void World::get_force_stats(uint32_t slot, uint32_t force, int32_t* iters, float* err) {
    if (slot >= fluids.size() || force >= fluids[slot].forces.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot / force index out of range");
    const FluidSlot& f = fluids[slot];
    if (iters) *iters = force < f.force_iters.size() ? (int32_t)f.force_iters[force] : 0;
    if (err) *err = force < f.force_errs.size() ? f.force_errs[force] : 0.0f;
}

// ------------------------------------------------------------------------------------------------ boundaries
void World::get_boundary(uint32_t slot, float* volumes, float* forces) {
    use_device();
    const SlotSpan sp = boundary_span(slot);
    if (sp.n == 0) return;
    if (volumes) {
        upload_tables();
        build_boundary_grid();
        scratch_f4.ensure(nb);
        scratch_f.ensure(nb, stream, false, 1.1f);  // (as before the helpers: World::device_bytes stays what it was)
        launch_unsort_f4(nb, bperm.p, bposv.p, scratch_f4.p, stream);
        download_w(scratch_f4.p + sp.off, sp.n, volumes);
    }
    if (forces) download_xyz(bforce.p + sp.off, sp.n, forces);
}

void World::get_boundary_particles(uint32_t slot, float* positions, float* velocities) {
    use_device();
    const SlotSpan sp = boundary_span(slot);
    if (sp.n == 0) return;
    if (positions) download_xyz(bst_pos.p + sp.off, sp.n, positions);
    if (velocities) download_xyz(bst_vel.p + sp.off, sp.n, velocities);
}

// ------------------------------------------------------------------------------------------------ contact exports
// The contact lists of the last step (they describe the positions the step started from, as the reference's
// ContactManager does after `step`) as CSR over `rows` particles: counts -> offsets -> the sizing return -> the device tables ->
// launch(offsets, fluid offsets, boundary offsets, j_model, j) -> the two arrays back.  d_counts: the rows' list lengths (null: all
// zero); with_moff: the launcher maps fluid indices to host order and wants every fluid's first row.  offsets: rows + 1 entries;
// entries are written only if `capacity` holds them all.
template <typename Launch>
uint64_t World::export_contacts(uint64_t rows, const uint32_t* d_counts, bool with_moff, uint64_t* offsets, uint32_t* j_model, uint32_t* j,
                                uint64_t capacity, Launch&& launch) {
    std::vector<uint32_t> cnt(rows, 0);
    if (d_counts && rows) {
        SALVA_HIP_CHECK(hipMemcpyAsync(cnt.data(), d_counts, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
    std::vector<uint64_t> offs(rows + 1, 0);
    for (uint64_t k = 0; k < rows; ++k) offs[k + 1] = offs[k] + cnt[k];
    const uint64_t total = offs[rows];
    if (offsets) memcpy(offsets, offs.data(), (rows + 1) * sizeof(uint64_t));
    if (!j_model || !j || capacity < total || total == 0) return total;
    std::vector<uint32_t> moff, boff(std::max<size_t>(bounds.size(), 1), 0);
    if (with_moff) {
        moff.assign(num_models(), 0);
        for (uint32_t s = 0; s < fluids.size(); ++s) moff[s] = (uint32_t)fluid_offset(s);
    }
    for (uint32_t s = 0; s < bounds.size(); ++s) boff[s] = (uint32_t)boundary_offset(s);
    DevBuf<uint64_t> d_offs;
    DevBuf<uint32_t> d_moff, d_boff, d_jm, d_j;
    d_offs.ensure(rows + 1); d_boff.ensure(boff.size()); d_jm.ensure(total); d_j.ensure(total);
    SALVA_HIP_CHECK(hipMemcpyAsync(d_offs.p, offs.data(), (rows + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    if (with_moff) {
        d_moff.ensure(moff.size());
        SALVA_HIP_CHECK(hipMemcpyAsync(d_moff.p, moff.data(), moff.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    }
    SALVA_HIP_CHECK(hipMemcpyAsync(d_boff.p, boff.data(), boff.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    flags_clean = false;
    launch(d_offs.p, d_moff.p, d_boff.p, d_jm.p, d_j.p);
    SALVA_HIP_CHECK(hipMemcpyAsync(j_model, d_jm.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipMemcpyAsync(j, d_j.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    return total;
}

// one fluid in host order: the counts are un-sorted first
uint64_t World::get_fluid_contacts(uint32_t slot, int boundary, uint64_t* offsets, uint32_t* j_model, uint32_t* j, uint64_t capacity) {
    use_device();
    const SlotSpan sp = fluid_span(slot);
    if (comm) throw HipError(SALVA_HIP_E_INVALID, "host-order contact export does not exist in a multi-GPU run: use salva_hip_get_local_contacts");
    if (!have_last_ctx || !sorted_valid) throw HipError(SALVA_HIP_E_INVALID, "no completed step: there are no contact lists yet");
    DevBuf<uint32_t> d_cnt;
    const bool any = !(boundary && nb == 0) && sp.n;
    if (any) {
        d_cnt.ensure(n);
        launch_unsort_u32(n, perm[cur].p, boundary ? nfb.p : nff.p, d_cnt.p, stream);
    }
    return export_contacts(sp.n, any ? d_cnt.p + sp.off : nullptr, true, offsets, j_model, j, capacity,
                           [&](const uint64_t* offs, const uint32_t* moff, const uint32_t* boff, uint32_t* jm, uint32_t* jj) {
                               launch_export_contacts(last_ctx, G().keys[1].p, slot, boundary, offs, moff, boff, jm, jj, stream);
                           });
}

// ---- the working set as it is (include/salva_hip.h "local view"): sorted order, global ids; per rank in a decomposed run
__global__ void k_local_ghost_flags(uint32_t n, const uint32_t* __restrict__ gtag, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (gtag && (gtag[i] & 0x80000000u)) ? 1 : 0;
}
void World::get_local(uint32_t* ids, uint32_t* fluid_slots, uint8_t* is_ghost, float* positions, float* velocities, float* densities, float* volumes) {
    use_device();
    if (!sorted_valid || (!have_last_ctx && !in_force_cb)) throw HipError(SALVA_HIP_E_INVALID, "no completed step: the working set has no order yet");
    if (n == 0) return;
    if (ids) SALVA_HIP_CHECK(hipMemcpyAsync(ids, perm[cur].p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (fluid_slots) SALVA_HIP_CHECK(hipMemcpyAsync(fluid_slots, model[cur].p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (is_ghost) {
        DevBuf<uint8_t> flags;
        flags.ensure(n);
        k_local_ghost_flags<<<nblk(n), BLOCK, 0, stream>>>(n, comm ? gtag[cur].p : nullptr, flags.p);
        SALVA_HIP_CHECK(hipMemcpyAsync(is_ghost, flags.p, (size_t)n, hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
    scratch_f.ensure(3 * (size_t)n, stream, false, 1.1f);  // (one size for all of them)
    if (positions) download_xyz(posm[cur].p, n, positions);
    // inside a force callback fluid.velocities equal w = v + dv (dfsph_solver.rs:688-693), as in force_get_state
    if (velocities) download_xyz(in_force_cb ? last_ctx.w : vel[cur].p, n, velocities);
    if (densities) SALVA_HIP_CHECK(hipMemcpyAsync(densities, rho.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (volumes) download_w(vel[cur].p, n, volumes);  // (they ride in vel.w, device_types.h)
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
}
// every local particle, in sorted order: the counts as they are, fluid indices stay local
uint64_t World::get_local_contacts(int boundary, uint64_t* offsets, uint32_t* j_model, uint32_t* j, uint64_t capacity) {
    use_device();
    if (!have_last_ctx || !sorted_valid) throw HipError(SALVA_HIP_E_INVALID, "no completed step: there are no contact lists yet");
    const uint32_t* d_counts = (boundary && nb == 0) ? nullptr : (boundary ? nfb.p : nff.p);
    return export_contacts(n, d_counts, false, offsets, j_model, j, capacity,
                           [&](const uint64_t* offs, const uint32_t*, const uint32_t* boff, uint32_t* jm, uint32_t* jj) {
                               launch_export_contacts_local(last_ctx, G().keys[1].p, boundary, offs, boff, jm, jj, stream);
                           });
}

// ------------------------------------------------------------------------------------------------ host force callbacks
__global__ void k_add_acc_local(uint32_t n, const float* __restrict__ in, float4* __restrict__ acc) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    float4 a = acc[s];
    a.x += in[3 * (size_t)s]; a.y += in[3 * (size_t)s + 1]; a.z += in[3 * (size_t)s + 2];
    acc[s] = a;
}
__global__ void k_add_acc_from_host(uint32_t n, const uint32_t* __restrict__ perm, uint32_t off, uint32_t nn,
                                    const float* __restrict__ in, float4* __restrict__ acc) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t g = perm[s] - off;  // host index within the fluid (wraps for other fluids)
    if (g >= nn) return;
    float4 a = acc[s];
    a.x += in[3 * g]; a.y += in[3 * g + 1]; a.z += in[3 * g + 2];
    acc[s] = a;
}

void World::force_get_state(uint32_t slot, float* positions, float* velocities, float* densities) {
    use_device();
    if (!in_force_cb) throw HipError(SALVA_HIP_E_INVALID, "only available inside a force callback");
    const SlotSpan sp = fluid_span(slot);
    const uint64_t nn = sp.n, off = sp.off;
    if (nn == 0) return;
    scratch_f4.ensure(n);
    scratch_f.ensure(std::max<size_t>(3 * nn, n), stream, false, 1.1f);  // (the un-sorted densities need n)
    for (int k = 0; k < 2; ++k) {
        float* out = k == 0 ? positions : velocities;
        if (!out) continue;
        // fluid.velocities equal w = v + dv while the forces run (dfsph_solver.rs:688-693)
        launch_unsort_f4(n, perm[cur].p, k == 0 ? last_ctx.posm : last_ctx.w, scratch_f4.p, stream);
        download_xyz(scratch_f4.p + off, nn, out);
    }
    if (densities) {
        launch_unsort_f32(n, perm[cur].p, last_ctx.rho, scratch_f.p, stream);
        download_f32(scratch_f.p + off, nn, densities);
    }
}

void World::force_add_accelerations(uint32_t slot, const float* acc_h) {
    use_device();
    if (!in_force_cb) throw HipError(SALVA_HIP_E_INVALID, "only available inside a force callback");
    const SlotSpan sp = fluid_span(slot);
    if (!acc_h) throw HipError(SALVA_HIP_E_INVALID, "null accelerations");
    if (sp.n == 0) return;
    k_add_acc_from_host<<<nblk(n), BLOCK, 0, stream>>>(n, perm[cur].p, (uint32_t)sp.off, (uint32_t)sp.n, stage_floats(acc_h, 3 * sp.n), last_ctx.acc);
    SALVA_HIP_CHECK(hipGetLastError());
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
}
void World::force_add_local_accelerations(const float* acc_h) {
    use_device();
    if (!in_force_cb) throw HipError(SALVA_HIP_E_INVALID, "only available inside a force callback");
    if (!acc_h) throw HipError(SALVA_HIP_E_INVALID, "null accelerations");
    if (n == 0) return;
    // (what lands on a ghost is overwritten by the refresh of w that follows the forces, world_dist)
    k_add_acc_local<<<nblk(n), BLOCK, 0, stream>>>(n, stage_floats(acc_h, 3 * (size_t)n), last_ctx.acc);
    SALVA_HIP_CHECK(hipGetLastError());
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
}

// ------------------------------------------------------------------------------------------------ Becker2009Elasticity (elastic.hip)
// The state is read and written at its own particle count n0: the fluid's count, except between a change of that count and the
// next step, when the state still has the old length (the next step re-initialises it from there: quirk 1 needs the old volumes0).
uint64_t World::get_elasticity_state(uint32_t slot, uint32_t force, uint64_t nn, float* positions0, float* volumes0, float* rotations,
                                     float* stress, float* grad_tr) {
    use_device();
    ElasticState& e = elastic_state(slot, force);
    if (e.n0 == 0) return 0;
    if (nn == 0) return e.nnz;  // (sizing call)
    if (nn != e.n0) throw HipError(SALVA_HIP_E_INVALID, "n is not the elastic state's particle count (salva_hip_get_elasticity_contacts)");
    if (positions0) download_xyz(e.p0.p, nn, positions0);
    auto down = [&](float* dst, const float* src, size_t cnt) {
        if (dst) SALVA_HIP_CHECK(hipMemcpyAsync(dst, src, cnt * sizeof(float), hipMemcpyDeviceToHost, stream));
    };
    down(volumes0, e.vol0.p, nn);
    down(rotations, e.rot.p, 9 * nn);
    down(stress, e.sig.p, 6 * nn);
    down(grad_tr, e.F.p, 9 * nn);
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    return e.nnz;
}

uint64_t World::get_elasticity_contacts(uint32_t slot, uint32_t force, uint64_t* n0, uint32_t* offsets, uint32_t* j, uint64_t capacity) {
    use_device();
    ElasticState& e = elastic_state(slot, force);
    if (n0) *n0 = e.n0;
    if (e.n0 == 0 || capacity < e.nnz) return e.n0 ? e.nnz : 0;
    if (offsets) SALVA_HIP_CHECK(hipMemcpyAsync(offsets, e.off.p, (e.n0 + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (j) SALVA_HIP_CHECK(hipMemcpyAsync(j, e.nbr.p, e.nnz * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    return e.nnz;
}

void World::set_elasticity_state(uint32_t slot, uint32_t force, uint64_t nn, const float* positions0, const float* volumes0,
                                 const float* rotations) {
    use_device();
    ElasticState& e = elastic_state(slot, force);
    if (nn == 0) throw HipError(SALVA_HIP_E_INVALID, "an elastic state needs at least one particle");
    const bool fresh = e.n0 != nn;
    if (fresh && !positions0) throw HipError(SALVA_HIP_E_INVALID, "positions0 is required when the state is new or changes length");
    e.p0.ensure(nn, stream, !fresh, 1.1f); e.hp.ensure(nn, stream, false, 1.1f);
    e.vol0.ensure(nn, stream, !fresh, 1.1f); e.rot.ensure(9 * nn, stream, !fresh, 1.1f);
    e.rot_new.ensure(9 * nn, stream, false, 1.1f); e.sig.ensure(6 * nn, stream, false, 1.1f); e.F.ensure(9 * nn, stream, false, 1.1f);
    if (fresh) {
        SALVA_HIP_CHECK(hipMemsetAsync(e.vol0.p, 0, nn * sizeof(float), stream));
        SALVA_HIP_CHECK(hipMemsetAsync(e.sig.p, 0, 6 * nn * sizeof(float), stream));
        SALVA_HIP_CHECK(hipMemsetAsync(e.F.p, 0, 9 * nn * sizeof(float), stream));
        launch_elastic_identity(e, 0, nn, stream);
    }
    if (positions0) upload_xyz(positions0, e.p0.p, nn, false);
    if (volumes0) SALVA_HIP_CHECK(hipMemcpyAsync(e.vol0.p, volumes0, nn * sizeof(float), hipMemcpyHostToDevice, stream));
    if (rotations) SALVA_HIP_CHECK(hipMemcpyAsync(e.rot.p, rotations, 9 * nn * sizeof(float), hipMemcpyHostToDevice, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    e.n0 = nn;
    e.ran = false;
    // the rest lists from positions0 now (the same lists the state had: rows are sorted); volumes0 stays as given
    elastic_build_rest(e, make_sph_consts(prm.particle_radius * prm.smoothing_factor * 2.0f), elastic_params(fluids[slot].forces[force].p),
                       true, stream);
}

}  // namespace salva

// userforce.hip — user-defined NonPressureForces as kernels (SALVA_HIP_FORCE_DEVICE, include/salva_hip.h).
//
// The reference's one extension point is `impl NonPressureForce` (solver/nonpressure_force.rs:10-30; examples3d/custom_forces3.rs:67-90).
// The host arm (SALVA_HIP_FORCE_CUSTOM) moves the substep's state over PCIe twice and waits; this arm tells the user where that state
// lies and on which stream the substep runs, and the user's callback enqueues a kernel there.  What the solver's own kernels read —
// ELL lists of 16-bit halo slots per tile — is no interface, so a force that needs contacts gets them as CSR tables over the sorted
// particle order: offsets (exclusive scan of nff / nfb), the neighbour's sorted index, and optionally W and grad W per contact.
//
// k_contact_tables.  A wave takes 64 consecutive rows.  Each lane walks to ITS row once (tile.h contact_row: keys -> slot -> slice ->
// list), the 64 descriptors go to LDS, and the wave then runs over the rows' entries as ONE flat range — the rows of consecutive
// particles are consecutive in a CSR table — with lane l writing entry base + l, base + 64 + l, ...: every store of the wave is one
// contiguous run of 256 bytes (indices) or 1 KiB (kernel values), whatever the rows' lengths, and every lane has work until the last
// trip.  (One thread per row writes at a stride of a row's length: 64 cache lines per store.)  An entry finds its row by a binary
// search over the 64 offsets in LDS; its list dword is read through the row's pointer — the rows of a slice are 16 bytes apart, so
// the wave's reads share their lines in L1 — and the neighbour's record is gathered as every neighbour pass gathers it.
// The file is compiled with -ffp-contract=off like the rest: r^2 is (dx dx + dy dy) + dz dz for (i, j) and (j, i) alike, so
// grad W_ij = -grad W_ji bit for bit.
#include <algorithm>
#include <cstring>

#include "kernels.h"
#include "tile.h"
#include "world.h"

namespace salva {

__global__ __launch_bounds__(BLOCK) void k_widen_counts(uint32_t n, const uint32_t* __restrict__ cnt, uint64_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i <= n) out[i] = i < n ? cnt[i] : 0u;  // (n + 1 entries: the scan's last one is the total)
}

// Contact::weight / Contact::gradient of one pair (geometry/contacts.rs:40-55) for the world's kernel pair: sph_math.h kernel_eval,
// with the reference's other kernels where the world was created with them (this file is compiled once, so the choice is a
// wave-uniform branch here and not a second compilation: a table build is no hot loop)
__device__ __forceinline__ float4 contact_kernel(const float4& pi, const float4& pj, const SphConsts& sc) {
    const float dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
    const float r2 = dist2_exact(dx, dy, dz);
    KernelEval e = kernel_eval(r2, sc);
    if (sc.kd) e.w = other_kernel_w(sc.kd, __builtin_amdgcn_sqrtf(r2), sc);
    if (sc.kg) e.g = other_kernel_g(sc.kg, r2, sc);
    return make_float4(e.g * dx, e.g * dy, e.g * dz, e.w);
}

template <bool KERN>
__global__ __launch_bounds__(BLOCK) void k_contact_tables(StepCtx c, const uint32_t* __restrict__ keys, int boundary,
                                                          const uint64_t* __restrict__ off, uint64_t capacity,
                                                          uint32_t* __restrict__ out_j, float4* __restrict__ out_kern) {
    constexpr uint32_t NW = BLOCK / WAVE;
    __shared__ uint32_t s_rel[NW][WAVE + 1];        // a row's first entry, relative to the wave's first; [WAVE] = the wave's entries
    __shared__ const uint32_t* s_p[NW][WAVE];       // ContactRow::p
    __shared__ uint64_t s_hoff[NW][WAVE];           // ContactRow::hoff
    const uint32_t wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const uint32_t i0 = blockIdx.x * BLOCK + wid * WAVE;  // the wave's first row
    const uint32_t i = i0 + lane;
    const uint64_t base = off[min(i0, c.n)];
    {
        ContactRow row{nullptr, 0ull, 0u};
        uint64_t o = base;
        if (i < c.n) { row = contact_row(c, keys, i, boundary); o = off[i]; }
        else if (i0 < c.n) o = off[c.n];
        s_rel[wid][lane] = (uint32_t)(o - base);
        if (lane == WAVE - 1) s_rel[wid][WAVE] = (uint32_t)(o - base) + row.cnt;
        s_p[wid][lane] = row.p;
        s_hoff[wid][lane] = row.hoff;
    }
    __syncthreads();  // (every thread arrives: nobody has returned)
    const uint32_t total = s_rel[wid][WAVE];
    for (uint32_t e = lane; e < total; e += WAVE) {
        // the row that holds entry e: the last one that starts at or before it (an empty row starts where its successor does)
        uint32_t lo = 0u, hi = WAVE;
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_rel[wid][mid] <= e) lo = mid; else hi = mid;
        }
        const uint64_t o = base + e;
        if (o >= capacity) continue;  // (the buffers are cut for the list totals the host has read: never taken)
        const uint32_t s = contact_row_entry(s_p[wid][lo], e - s_rel[wid][lo]);
        const uint32_t g = boundary ? c.bhalo_src[s_hoff[wid][lo] + s] : c.halo_src[s_hoff[wid][lo] + s];
        out_j[o] = g;
        if (KERN) out_kern[o] = contact_kernel(c.posm[i0 + lo], boundary ? c.bposv[g] : c.posm[g], c.sc);
    }
}

void launch_contact_offsets(uint32_t n, const uint32_t* counts, uint64_t* off, void* temp, size_t temp_bytes, hipStream_t s) {
    k_widen_counts<<<div_up((size_t)n + 1, BLOCK), BLOCK, 0, s>>>(n, counts, off);
    scan_u64(temp, temp_bytes, off, off, n + 1, s);  // (in place)
}
void launch_contact_tables(const StepCtx& c, const uint32_t* keys, int boundary, const uint64_t* off, uint64_t capacity, uint32_t* out_j,
                           float4* out_kern, hipStream_t s) {
    if (!c.n) return;
    if (out_kern) k_contact_tables<true><<<div_up(c.n, BLOCK), BLOCK, 0, s>>>(c, keys, boundary, off, capacity, out_j, out_kern);
    else k_contact_tables<false><<<div_up(c.n, BLOCK), BLOCK, 0, s>>>(c, keys, boundary, off, capacity, out_j, nullptr);
}

// The tables of this pass's lists, for the union of what the pass's device forces ask for: built once, by the first force that asks.
void World::build_contact_tables(const StepCtx& c, uint32_t needs) {
    // (a world with a device force neither speculates nor defers its list check: build_lists has read the totals back)
    if (pass.spec || pass.defer_lists) throw HipError(SALVA_HIP_E_HIP, "internal error: contact tables in a pass whose list totals are not known");
    const bool kern = (needs & SALVA_HIP_DEVICE_NEEDS_KERNEL) != 0;
    const size_t tb = scan_temp_bytes(n + 1);
    ensure_cub_temp(tb);
    auto grow = [&](auto& buf, size_t count) {
        const bool had = buf.p != nullptr;
        try {
            if (buf.ensure(count, stream, false, 1.1f) && had) ++dforce_stats[3];  // (releasing the old buffer made the host wait for the device)
        } catch (const HipError& e) {
            (void)hipGetLastError();
            throw HipError(SALVA_HIP_E_CAPACITY, std::string("the contact tables of a device force do not fit: ") + e.what());
        }
    };
    for (int b = 0; b < 2; ++b) {
        if (!(needs & (b ? SALVA_HIP_DEVICE_NEEDS_FB : SALVA_HIP_DEVICE_NEEDS_FF))) continue;
        const uint64_t total = (b && nb == 0) ? 0ull : (b ? h_rb->ncontacts_fb : h_rb->ncontacts_ff);
        grow(dtab.off[b], (size_t)n + 1);
        grow(dtab.j[b], std::max<uint64_t>(total, 1));
        if (kern) grow(dtab.kern[b], std::max<uint64_t>(total, 1));
        if (b && nb == 0) {  // (no boundary particle: the counts were never written)
            SALVA_HIP_CHECK(hipMemsetAsync(dtab.off[b].p, 0, ((size_t)n + 1) * sizeof(uint64_t), stream));
        } else {
            launch_contact_offsets(n, b ? nfb.p : nff.p, dtab.off[b].p, cub_temp.p, tb, stream);
            launch_contact_tables(c, G().keys[1].p, b, dtab.off[b].p, total, dtab.j[b].p, kern ? dtab.kern[b].p : nullptr, stream);
        }
        SALVA_HIP_CHECK(hipGetLastError());
        dforce_stats[2] += ((uint64_t)n + 1) * sizeof(uint64_t) + total * (sizeof(uint32_t) + (kern ? sizeof(float4) : 0));
    }
    pass.dforce_tables = needs;
    ++dforce_stats[1];
}

// A user's `NonPressureForce::solve` as a kernel, at its place in the list: no wait, nothing over PCIe.
void World::run_device_force(const StepCtx& c, uint32_t slot, uint32_t force) {
    const SalvaHipForceDesc& d = fluids[slot].forces[force];
    if (!dforce_cb) throw HipError(SALVA_HIP_E_INVALID, "a SALVA_HIP_FORCE_DEVICE entry needs salva_hip_set_device_force_callback");
    if (comm || c.gate) throw HipError(SALVA_HIP_E_HIP, "internal error: a device force in a decomposed or chained pass");
    const uint32_t needs = (uint32_t)d.p[0];
    if ((needs & (SALVA_HIP_DEVICE_NEEDS_FF | SALVA_HIP_DEVICE_NEEDS_FB)) && !pass.dforce_tables) {
        uint32_t all = 0;  // what the device forces of this pass ask for between them: the lists do not change between forces
        for (const FluidSlot& f : fluids)
            if (f.n)
                for (const SalvaHipForceDesc& e : f.forces)
                    if (e.kind == SALVA_HIP_FORCE_DEVICE && ((uint32_t)e.p[0] & 3u)) all |= (uint32_t)e.p[0];
        build_contact_tables(c, all);
    }
    SalvaHipDeviceView v;
    memset(&v, 0, sizeof(v));
    v.struct_size = (uint32_t)sizeof(v); v.version = SALVA_HIP_DEVICE_VIEW_VERSION;
    v.stream = (void*)stream;
    v.fluid_slot = slot; v.force_index = force;
    v.dt = dt_prev; v.inv_dt = inv_dt_prev;
    v.h = sc.h; v.particle_radius = prm.particle_radius;
    v.kernel_density = prm.kernel_density; v.kernel_gradient = prm.kernel_gradient;
    memcpy(v.params, d.p, sizeof(v.params));
    v.needs = needs;
    v.n = c.n; v.nfluids = (uint32_t)fluids.size();
    v.posm = reinterpret_cast<const float*>(c.posm); v.vel = reinterpret_cast<const float*>(c.w); v.acc = reinterpret_cast<float*>(c.acc);
    v.rho = c.rho; v.model = c.model; v.id = c.perm; v.rho0 = c.rho0_tab;
    v.nb = c.nb; v.bforce_scale = c.bforce_scale;
    v.bposv = reinterpret_cast<const float*>(c.bposv); v.bvel = reinterpret_cast<const float*>(c.bvel); v.bid = c.bperm;
    v.bforce_fx = reinterpret_cast<uint64_t*>(c.bforce_fx); v.bwants = c.bwants;
    const bool kern = (needs & SALVA_HIP_DEVICE_NEEDS_KERNEL) != 0;
    if (needs & SALVA_HIP_DEVICE_NEEDS_FF) {
        v.ff_off = dtab.off[0].p; v.ff_j = dtab.j[0].p;
        if (kern) v.ff_kern = reinterpret_cast<const float*>(dtab.kern[0].p);
    }
    if (needs & SALVA_HIP_DEVICE_NEEDS_FB) {
        v.fb_off = dtab.off[1].p; v.fb_j = dtab.j[1].p;
        if (kern) v.fb_kern = reinterpret_cast<const float*>(dtab.kern[1].p);
    }
    // (inside the callback the local getters read what the host arm's callback reads: this pass's context)
    last_ctx = c; last_ctx.ctl = nullptr; have_last_ctx = true;
    in_force_cb = true; in_dforce_cb = true;
    int rc = 0;
    try {
        rc = dforce_cb(dforce_user, dforce_owner, &v);
    } catch (...) {
        in_force_cb = false; in_dforce_cb = false; have_last_ctx = false;
        throw;
    }
    in_force_cb = false; in_dforce_cb = false; have_last_ctx = false;
    ++dforce_stats[0];
    if (rc != 0) throw HipError(SALVA_HIP_E_INVALID, "the device force callback reported an error");
    SALVA_HIP_CHECK(hipGetLastError());  // (a launch of the user's that failed to enqueue)
}

void World::device_view_read(const void* device_src, void* host_dst, uint64_t bytes) {
    use_device();
    if (!in_dforce_cb) throw HipError(SALVA_HIP_E_INVALID, "only available inside a device force callback");
    if (bytes && (!device_src || !host_dst)) throw HipError(SALVA_HIP_E_INVALID, "null argument");
    if (!bytes) return;
    SALVA_HIP_CHECK(hipMemcpyAsync(host_dst, device_src, bytes, hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
}

}  // namespace salva

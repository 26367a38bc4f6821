// world.hip — host side of libsalva_hip: device memory, object edits, the per-model tables, up/download, timing probes.
// The per-step launch sequence (World::step, World::substep and what they call) is world_step.hip, rigid-body coupling and
// DynamicContactSampling are world_coupling.hip, the particle queries world_query.hip.
// Host <-> device traffic happens only in set_* / get_*.
#include "world.h"
#include "bbox.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include <mutex>
#include <unordered_map>

namespace salva {

void raise_tile_lds_limit(const void* kernel, uint32_t bytes) {
    if (bytes > 160u * 1024u)
        throw HipError(SALVA_HIP_E_CAPACITY, "a tile's halo does not fit the 160 KiB LDS (particles are compressed far beyond rest density)");
    static std::mutex mu;
    static std::unordered_map<const void*, uint32_t> granted;
    std::lock_guard<std::mutex> lock(mu);
    uint32_t& g = granted[kernel];
    if (bytes <= g) return;
    const uint32_t want = std::min<uint32_t>(160u * 1024u, std::max<uint32_t>(bytes + bytes / 4, 64u * 1024u));
    SALVA_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want));
    g = want;
}

// ------------------------------------------------------------------------------------------------ small helpers
__global__ void k_pack_xyz(uint32_t n, const float* __restrict__ src, float4* __restrict__ dst, int keep_w, float wval) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    float4 d = dst[i];
    d.x = src[3 * i]; d.y = src[3 * i + 1]; d.z = src[3 * i + 2];
    if (!keep_w) d.w = wval;
    dst[i] = d;
}
__global__ void k_pack_w(uint32_t n, const float* __restrict__ src, float4* __restrict__ dst) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) reinterpret_cast<float*>(&dst[i])[3] = src[i];
}
__global__ void k_fill_f4(uint32_t n, float4* __restrict__ dst, float4 v, int keep_w) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (keep_w) v.w = dst[i].w;
    dst[i] = v;
}
__global__ void k_fill_w(uint32_t n, float4* __restrict__ dst, float v) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) reinterpret_cast<float*>(&dst[i])[3] = v;
}
__global__ void k_fill_u32(uint32_t n, uint32_t* __restrict__ dst, uint32_t v) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) dst[i] = v;
}
__global__ void k_unpack_xyz(uint32_t n, const float4* __restrict__ src, float* __restrict__ dst) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 s = src[i];
    dst[3 * i] = s.x; dst[3 * i + 1] = s.y; dst[3 * i + 2] = s.z;
}
void launch_unpack_xyz(uint32_t n, const float4* src, float* dst, hipStream_t s) { k_unpack_xyz<<<nblk(n), BLOCK, 0, s>>>(n, src, dst); }
__global__ void k_unpack_w(uint32_t n, const float4* __restrict__ src, float* __restrict__ dst) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) dst[i] = src[i].w;
}
__global__ void k_set_bmodel(uint32_t n, float4* __restrict__ bvel, uint32_t m) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) reinterpret_cast<float*>(&bvel[i])[3] = __uint_as_float(m);
}

struct Piece { uint64_t src_off, len; bool from_old; };

template <typename T>
static void rebuild(DevBuf<T>& buf, const std::vector<Piece>& pieces, uint64_t new_total, hipStream_t s) {
    DevBuf<T> nb;
    nb.ensure(new_total ? new_total : 1);
    uint64_t off = 0;
    for (const Piece& p : pieces) {
        if (p.from_old && p.len)
            SALVA_HIP_CHECK(hipMemcpyAsync(nb.p + off, buf.p + p.src_off, p.len * sizeof(T), hipMemcpyDeviceToDevice, s));
        off += p.len;
    }
    SALVA_HIP_CHECK(hipStreamSynchronize(s));
    std::swap(buf.p, nb.p);
    std::swap(buf.cap, nb.cap);
}

int bits_for(uint64_t ncells) {
    int b = 1;
    while (b < 32 && ((uint64_t)1 << b) < ncells) ++b;
    return b;
}

// the model id of every staged particle: a slot's particles move when a slot before it changes its length
void World::stamp_fluid_models() {
    uint64_t o = 0;
    for (uint32_t s = 0; s < fluids.size(); ++s) {
        if (fluids[s].n) k_fill_u32<<<nblk(fluids[s].n), BLOCK, 0, stream>>>((uint32_t)fluids[s].n, st_model.p + o, s);
        o += fluids[s].n;
    }
}
void World::stamp_boundary_models() {  // (boundary model ids ride in bst_vel.w)
    uint64_t o = 0;
    for (uint32_t s = 0; s < bounds.size(); ++s) {
        if (bounds[s].n) k_set_bmodel<<<nblk(bounds[s].n), BLOCK, 0, stream>>>((uint32_t)bounds[s].n, bst_vel.p + o, s);
        o += bounds[s].n;
    }
}

// ------------------------------------------------------------------------------------------------ switches
// The one place where a world looks at the environment (switches.h): a host that calls setenv while a world steps changes nothing.
Switches Switches::from_env() {
    Switches s;
    auto on = [](const char* name) { return getenv(name) != nullptr; };
    s.spec_dist_off = on("SALVA_HIP_NO_SPEC_DIST");
    s.overlap_exchange = !on("SALVA_HIP_NO_OVERLAP");
    s.spec_off = !on("SALVA_HIP_SPECULATE") || on("SALVA_HIP_NO_SPECULATION");
    s.spec_tight = on("SALVA_HIP_SPEC_TIGHT");
    s.defer_off = on("SALVA_HIP_NO_DEFER_LISTS");
    s.spec_apply_off = on("SALVA_HIP_NO_SPEC_APPLY");
    s.chain_off = on("SALVA_HIP_NO_CHAIN");
    s.pre_off = on("SALVA_HIP_NO_PREGRID");
    s.no_publish = on("SALVA_HIP_NO_PUBLISH");
    s.split_off = on("SALVA_HIP_NO_SPLIT");
    s.classes_off = on("SALVA_HIP_NO_CLASSES");
    s.classes_forced = on("SALVA_HIP_CLASSES");
    s.light_on = on("SALVA_HIP_LIGHT");
    s.ref_off = on("SALVA_HIP_FULL_HALO");
    s.ref_forced = on("SALVA_HIP_REF_HALO");
    s.ref_tight = on("SALVA_HIP_REF_TIGHT");
    s.compact_halo = on("SALVA_HIP_COMPACT_HALO");
    if (const char* e = getenv("SALVA_HIP_SPLIT_S")) s.split_forced = (uint32_t)std::max(atoi(e), 1);
    s.no_planes = on("SALVA_HIP_NO_PLANES");
    s.two_mass_off = on("SALVA_HIP_NO_TWO_MASS");
    if (const char* e = getenv("SALVA_HIP_MAX_MASSES")) s.max_masses = (uint32_t)std::min(std::max(atoi(e), 2), 4);  // (2 = round 5's rule, the default)
    s.fold_off = on("SALVA_HIP_NO_FOLD");
    if (const char* e = getenv("SALVA_HIP_FOLD_CELLS")) {
        const long v = atol(e);
        if (v >= 8 && v <= (1 << 20) && (v & (v - 1)) == 0) s.fold_forced = (uint32_t)v;
    }
    s.tile_trace = on("SALVA_HIP_TILE_TRACE");
    s.dist_trace = on("SALVA_HIP_DIST_TRACE");
    s.no_fused_div = on("SALVA_HIP_NO_FUSED_DIV");
    s.dcs_batch_off = on("SALVA_HIP_NO_DCS_BATCH");
    if (const char* e = getenv("SALVA_HIP_DCSB_CAP0")) s.dcsb_cap0 = (uint32_t)std::max(atoi(e), 1);
    if (const char* e = getenv("SALVA_HIP_RADIX_SORT")) s.sort_mode = atoi(e) != 0 ? 1 : 0;
    if (const char* e = getenv("SALVA_HIP_DS_LEVEL")) s.ds_level = (uint32_t)std::max(0, atoi(e));
    if (const char* e = getenv("SALVA_HIP_LIST_CAP0")) { s.list_cap0 = std::max<uint32_t>(LIST_REGS, ((uint32_t)atoi(e) + 3u) & ~3u); s.trust_cap0 = true; }
#ifdef SALVA_HIP_DIAG
    if (const char* e = getenv("SALVA_HIP_SCHED")) s.sched_mode = atoi(e);
    if (const char* e = getenv("SALVA_HIP_TILE_THREADS")) { s.tile_threads = (uint32_t)atoi(e); s.tile_threads_set = true; }
    s.no_pipeline = on("SALVA_HIP_NO_PIPELINE");
    if (const char* e = getenv("SALVA_HIP_PIPE_WAVES")) s.pipe_waves = std::min<uint32_t>(std::max(atoi(e), 1), PIPE_MAX_WAVES);
    s.tile_timing = on("SALVA_HIP_TILE_TIMING");
#endif
    return s;
}

// ------------------------------------------------------------------------------------------------ ctor / dtor
World::World(const SalvaHipParams& p) : prm(p) {
    if (!(p.particle_radius > 0.0f) || !(p.smoothing_factor > 0.0f))
        throw HipError(SALVA_HIP_E_INVALID, "particle_radius and smoothing_factor must be positive");
    if (p.solver != SALVA_HIP_SOLVER_DFSPH && p.solver != SALVA_HIP_SOLVER_IISPH)
        throw HipError(SALVA_HIP_E_INVALID, "unknown solver kind");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        throw HipError(SALVA_HIP_E_HIP, "no HIP device available: libsalva_hip has no CPU fallback");
    if (p.device < 0 || p.device >= ndev) throw HipError(SALVA_HIP_E_INVALID, "device ordinal out of range");
    use_device();
    // h = particle_radius * smoothing_factor * 2 (liquid_world.rs:44)
    const float h = p.particle_radius * p.smoothing_factor * 2.0f;
    sc = make_sph_consts(h);
    if (p.kernel_density < 0 || p.kernel_density > SALVA_HIP_KERNEL_VISCOSITY || p.kernel_gradient < 0 || p.kernel_gradient > SALVA_HIP_KERNEL_VISCOSITY)
        throw HipError(SALVA_HIP_E_INVALID, "unknown kernel kind");
    sc.kd = p.kernel_density;
    sc.kg = p.kernel_gradient;
    SALVA_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    SALVA_HIP_CHECK(hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking));
    SALVA_HIP_CHECK(hipEventCreateWithFlags(&ev_pre_refresh, hipEventDisableTiming));
    SALVA_HIP_CHECK(hipEventCreateWithFlags(&ev_interior, hipEventDisableTiming));
    SALVA_HIP_CHECK(hipEventCreateWithFlags(&ev_spec_eval, hipEventDisableTiming));
    SALVA_HIP_CHECK(hipEventCreateWithFlags(&ev_spec_apply, hipEventDisableTiming));
    lds.ds_level = sw.ds_level;
    if (sw.trust_cap0) cap_ff = sw.list_cap0;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, p.device) == hipSuccess && cus > 0) num_cus = cus;
    }
    SALVA_HIP_CHECK(hipHostMalloc((void**)&h_rb, sizeof(Readback), hipHostMallocDefault));
    memset(h_rb, 0, sizeof(Readback));
    SALVA_HIP_CHECK(hipHostMalloc((void**)&h_ctl, 2 * NUM_SOLVES * sizeof(SolveCtl), hipHostMallocDefault));
    memset(h_ctl, 0, 2 * NUM_SOLVES * sizeof(SolveCtl));
    SALVA_HIP_CHECK(hipHostMalloc((void**)&h_pub, NUM_SOLVES * sizeof(SolveCtl), hipHostMallocMapped | hipHostMallocCoherent));
    memset(h_pub, 0, NUM_SOLVES * sizeof(SolveCtl));
    SALVA_HIP_CHECK(hipHostMalloc((void**)&h_hostpub, sizeof(HostPub), hipHostMallocMapped | hipHostMallocCoherent));
    memset(h_hostpub, 0, sizeof(HostPub));
    d_ctl.ensure(NUM_SOLVES);
    d_rb.ensure(1);
    d_flags.p = &d_rb.p->flags;
    SALVA_HIP_CHECK(hipMemset(d_rb.p, 0, sizeof(Readback)));
    {
        mass_slots.ensure(2 * MASS_SLOTS);  // (k_cell_keys' "a mass differs" flags + the reference bits, grid.hip)
        SALVA_HIP_CHECK(hipMemset(mass_slots.p, 0, 2 * MASS_SLOTS * sizeof(uint32_t)));
    }
    d_counters.ensure(4);
    for (auto& e2 : ev) SALVA_HIP_CHECK(hipEventCreate(&e2));
    for (auto& e2 : evc) SALVA_HIP_CHECK(hipEventCreate(&e2));
    SALVA_HIP_CHECK(hipEventCreateWithFlags(&ev_sync, hipEventDisableTiming));
}

World::~World() {
    (void)hipSetDevice(prm.device);
    if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
    if (stream2) { (void)hipStreamSynchronize(stream2); (void)hipStreamDestroy(stream2); }
    if (dl_stream) { (void)hipStreamSynchronize(dl_stream); (void)hipStreamDestroy(dl_stream); }
    if (ev_dl_ready) (void)hipEventDestroy(ev_dl_ready);
    if (ev_dl_done) (void)hipEventDestroy(ev_dl_done);
    for (float* p : h_dl) if (p) (void)hipHostFree(p);
    for (hipEvent_t e : dist_ev) if (e) (void)hipEventDestroy(e);
    if (ev_pre_refresh) (void)hipEventDestroy(ev_pre_refresh);
    if (ev_interior) (void)hipEventDestroy(ev_interior);
    if (ev_spec_eval) (void)hipEventDestroy(ev_spec_eval);
    if (ev_spec_apply) (void)hipEventDestroy(ev_spec_apply);
    if (h_rb) (void)hipHostFree(h_rb);
    if (h_ctl) (void)hipHostFree(h_ctl);
    if (h_pub) (void)hipHostFree(h_pub);
    if (h_hostpub) (void)hipHostFree(h_hostpub);
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : evc) if (e) (void)hipEventDestroy(e);
    if (ev_sync) (void)hipEventDestroy(ev_sync);
}

void World::use_device() const { SALVA_HIP_CHECK(hipSetDevice(prm.device)); }

uint64_t World::fluid_offset(uint32_t slot) const {
    uint64_t o = 0;
    for (uint32_t s = 0; s < slot; ++s) o += fluids[s].n;
    return o;
}
uint64_t World::boundary_offset(uint32_t slot) const {
    uint64_t o = 0;
    for (uint32_t s = 0; s < slot; ++s) o += bounds[s].n;
    return o;
}

FluidArrays World::arrays(int which) {
    FluidArrays a;
    a.posm = posm[which].p; a.vel = vel[which].p; a.dv = dv[which].p; a.model = model[which].p; a.perm = perm[which].p;
    a.gtag = comm ? gtag[which].p : nullptr;
    return a;
}

void World::ensure_cub_temp(size_t bytes) { cub_temp.ensure(bytes ? bytes : 1, stream, false, 1.25f); }

// Bring the canonical (host-order) staging arrays up to date with the sorted working set.
void World::ensure_staging_current() {
    if (staging_current) return;
    if (comm && dist_started)
        throw HipError(SALVA_HIP_E_INVALID, "host-order fluid arrays are not maintained in a multi-GPU run: use salva_hip_get_owned");
    if (sorted_valid && n) {
        launch_sorted_to_stage(n, arrays(cur), st_pos.p, st_vel.p, st_dv.p, stream);
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
    staging_current = true;
}

// ------------------------------------------------------------------------------------------------ fluids
void World::set_fluid(uint32_t slot, uint64_t nn, const float* pos, const float* vel_h, const float* vol,
                      const float* acc_h, const float* dvs, float density0, uint32_t memberships, uint32_t filter,
                      uint32_t dirty) {
    use_device();
    if (slot > fluids.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot out of range (slots are dense)");
    if (slot >= (uint32_t)MAX_MODELS) throw HipError(SALVA_HIP_E_CAPACITY, "at most 32 fluids per world");
    const bool is_new = slot == fluids.size();
    if ((uint64_t)n - (is_new ? 0 : fluids[slot].n) + nn >= 0xfffffff0ull)
        throw HipError(SALVA_HIP_E_CAPACITY, "more than 2^32 fluid particles on one device");
    ensure_staging_current();
    const uint64_t old_n = is_new ? 0 : fluids[slot].n;
    const bool resized = is_new || old_n != nn;
    if (resized) {
        if (nn && !pos) throw HipError(SALVA_HIP_E_INVALID, "positions are required when a fluid is created or resized");
        dirty = SALVA_HIP_DIRTY_ALL;
    }
    if (is_new) fluids.emplace_back();
    const uint64_t off = fluid_offset(slot);
    const uint64_t old_total = n;
    const uint64_t new_total = old_total - old_n + nn;
    if (resized) {
        std::vector<Piece> pieces = {{0, off, true}, {0, nn, false}, {off + old_n, old_total - off - old_n, true}};
        rebuild(st_pos, pieces, new_total, stream);
        rebuild(st_vel, pieces, new_total, stream);
        rebuild(st_dv, pieces, new_total, stream);
        rebuild(st_acc, pieces, new_total, stream);
        rebuild(st_model, pieces, new_total, stream);
        n = (uint32_t)new_total;
        if (nn) {
            // defaults: zero velocity / velocity change / acceleration, Fluid::particle_volume (fluid.rs:110-120)
            const float r = prm.particle_radius;
            const float default_vol = r * r * r * 6.4f;  // 8 * 0.8
            k_fill_f4<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, st_pos.p + off, make_float4(0, 0, 0, default_vol), 0);
            k_fill_f4<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, st_vel.p + off, make_float4(0, 0, 0, 0), 0);
            k_fill_f4<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, st_dv.p + off, make_float4(0, 0, 0, 0), 0);
            k_fill_f4<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, st_acc.p + off, make_float4(0, 0, 0, 0), 0);
        }
        if (is_new && !dvs) {
            auto it = sticky.find(slot);
            if (it != sticky.end()) {  // buffer[slot] of a fluid removed since the last step: inherited (world.h `sticky`)
                const uint64_t inherit = std::min<uint64_t>(it->second.len, nn);
                if (inherit) SALVA_HIP_CHECK(hipMemcpyAsync(st_dv.p + off, it->second.data->p, inherit * sizeof(float4), hipMemcpyDeviceToDevice, stream));
                if (it->second.len <= nn) sticky.erase(it);
            }
        }
        // model ids of every slot at/after this one may have moved
        fluids[slot].n = nn;
        stamp_fluid_models();
    }
    FluidSlot& f = fluids[slot];
    f.density0 = density0; f.memberships = memberships; f.filter = filter;
    {   // the fluid's one volume, if it has one (FluidSlot::vol_uniform): a resize filled the default in, an upload may change it
        const float r = prm.particle_radius;
        if (resized) f.vol_uniform = r * r * r * 6.4f;
        if (nn && (dirty & SALVA_HIP_DIRTY_VOLUMES) && vol) {
            bool same = true;
            for (uint64_t k = 1; k < nn && same; ++k) same = vol[k] == vol[0];
            f.vol_uniform = same ? vol[0] : std::numeric_limits<float>::quiet_NaN();
        }
    }
    auto upload3 = [&](const float* src, float4* dst, int keep_w) {
        scratch_f.ensure(3 * nn, stream, false, 1.1f);
        SALVA_HIP_CHECK(hipMemcpyAsync(scratch_f.p, src, 3 * nn * sizeof(float), hipMemcpyHostToDevice, stream));
        k_pack_xyz<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, scratch_f.p, dst, keep_w, 0.0f);
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    };
    if (nn) {
        if ((dirty & SALVA_HIP_DIRTY_POSITIONS) && pos) upload3(pos, st_pos.p + off, 1);
        if ((dirty & SALVA_HIP_DIRTY_VELOCITIES) && vel_h) upload3(vel_h, st_vel.p + off, 1);
        if ((dirty & SALVA_HIP_DIRTY_VOLUMES) && vol) {
            scratch_f.ensure(nn, stream, false, 1.1f);
            SALVA_HIP_CHECK(hipMemcpyAsync(scratch_f.p, vol, nn * sizeof(float), hipMemcpyHostToDevice, stream));
            k_pack_w<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, scratch_f.p, st_pos.p + off);
            SALVA_HIP_CHECK(hipStreamSynchronize(stream));
        }
        if ((dirty & SALVA_HIP_DIRTY_ACCELERATIONS) && acc_h) {
            // accelerations are zero between steps; the first user upload must not resurrect stale staging values
            if (!acc_user) SALVA_HIP_CHECK(hipMemsetAsync(st_acc.p, 0, (size_t)n * sizeof(float4), stream));
            upload3(acc_h, st_acc.p + off, 1);
            acc_user = true;
        }
        if (dvs) upload3(dvs, st_dv.p + off, 1);
    }
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    sorted_valid = false;
    bbox_known = false;
    tables_dirty = true;
    have_last_ctx = false;
}

// Fluid::add_particles (fluid.rs:126-150): append to the fluid's arrays — default volume, zero acceleration, zero
// velocity change (the solver's buffers grow with zeros, dfsph_solver.rs:526-549) — without re-uploading the rest.
void World::add_particles(uint32_t slot, uint64_t n_add, const float* pos, const float* vel_h) {
    use_device();
    if (slot >= fluids.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot out of range");
    if (comm && dist_started) { dist_add_particles(slot, n_add, pos, vel_h); return; }  // (collective, world_dist.hip)
    if (n_add == 0) return;
    if (!pos) throw HipError(SALVA_HIP_E_INVALID, "positions are required");
    const uint64_t at = append_particles(slot, n_add);
    scratch_f.ensure(3 * n_add, stream, false, 1.1f);
    SALVA_HIP_CHECK(hipMemcpyAsync(scratch_f.p, pos, 3 * n_add * sizeof(float), hipMemcpyHostToDevice, stream));
    k_pack_xyz<<<nblk(n_add), BLOCK, 0, stream>>>((uint32_t)n_add, scratch_f.p, st_pos.p + at, 1, 0.0f);
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    if (vel_h) {
        SALVA_HIP_CHECK(hipMemcpyAsync(scratch_f.p, vel_h, 3 * n_add * sizeof(float), hipMemcpyHostToDevice, stream));
        k_pack_xyz<<<nblk(n_add), BLOCK, 0, stream>>>((uint32_t)n_add, scratch_f.p, st_vel.p + at, 1, 0.0f);
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
}

// The growing half of add_particles: room for n_add particles behind the fluid's last one, filled with the defaults (zero position,
// velocity and acceleration, default volume, the inherited velocity-change tail).  Returns the staging index of the first new
// particle; the caller writes positions (and velocities) there — from the host (add_particles) or on the device
// (add_particles_sampled, sample.hip).
uint64_t World::append_particles(uint32_t slot, uint64_t n_add) {
    if ((uint64_t)n + n_add >= 0xfffffff0ull) throw HipError(SALVA_HIP_E_CAPACITY, "more than 2^32 fluid particles on one device");
    ensure_staging_current();
    const uint64_t old_n = fluids[slot].n, off = fluid_offset(slot), at = off + old_n, old_total = n, new_total = old_total + n_add;
    std::vector<Piece> pieces = {{0, at, true}, {0, n_add, false}, {at, old_total - at, true}};
    rebuild(st_pos, pieces, new_total, stream);
    rebuild(st_vel, pieces, new_total, stream);
    rebuild(st_dv, pieces, new_total, stream);
    rebuild(st_acc, pieces, new_total, stream);
    rebuild(st_model, pieces, new_total, stream);
    n = (uint32_t)new_total;
    fluids[slot].n = old_n + n_add;
    {   // (the new particles have the default volume: the fluid keeps ONE volume only if that is the one it had)
        const float r = prm.particle_radius, default_vol = r * r * r * 6.4f;
        FluidSlot& f = fluids[slot];
        if (old_n == 0) f.vol_uniform = default_vol;
        else if (!(f.vol_uniform == default_vol)) f.vol_uniform = std::numeric_limits<float>::quiet_NaN();
    }
    const float r = prm.particle_radius;
    k_fill_f4<<<nblk(n_add), BLOCK, 0, stream>>>((uint32_t)n_add, st_pos.p + at, make_float4(0, 0, 0, r * r * r * 6.4f), 0);
    k_fill_f4<<<nblk(n_add), BLOCK, 0, stream>>>((uint32_t)n_add, st_vel.p + at, make_float4(0, 0, 0, 0), 0);
    k_fill_f4<<<nblk(n_add), BLOCK, 0, stream>>>((uint32_t)n_add, st_dv.p + at, make_float4(0, 0, 0, 0), 0);
    k_fill_f4<<<nblk(n_add), BLOCK, 0, stream>>>((uint32_t)n_add, st_acc.p + at, make_float4(0, 0, 0, 0), 0);
    {
        auto it = sticky.find(slot);
        if (it != sticky.end() && it->second.len > old_n) {  // `velocity_changes[slot].resize(n)` exposes the inherited tail
            const uint64_t take = std::min<uint64_t>(it->second.len - old_n, n_add);
            SALVA_HIP_CHECK(hipMemcpyAsync(st_dv.p + at, it->second.data->p + old_n, take * sizeof(float4), hipMemcpyDeviceToDevice, stream));
        }
    }
    stamp_fluid_models();
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    sorted_valid = false; bbox_known = false; tables_dirty = true; have_last_ctx = false;
    return at;
}

// Fluid::apply_particles_removal (fluid.rs:88-98) together with the compaction of the solver's velocity_changes
// (dfsph_solver.rs:550-560 / iisph_solver.rs:505-537): a stable compaction (`filter_from_mask`, helper.rs:4-12) of every
// per-particle array of the fluid, on the device.  `mask[i] != 0` deletes particle i.  Returns the remaining count.
uint64_t World::delete_particles(uint32_t slot, const uint8_t* mask) {
    use_device();
    if (slot >= fluids.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot out of range");
    if (comm && dist_started) throw HipError(SALVA_HIP_E_INVALID, "host indices do not exist in a running multi-GPU world: delete by global id (salva_hip_delete_owned)");
    const uint64_t nn = fluids[slot].n, off = fluid_offset(slot);
    if (nn == 0 || !mask) return nn;
    ensure_staging_current();
    // keep flags over the whole staging range (other fluids are kept)
    std::vector<uint8_t> keep((size_t)n, 1);
    uint64_t kept = 0;
    for (uint64_t k = 0; k < nn; ++k) { keep[off + k] = mask[k] ? 0 : 1; kept += keep[off + k]; }
    if (kept == nn) return nn;
    DevBuf<uint8_t> d_keep;
    DevBuf<uint32_t> d_num;
    d_keep.ensure(n); d_num.ensure(1);
    SALVA_HIP_CHECK(hipMemcpyAsync(d_keep.p, keep.data(), (size_t)n, hipMemcpyHostToDevice, stream));
    const uint64_t new_total = (uint64_t)n - (nn - kept);
    auto compact = [&](DevBuf<float4>& buf) {
        DevBuf<float4> out;
        out.ensure(std::max<uint64_t>(new_total, 1));
        const size_t tb = select_flagged_temp_bytes(n);
        ensure_cub_temp(tb);
        select_flagged_f4(cub_temp.p, tb, buf.p, d_keep.p, out.p, d_num.p, n, stream);
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
        std::swap(buf.p, out.p);
        std::swap(buf.cap, out.cap);
    };
    compact(st_pos); compact(st_vel); compact(st_dv); compact(st_acc);
    {
        // an inherited solver buffer (world.h `sticky`) is filtered with the same mask by the reference — after its resize, so
        // the entries beyond the fluid's particles (handed to particles added before the next step) just move down
        auto it = sticky.find(slot);
        if (it != sticky.end() && it->second.len) {
            const uint64_t L = it->second.len, head = std::min<uint64_t>(L, nn);
            std::vector<uint8_t> k2((size_t)L, 1);
            uint64_t kept2 = 0;
            for (uint64_t k = 0; k < L; ++k) { if (k < head) k2[k] = mask[k] ? 0 : 1; kept2 += k2[k]; }
            DevBuf<uint8_t> d_k2;
            d_k2.ensure(L);
            SALVA_HIP_CHECK(hipMemcpyAsync(d_k2.p, k2.data(), (size_t)L, hipMemcpyHostToDevice, stream));
            auto out = std::make_shared<DevBuf<float4>>();
            out->ensure(std::max<uint64_t>(kept2, 1));
            const size_t tb = select_flagged_temp_bytes((uint32_t)L);
            ensure_cub_temp(tb);
            select_flagged_f4(cub_temp.p, tb, it->second.data->p, d_k2.p, out->p, d_num.p, (uint32_t)L, stream);
            SALVA_HIP_CHECK(hipStreamSynchronize(stream));
            it->second.data = out;
            it->second.len = kept2;
        }
    }
    n = (uint32_t)new_total;
    fluids[slot].n = kept;
    stamp_fluid_models();
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    sorted_valid = false; bbox_known = false; tables_dirty = true; have_last_ctx = false;
    return kept;
}

void World::set_fluid_forces(uint32_t slot, const SalvaHipForceDesc* f, uint32_t nf) {
    if (slot >= fluids.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot out of range");
    for (uint32_t k = 0; k < nf; ++k)
        if (f[k].kind < SALVA_HIP_FORCE_XSPH || f[k].kind > SALVA_HIP_FORCE_DEVICE)
            throw HipError(SALVA_HIP_E_INVALID, "unknown non-pressure force kind (only built-ins run on the device)");
    for (uint32_t k = 0; k < nf; ++k)
        if (f[k].kind == SALVA_HIP_FORCE_DEVICE) {
            if (comm)  // ghost rows and the local view's ownership rules are not part of SalvaHipDeviceView
                throw HipError(SALVA_HIP_E_INVALID, "SALVA_HIP_FORCE_DEVICE is not available in a decomposed world (salva_hip_set_domain)");
            if (!(f[k].p[0] >= 0.0f && f[k].p[0] <= 7.0f && f[k].p[0] == (float)(uint32_t)f[k].p[0]))
                throw HipError(SALVA_HIP_E_INVALID, "SALVA_HIP_FORCE_DEVICE: p[0] must be a sum of SALVA_HIP_DEVICE_NEEDS_* bits (0 ... 7)");
        }
    for (uint32_t k = 0; k < nf; ++k)
        if (f[k].kind == SALVA_HIP_FORCE_BECKER2009) {
            if (comm)  // the rest lists cross slabs and have no ghost protocol
                throw HipError(SALVA_HIP_E_INVALID, "Becker2009Elasticity is not available in a decomposed world (salva_hip_set_domain)");
            for (int q = 3; q < 5; ++q)
                if (!(f[k].p[q] == 0.0f || f[k].p[q] == 1.0f || f[k].p[q] == 2.0f || f[k].p[q] == 3.0f))
                    throw HipError(SALVA_HIP_E_INVALID, "Becker2009Elasticity: p[3] / p[4] must be a SALVA_HIP_KERNEL_* kind");
        }
    for (uint32_t k = 0; k < nf; ++k)
        if (f[k].kind == SALVA_HIP_FORCE_DFSPH_VISCOSITY && !(f[k].p[0] >= 0.0f && f[k].p[0] <= 1.0f))
            throw HipError(SALVA_HIP_E_INVALID, "The viscosity coefficient must be between 0.0 and 1.0.");  // dfsph_viscosity.rs:104-108
    for (uint32_t k = 0; k < nf; ++k)
        if (f[k].kind == SALVA_HIP_FORCE_WCSPH_TENSION && f[k].p[1] != 0.0f)
            // wcsph_surface_tension.rs:66-83 walks the fluid-fluid contacts while indexing the boundaries: it panics
            throw HipError(SALVA_HIP_E_INVALID, "WCSPHSurfaceTension: a non-zero boundary coefficient panics in the reference (index out of bounds)");
    // an elastic entry keeps its state when entry k is what it was (same kind, bit-identical p[]): the Python mirror re-uploads the
    // whole list when any coefficient changes, and a block must not lose its rest shape because another force was appended
    FluidSlot& fs = fluids[slot];
    std::vector<std::shared_ptr<ElasticState>> el(nf);
    for (uint32_t k = 0; k < nf; ++k)
        if (f[k].kind == SALVA_HIP_FORCE_BECKER2009 && k < fs.forces.size() && k < fs.elastic.size() && fs.elastic[k] &&
            fs.forces[k].kind == f[k].kind && memcmp(fs.forces[k].p, f[k].p, sizeof(f[k].p)) == 0)
            el[k] = fs.elastic[k];
    fs.forces.assign(f, f + nf);
    fs.elastic = std::move(el);
}

void World::remove_fluid(uint32_t slot) {
    use_device();
    if (slot >= fluids.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot out of range");
    ensure_staging_current();
    // ContiguousArena::remove is a swap-remove (contiguous_arena.rs): the last fluid takes the freed slot.
    const uint32_t last = (uint32_t)fluids.size() - 1;
    const uint64_t off = fluid_offset(slot), len = fluids[slot].n;
    const uint64_t loff = fluid_offset(last), llen = fluids[last].n;
    std::vector<Piece> pieces;
    pieces.push_back({0, off, true});
    if (slot != last) {
        pieces.push_back({loff, llen, true});
        pieces.push_back({off + len, loff - off - len, true});
    }
    const uint64_t new_total = n - len;
    rebuild(st_pos, pieces, new_total, stream);
    rebuild(st_vel, pieces, new_total, stream);
    {
        // The solver's per-fluid buffers are positional in the reference and are NOT swapped with the object
        // (liquid_world.rs:171-173 removes from the arena only; init_with_fluids then resizes `velocity_changes[slot]` /
        // `pressures[slot]` to the new occupant's particle count, dfsph_solver.rs:526-549 / iisph_solver.rs:479-501): the
        // fluid that moves into the freed slot inherits the removed fluid's velocity changes and pressures, truncated
        // or zero-extended, and the buffer of the last slot lives on until the next step (a fluid added before then
        // inherits it).  Reproduced: results must match the reference's, quirks included.  See `sticky` in world.h.
        auto content_of = [&](uint32_t sl, uint64_t o, uint64_t l) {
            auto it = sticky.find(sl);
            if (it != sticky.end()) return it->second;
            StickyBuf b;
            b.data = std::make_shared<DevBuf<float4>>();
            b.len = l;
            b.data->ensure(std::max<uint64_t>(l, 1));
            if (l) SALVA_HIP_CHECK(hipMemcpyAsync(b.data->p, st_dv.p + o, l * sizeof(float4), hipMemcpyDeviceToDevice, stream));
            return b;
        };
        const StickyBuf A = content_of(slot, off, len);
        const StickyBuf B = slot != last ? content_of(last, loff, llen) : StickyBuf{};
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
        std::vector<Piece> dvp;
        dvp.push_back({0, off, true});
        if (slot != last) {
            dvp.push_back({0, llen, false});
            dvp.push_back({off + len, loff - off - len, true});
        }
        rebuild(st_dv, dvp, new_total, stream);
        sticky.erase(slot);
        sticky.erase(last);
        if (slot != last) {
            const uint64_t inherit = std::min(A.len, llen);
            if (inherit) SALVA_HIP_CHECK(hipMemcpyAsync(st_dv.p + off, A.data->p, inherit * sizeof(float4), hipMemcpyDeviceToDevice, stream));
            if (llen > inherit) SALVA_HIP_CHECK(hipMemsetAsync(st_dv.p + off + inherit, 0, (llen - inherit) * sizeof(float4), stream));
            if (A.len > llen) sticky[slot] = A;  // its tail goes to particles added before the next step
            sticky[last] = B;
        } else {
            sticky[last] = A;
        }
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
    rebuild(st_acc, pieces, new_total, stream);
    rebuild(st_model, pieces, new_total, stream);
    if (slot != last) fluids[slot] = fluids[last];
    fluids.pop_back();
    n = (uint32_t)new_total;
    stamp_fluid_models();
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    sorted_valid = false; bbox_known = false; tables_dirty = true; have_last_ctx = false;
}

// ------------------------------------------------------------------------------------------------ boundaries
void World::set_boundary(uint32_t slot, uint64_t nn, const float* pos, const float* vel_h, uint32_t memberships,
                         uint32_t filter, bool wants_forces) {
    set_boundary_from(slot, nn, pos, vel_h, memberships, filter, wants_forces, nullptr);
}

// fill_dev != nullptr: the positions are written on the device — (*fill_dev)(first float4 of the slot), enqueued on the world's
// stream — instead of uploaded from `pos` (set_boundary_sampling_from_shape, sample.hip)
void World::set_boundary_from(uint32_t slot, uint64_t nn, const float* pos, const float* vel_h, uint32_t memberships, uint32_t filter,
                              bool wants_forces, const std::function<void(float4*)>* fill_dev) {
    use_device();
    if (slot > bounds.size()) throw HipError(SALVA_HIP_E_INVALID, "boundary slot out of range (slots are dense)");
    const bool is_new = slot == bounds.size();
    const uint64_t old_n = is_new ? 0 : bounds[slot].n;
    if ((uint64_t)nb - old_n + nn >= 0xfffffff0ull) throw HipError(SALVA_HIP_E_CAPACITY, "too many boundary particles");
    if (nn && !pos && !fill_dev) throw HipError(SALVA_HIP_E_INVALID, "boundary positions are required");
    if (is_new) bounds.emplace_back();
    const uint64_t off = boundary_offset(slot);
    const uint64_t old_total = nb, new_total = old_total - old_n + nn;
    const bool resized = is_new || old_n != nn;
    if (resized) {
        std::vector<Piece> pieces = {{0, off, true}, {0, nn, false}, {off + old_n, old_total - off - old_n, true}};
        rebuild(bst_pos, pieces, new_total, stream);
        rebuild(bst_vel, pieces, new_total, stream);
        rebuild(bforce, pieces, new_total, stream);
        nb = (uint32_t)new_total;
        if (nn) {
            k_fill_f4<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, bst_pos.p + off, make_float4(0, 0, 0, 0), 0);
            k_fill_f4<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, bst_vel.p + off, make_float4(0, 0, 0, 0), 0);
            k_fill_f4<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, bforce.p + off, make_float4(0, 0, 0, 0), 0);
        }
    }
    BoundarySlot& b = bounds[slot];
    b.n = nn; b.memberships = memberships; b.filter = filter; b.wants_forces = wants_forces;
    b.dyn.reset();  // (re)uploading particles makes it a plain boundary; the sampling setters mark it again
    b.vel_zero = true;
    if (nn) {
        scratch_f.ensure(3 * nn, stream, false, 1.1f);
        if (fill_dev) {
            (*fill_dev)(bst_pos.p + off);
        } else {
            SALVA_HIP_CHECK(hipMemcpyAsync(scratch_f.p, pos, 3 * nn * sizeof(float), hipMemcpyHostToDevice, stream));
            k_pack_xyz<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, scratch_f.p, bst_pos.p + off, 0, 0.0f);
        }
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
        b.vel_zero = true;
        if (vel_h)
            for (uint64_t k = 0; k < 3 * nn && b.vel_zero; ++k) b.vel_zero = vel_h[k] == 0.0f;
        if (vel_h) {
            SALVA_HIP_CHECK(hipMemcpyAsync(scratch_f.p, vel_h, 3 * nn * sizeof(float), hipMemcpyHostToDevice, stream));
            k_pack_xyz<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, scratch_f.p, bst_vel.p + off, 0, 0.0f);
        } else {
            k_fill_f4<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, bst_vel.p + off, make_float4(0, 0, 0, 0), 0);
        }
    }
    // boundary model ids ride in bst_vel.w
    stamp_boundary_models();
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    b_dirty = true; tables_dirty = true; have_last_ctx = false;
}

void World::remove_boundary(uint32_t slot) {
    use_device();
    if (slot >= bounds.size()) throw HipError(SALVA_HIP_E_INVALID, "boundary slot out of range");
    const uint32_t last = (uint32_t)bounds.size() - 1;
    const uint64_t off = boundary_offset(slot), len = bounds[slot].n;
    const uint64_t loff = boundary_offset(last), llen = bounds[last].n;
    std::vector<Piece> pieces;
    pieces.push_back({0, off, true});
    if (slot != last) {
        pieces.push_back({loff, llen, true});
        pieces.push_back({off + len, loff - off - len, true});
    }
    const uint64_t new_total = nb - len;
    rebuild(bst_pos, pieces, new_total, stream);
    rebuild(bst_vel, pieces, new_total, stream);
    rebuild(bforce, pieces, new_total, stream);
    if (slot != last) bounds[slot] = bounds[last];
    bounds.pop_back();
    nb = (uint32_t)new_total;
    stamp_boundary_models();
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    b_dirty = true; tables_dirty = true; have_last_ctx = false;
}

// ------------------------------------------------------------------------------------------------ tables
// InteractionGroups::test (interaction_groups.rs:64-69)
static inline bool groups_test(uint32_t m1, uint32_t f1, uint32_t m2, uint32_t f2) {
    return (m1 & f2) != 0 && (m2 & f1) != 0;
}

void World::upload_tables() {
    if (!tables_dirty) return;
    lists_checked = sw.trust_cap0;  // the objects changed: the next step checks the list capacity before it solves (World::step)
    const uint32_t nm = num_models(), nbm = (uint32_t)std::max<size_t>(bounds.size(), 1);
    std::vector<float> r0(nm, 1000.0f);
    std::vector<uint32_t> counts(nm, 0);
    std::vector<uint8_t> ff(nm * nm, 1), fb(nm * nbm, 1), bb(nbm * nbm, 1), bw(nbm, 0);
    any_wants_forces = false;
    for (uint32_t a = 0; a < fluids.size(); ++a) {
        r0[a] = fluids[a].density0;
        counts[a] = (uint32_t)fluids[a].n;
        for (uint32_t b = 0; b < fluids.size(); ++b)  // a fluid always interacts with itself (contacts.rs:350-358)
            ff[a * nm + b] = (a == b) || groups_test(fluids[a].memberships, fluids[a].filter, fluids[b].memberships, fluids[b].filter);
        for (uint32_t b = 0; b < bounds.size(); ++b)
            fb[a * nbm + b] = groups_test(fluids[a].memberships, fluids[a].filter, bounds[b].memberships, bounds[b].filter);
    }
    for (uint32_t a = 0; a < bounds.size(); ++a) {
        bw[a] = bounds[a].wants_forces ? 1 : 0;
        any_wants_forces |= bounds[a].wants_forces;
        for (uint32_t b = 0; b < bounds.size(); ++b)
            bb[a * nbm + b] = (a == b) || groups_test(bounds[a].memberships, bounds[a].filter, bounds[b].memberships, bounds[b].filter);
    }
    rho0_tab.ensure(nm); model_counts.ensure(nm); ff_ok.ensure(nm * nm); fb_ok.ensure(nm * nbm); bb_ok.ensure(nbm * nbm); bwants.ensure(nbm);
    SALVA_HIP_CHECK(hipMemcpyAsync(rho0_tab.p, r0.data(), nm * sizeof(float), hipMemcpyHostToDevice, stream));
    // (decomposed runs: the error averages divide by the GLOBAL particle count of each fluid, all-reduced once by
    // dist_prepare — a later table upload, e.g. after the caller re-uploaded boundaries for a re-cut slab, must not put the
    // local counts back: the ranks would then disagree on convergence and fall out of step)
    if (comm && dist_started && global_counts.size() == nm) counts = global_counts;
    SALVA_HIP_CHECK(hipMemcpyAsync(model_counts.p, counts.data(), nm * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    SALVA_HIP_CHECK(hipMemcpyAsync(ff_ok.p, ff.data(), ff.size(), hipMemcpyHostToDevice, stream));
    SALVA_HIP_CHECK(hipMemcpyAsync(fb_ok.p, fb.data(), fb.size(), hipMemcpyHostToDevice, stream));
    SALVA_HIP_CHECK(hipMemcpyAsync(bb_ok.p, bb.data(), bb.size(), hipMemcpyHostToDevice, stream));
    SALVA_HIP_CHECK(hipMemcpyAsync(bwants.p, bw.data(), bw.size(), hipMemcpyHostToDevice, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));  // host vectors go out of scope
    tables_dirty = false;
    b_dirty = true;  // group changes alter the boundary-boundary sums
}

float World::bforce_scale() const {
    const float r = prm.particle_radius;
    return std::exp2f(36.0f - std::ceil(std::log2(1000.0f * r * r * r)));
}

StepCtx World::make_ctx() {
    StepCtx c{};
    if (any_wants_forces && bforce_fx_n != nb) {  // (all zero between steps: a change of the boundary set starts from zeros again)
        bforce_fx.ensure(3 * (size_t)std::max<uint32_t>(nb, 1u), stream, false, 1.2f);
        SALVA_HIP_CHECK(hipMemsetAsync(bforce_fx.p, 0, 3 * (size_t)std::max<uint32_t>(nb, 1u) * sizeof(unsigned long long), stream));
        bforce_fx_n = nb;
    }
    c.sc = sc;
    {   // groups of 64 slots (what one XCD's 32 CUs hold at a time), fewer for launches of less than 1024 tiles
        uint32_t lg = 1u;
        while (lg < 7u && (16u << lg) <= pass.nlaunch) ++lg;
        c.xcd = lg;
    }
    c.n = n;
    c.posm = posm[cur].p; c.vel = vel[cur].p; c.dv = dv[cur].p; c.acc = acc.p; c.w = w.p; c.normal = normal.p;
    c.model = model[cur].p; c.perm = perm[cur].p; c.gtag = comm ? gtag[cur].p : nullptr;
    c.rho = rho.p; c.alpha = alpha.p; c.kappa = kappa.p; c.kappa2 = kappa2.p; c.rho_star = rho_star.p; c.aii = aii.p;
    c.dii = dii.p; c.dijpj = dijpj.p; c.iisph_q = iisph_q.p; c.iisph_pr = iisph_pr.p; c.posmr = posmr.p;
    c.nff = nff.p; c.nfb = nfb.p;
    c.nbr_ff = nbr_ff.p; c.nbr_fb = nbr_fb.p; c.cap_ff = cap_ff; c.cap_fb = cap_fb;
    c.slice_near = slice_near.p;
    c.tile_off = G().tile_off.p; c.halo_src = halo_src.p; c.bhalo_src = bhalo_src.p;
    c.halo_stride = halo_stride; c.bhalo_stride = bhalo_stride;
    c.ntiles = (uint32_t)gf.ntiles();
    c.split_s = pass.split_s_cur;
    c.slot_order = (pass.class_ntiny || pass.class_nlight) ? slot_order.p : nullptr; c.slot_base = 0u; c.ntiny = pass.class_ntiny; c.nlight = pass.class_nlight;
    c.tile_ids = G().tile_ids.p; c.tile_rank = G().tile_rank.p; c.nlaunch = pass.nlaunch; c.slot_desc = G().slot_desc.p; c.slot_info = slot_info.p;
    c.spec = pass.spec_mode ? 1u : 0u; c.halo_cap = pass.halo_cap; c.bhalo_cap = pass.bhalo_cap; c.nslices_cap = pass.nslices_cap;
    c.halo_len = pass.halo_len; c.bhalo_len = pass.bhalo_len;
    c.gf = gf.device(G().cell_start_f.p);
    c.stale_keys = has_dynamic_sampling() ? G().keys[1].p : nullptr;
    c.nb = nb;
    c.bposv = bposv.p; c.bvel = bvel.p; c.bperm = bperm.p;
    c.bforce = any_wants_forces ? bforce.p : nullptr;
    c.bforce_fx = any_wants_forces ? bforce_fx.p : nullptr;
    c.bforce_scale = bforce_scale();
    c.bwants = bwants.p;
    c.gb = gb.device(cell_start_b.p);
    c.nmodels = num_models();
    c.nbmodels = (uint32_t)std::max<size_t>(bounds.size(), 1);
    c.mass_uniform = mass_uniform;
    c.two_mass = pass.two_mass ? 1u : 0u;
    c.nmass = pass.two_mass ? pass.nmass : 0u; c.cmask = pass.mass_cmask;
    for (int k = 0; k < 4; ++k) c.class_mass[k] = pass.mass_classes[k];
    c.tile_mass_bits = pass.two_mass ? tile_mass_bits.p : nullptr;
    c.tile_massb_bits = pass.two_mass ? tile_massb_bits.p : nullptr;
    c.tile_masscd_bits = (pass.two_mass && pass.nmass > 2u) ? tile_masscd_bits.p : nullptr;
    c.nffb = pass.two_mass ? nffb.p : nullptr;
    c.nffc = (pass.two_mass && pass.nmass > 2u) ? nffc.p : nullptr;
    c.bvel_zero = 1u;  // no boundary particle moves: the passes that subtract a boundary velocity need not stage it
    for (const BoundarySlot& b : bounds) if (b.n && (!b.vel_zero || b.sampling || b.dyn)) c.bvel_zero = 0u;
    c.rho0_tab = rho0_tab.p; c.rho0_single = fluids.empty() ? 1000.0f : fluids[0].density0; c.ff_ok = ff_ok.p; c.fb_ok = fb_ok.p; c.bb_ok = bb_ok.p;
    c.partials = partials.p;
    c.spec_k = -1; c.spec_ring = spec_ring.p; c.spec_pub = nullptr; c.model_counts = model_counts.p; c.w2 = w2.p;
    c.flags = d_flags.p;
    c.min_neighbors_for_divergence = 20;  // dfsph_solver.rs:62 (DIM == 3)
    c.phase = 0;
    c.ghost_lo_cx = (comm && comm->has_lo()) ? slab_lo - 1 : INT32_MIN;
    c.ghost_hi_cx = (comm && comm->has_hi()) ? slab_hi + 1 : INT32_MAX;
    return c;
}

// Tile grid over a cell bounding box.  The origin is the box's own minimum corner, so a block of fluid is cut into
// the same number of tiles wherever it sits (an absolute tile lattice would add a partially filled layer of tiles per
// axis whenever the block is not aligned with it).  Fluid and boundary grids have independent origins: a fluid
// tile looks boundary cells up by absolute cell coordinates.
// `fold` (fluid grid only): when the box holds more than fold->budget cells, fold its longest axes to power-of-two periods — never
// below fold->min_period[a] — until it does (device_types.h TileGrid: the table becomes a torus, the lists stay what they were).
void dims_from_bbox(const int32_t* bb, GridDims& g, const FoldRule* fold) {
    static const int T[3] = {TX, TY, TZ};
    int64_t cells[3];
    for (int a = 0; a < 3; ++a) {
        if (bb[a] > bb[3 + a]) throw HipError(SALVA_HIP_E_CAPACITY, "empty cell bounding box");
        const int64_t extent = (int64_t)bb[3 + a] - (int64_t)bb[a] + 1;
        if (extent > (1 << 30)) throw HipError(SALVA_HIP_E_CAPACITY, "cell bounding box too large");
        g.o[a] = bb[a];
        g.nt[a] = (int)((extent + T[a] - 1) / T[a]);
        g.mask[a] = 0xffffffffu;
        cells[a] = (int64_t)g.nt[a] * T[a];
    }
    if (fold && (double)cells[0] * (double)cells[1] * (double)cells[2] > fold->budget) {
        for (;;) {
            if ((double)cells[0] * (double)cells[1] * (double)cells[2] <= fold->target) break;
            // the longest axis that can still be folded: to the largest power of two below its present length
            int best = -1;
            int64_t best_p = 0;
            for (int a = 0; a < 3; ++a) {
                int64_t p = 1;
                while (p * 2 < cells[a]) p *= 2;
                if (!fold->axis[a] || p < (int64_t)fold->min_period[a] || p >= cells[a]) continue;
                if (best < 0 || cells[a] > cells[best]) { best = a; best_p = p; }
            }
            if (best < 0) break;  // (nothing left to fold: the budget check below decides)
            cells[best] = best_p;
            g.nt[best] = (int)(best_p / T[best]);
            g.mask[best] = (uint32_t)best_p - 1u;
        }
    }
    const double nc = (double)cells[0] * (double)cells[1] * (double)cells[2];
    if (nc >= 4.0e9) throw HipError(SALVA_HIP_E_CAPACITY, "dense cell table would exceed 2^32 cells; particles are too spread out");
    // The reference's hash grid costs memory per OCCUPIED cell; this table costs 4 bytes per cell of the (folded) bounding box, plus
    // 8 bytes per tile of 64 cells.  Where folding is not possible (the x axis of a decomposed run, a boundary set as wide
    // as the box, SALVA_HIP_NO_FOLD) a few stray particles far from the rest cost memory here that they do not cost there: refuse beyond a budget, with
    // a message that says what to do, rather than exhaust HBM.
    static const double budget_gib = [] {
        const char* e = getenv("SALVA_HIP_CELL_TABLE_GIB");
        const double v = e ? atof(e) : 8.0;
        return v > 0.0 ? v : 8.0;
    }();
    const double gib = (nc * 4.0 + nc / TCELLS * 8.0) / (1024.0 * 1024.0 * 1024.0);
    if (gib > budget_gib) {
        char msg[512];
        snprintf(msg, sizeof msg,
                 "the cell table over the particles' bounding box (%d x %d x %d tiles of %dx%dx%d cells) would take %.1f GiB, over the "
                 "%.1f GiB budget: particles are too spread out for the dense grid — delete strays (salva_hip_particles_intersecting_aabb "
                 "+ salva_hip_delete_particles) or raise SALVA_HIP_CELL_TABLE_GIB",
                 g.nt[0], g.nt[1], g.nt[2], TX, TY, TZ, gib, budget_gib);
        throw HipError(SALVA_HIP_E_CAPACITY, msg);
    }
}

// Sort the boundary particles by cell, build their cell table and volumes.  Runs when the boundary set changed
// (the reference redoes this every substep, contacts.rs:142-151 + dfsph_solver.rs:72-96; for unchanged boundary
// positions the result is identical).
void World::build_boundary_grid() {
    if (!b_dirty) return;
    ncontacts_bb = 0;
    if (nb == 0) { b_dirty = false; return; }
    bbox_partials.ensure(6 * std::max<size_t>(bbox_blocks(nb), 1024));
    launch_bbox(bst_pos.p, nb, sc.h, bbox_partials.p, d_rb.p->bbbox, d_flags.p, stream);
    SALVA_HIP_CHECK(hipMemcpyAsync(h_rb->bbbox, d_rb.p->bbbox, sizeof(int32_t) * 6, hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    dims_from_bbox(h_rb->bbbox, gb);
    const size_t nc = gb.ncells();
    bkeys[0].ensure(nb); bkeys[1].ensure(nb); bidx[0].ensure(nb); bidx[1].ensure(nb);
    bposv.ensure(nb); bvel.ensure(nb); bperm.ensure(nb); cell_start_b.ensure(nc + 1);
    TileGrid gv = gb.device(nullptr);
    launch_cell_keys(bst_pos.p, nb, sc.h, gv, bkeys[0].p, bidx[0].p, d_flags.p, nullptr, nullptr, nullptr, stream);
    const int end_bit = bits_for(nc);
    const size_t tb = sort_pairs_temp_bytes(nb, end_bit);
    ensure_cub_temp(tb);
    sort_pairs(cub_temp.p, tb, bkeys[0].p, bkeys[1].p, bidx[0].p, bidx[1].p, nb, end_bit, stream);
    launch_reorder_boundary(nb, bidx[1].p, bst_pos.p, bst_vel.p, bposv.p, bvel.p, bperm.p, stream);
    launch_cell_start(bkeys[1].p, nb, (uint32_t)nc, cell_start_b.p, stream);
    StepCtx c = make_ctx();
    SALVA_HIP_CHECK(hipMemsetAsync(d_counters.p + 2, 0, sizeof(unsigned long long), stream));
    launch_boundary_volumes(c, d_counters.p + 2, stream);
    SALVA_HIP_CHECK(hipMemcpyAsync(&h_rb->ncontacts_bb, d_counters.p + 2, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    ncontacts_bb = h_rb->ncontacts_bb;
    b_dirty = false;
}

// ------------------------------------------------------------------------------------------------ Becker2009Elasticity (elastic.hip)
ElasticState& World::elastic_state(uint32_t slot, uint32_t force) {
    if (slot >= fluids.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot out of range");
    FluidSlot& fs = fluids[slot];
    if (force >= fs.forces.size() || fs.forces[force].kind != SALVA_HIP_FORCE_BECKER2009)
        throw HipError(SALVA_HIP_E_INVALID, "that force entry is not a Becker2009Elasticity");
    if (fs.elastic.size() < fs.forces.size()) fs.elastic.resize(fs.forces.size());
    if (!fs.elastic[force]) fs.elastic[force] = std::make_shared<ElasticState>();
    return *fs.elastic[force];
}

bool World::has_elastic() const { return has_force(SALVA_HIP_FORCE_BECKER2009); }

bool World::elastic_stale() const {
    for (const FluidSlot& f : fluids)
        for (size_t k = 0; k < f.forces.size(); ++k)
            if (f.forces[k].kind == SALVA_HIP_FORCE_BECKER2009 && f.n) {
                const ElasticState* e = k < f.elastic.size() ? f.elastic[k].get() : nullptr;
                if (!e || e->n0 != f.n || !e->list_valid) return true;
            }
    return false;
}

// The state is read and written at its own particle count n0: the fluid's count, except between a change of that count and the
// next step, when the state still has the old length (the next step re-initialises it from there: quirk 1 needs the old volumes0).
uint64_t World::get_elasticity_state(uint32_t slot, uint32_t force, uint64_t nn, float* positions0, float* volumes0, float* rotations,
                                     float* stress, float* grad_tr) {
    use_device();
    ElasticState& e = elastic_state(slot, force);
    if (e.n0 == 0) return 0;
    if (nn == 0) return e.nnz;  // (sizing call)
    if (nn != e.n0) throw HipError(SALVA_HIP_E_INVALID, "n is not the elastic state's particle count (salva_hip_get_elasticity_contacts)");
    if (positions0) {
        std::vector<float4> t(nn);
        SALVA_HIP_CHECK(hipMemcpyAsync(t.data(), e.p0.p, nn * sizeof(float4), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
        for (uint64_t i = 0; i < nn; ++i) { positions0[3 * i] = t[i].x; positions0[3 * i + 1] = t[i].y; positions0[3 * i + 2] = t[i].z; }
    }
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
    if (positions0) {
        std::vector<float4> t(nn);
        for (uint64_t i = 0; i < nn; ++i) t[i] = make_float4(positions0[3 * i], positions0[3 * i + 1], positions0[3 * i + 2], 0.0f);
        SALVA_HIP_CHECK(hipMemcpyAsync(e.p0.p, t.data(), nn * sizeof(float4), hipMemcpyHostToDevice, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
    if (volumes0) SALVA_HIP_CHECK(hipMemcpyAsync(e.vol0.p, volumes0, nn * sizeof(float), hipMemcpyHostToDevice, stream));
    if (rotations) SALVA_HIP_CHECK(hipMemcpyAsync(e.rot.p, rotations, 9 * nn * sizeof(float), hipMemcpyHostToDevice, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    e.n0 = nn;
    e.ran = false;
    // the rest lists from positions0 now (the same lists the state had: rows are sorted); volumes0 stays as given
    elastic_build_rest(e, make_sph_consts(prm.particle_radius * prm.smoothing_factor * 2.0f), elastic_params(fluids[slot].forces[force].p),
                       true, stream);
}

// The contact lists of the last step (they describe the positions the step started from, as the reference's
// ContactManager does after `step`).  offsets: n+1 entries; entries are written only if `capacity` holds them all.
uint64_t World::get_fluid_contacts(uint32_t slot, int boundary, uint64_t* offsets, uint32_t* j_model, uint32_t* j, uint64_t capacity) {
    use_device();
    if (slot >= fluids.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot out of range");
    if (comm) throw HipError(SALVA_HIP_E_INVALID, "host-order contact export does not exist in a multi-GPU run: use salva_hip_get_local_contacts");
    if (!have_last_ctx || !sorted_valid) throw HipError(SALVA_HIP_E_INVALID, "no completed step: there are no contact lists yet");
    const uint64_t nn = fluids[slot].n, off = fluid_offset(slot);
    std::vector<uint32_t> cnt(nn, 0);
    DevBuf<uint32_t> d_cnt;
    d_cnt.ensure(std::max<size_t>(n, 1));
    if (!(boundary && nb == 0) && nn) {
        launch_unsort_u32(n, perm[cur].p, boundary ? nfb.p : nff.p, d_cnt.p, stream);
        SALVA_HIP_CHECK(hipMemcpyAsync(cnt.data(), d_cnt.p + off, nn * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
    std::vector<uint64_t> offs(nn + 1, 0);
    for (uint64_t k = 0; k < nn; ++k) offs[k + 1] = offs[k] + cnt[k];
    const uint64_t total = offs[nn];
    if (offsets) memcpy(offsets, offs.data(), (nn + 1) * sizeof(uint64_t));
    if (!j_model || !j || capacity < total || total == 0) return total;
    std::vector<uint32_t> moff(num_models(), 0), boff(std::max<size_t>(bounds.size(), 1), 0);
    for (uint32_t s = 0; s < fluids.size(); ++s) moff[s] = (uint32_t)fluid_offset(s);
    for (uint32_t s = 0; s < bounds.size(); ++s) boff[s] = (uint32_t)boundary_offset(s);
    DevBuf<uint64_t> d_offs;
    DevBuf<uint32_t> d_moff, d_boff, d_jm, d_j;
    d_offs.ensure(nn + 1); d_moff.ensure(moff.size()); d_boff.ensure(boff.size()); d_jm.ensure(total); d_j.ensure(total);
    SALVA_HIP_CHECK(hipMemcpyAsync(d_offs.p, offs.data(), (nn + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    SALVA_HIP_CHECK(hipMemcpyAsync(d_moff.p, moff.data(), moff.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    SALVA_HIP_CHECK(hipMemcpyAsync(d_boff.p, boff.data(), boff.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    flags_clean = false;
    launch_export_contacts(last_ctx, G().keys[1].p, slot, boundary, d_offs.p, d_moff.p, d_boff.p, d_jm.p, d_j.p, stream);
    SALVA_HIP_CHECK(hipMemcpyAsync(j_model, d_jm.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipMemcpyAsync(j, d_j.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    return total;
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
    scratch_f.ensure(3 * (size_t)n, stream, false, 1.1f);
    for (int k = 0; k < 2; ++k) {
        float* out = k == 0 ? positions : velocities;
        if (!out) continue;
        // inside a force callback fluid.velocities equal w = v + dv (dfsph_solver.rs:688-693), as in force_get_state
        const float4* src = k == 0 ? posm[cur].p : (in_force_cb ? last_ctx.w : vel[cur].p);
        k_unpack_xyz<<<nblk(n), BLOCK, 0, stream>>>(n, src, scratch_f.p);
        SALVA_HIP_CHECK(hipMemcpyAsync(out, scratch_f.p, 3 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
    if (densities) SALVA_HIP_CHECK(hipMemcpyAsync(densities, rho.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (volumes) {  // (they ride in vel.w, device_types.h)
        k_unpack_w<<<nblk(n), BLOCK, 0, stream>>>(n, vel[cur].p, scratch_f.p);
        SALVA_HIP_CHECK(hipMemcpyAsync(volumes, scratch_f.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, stream));
    }
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
}
uint64_t World::get_local_contacts(int boundary, uint64_t* offsets, uint32_t* j_model, uint32_t* j, uint64_t capacity) {
    use_device();
    if (!have_last_ctx || !sorted_valid) throw HipError(SALVA_HIP_E_INVALID, "no completed step: there are no contact lists yet");
    std::vector<uint32_t> cnt(n, 0);
    if (!(boundary && nb == 0) && n) {
        SALVA_HIP_CHECK(hipMemcpyAsync(cnt.data(), boundary ? nfb.p : nff.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
    std::vector<uint64_t> offs((size_t)n + 1, 0);
    for (uint64_t k = 0; k < n; ++k) offs[k + 1] = offs[k] + cnt[k];
    const uint64_t total = offs[n];
    if (offsets) memcpy(offsets, offs.data(), ((size_t)n + 1) * sizeof(uint64_t));
    if (!j_model || !j || capacity < total || total == 0) return total;
    std::vector<uint32_t> boff(std::max<size_t>(bounds.size(), 1), 0);
    for (uint32_t s = 0; s < bounds.size(); ++s) boff[s] = (uint32_t)boundary_offset(s);
    DevBuf<uint64_t> d_offs;
    DevBuf<uint32_t> d_boff, d_jm, d_j;
    d_offs.ensure((size_t)n + 1); d_boff.ensure(boff.size()); d_jm.ensure(total); d_j.ensure(total);
    SALVA_HIP_CHECK(hipMemcpyAsync(d_offs.p, offs.data(), ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    SALVA_HIP_CHECK(hipMemcpyAsync(d_boff.p, boff.data(), boff.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    flags_clean = false;
    launch_export_contacts_local(last_ctx, G().keys[1].p, boundary, d_offs.p, d_boff.p, d_jm.p, d_j.p, stream);
    SALVA_HIP_CHECK(hipMemcpyAsync(j_model, d_jm.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipMemcpyAsync(j, d_j.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    return total;
}
__global__ void k_add_acc_local(uint32_t n, const float* __restrict__ in, float4* __restrict__ acc) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    float4 a = acc[s];
    a.x += in[3 * (size_t)s]; a.y += in[3 * (size_t)s + 1]; a.z += in[3 * (size_t)s + 2];
    acc[s] = a;
}
void World::force_add_local_accelerations(const float* acc_h) {
    use_device();
    if (!in_force_cb) throw HipError(SALVA_HIP_E_INVALID, "only available inside a force callback");
    if (!acc_h) throw HipError(SALVA_HIP_E_INVALID, "null accelerations");
    if (n == 0) return;
    scratch_f.ensure(3 * (size_t)n, stream, false, 1.1f);
    SALVA_HIP_CHECK(hipMemcpyAsync(scratch_f.p, acc_h, 3 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, stream));
    // (what lands on a ghost is overwritten by the refresh of w that follows the forces, world_dist)
    k_add_acc_local<<<nblk(n), BLOCK, 0, stream>>>(n, scratch_f.p, last_ctx.acc);
    SALVA_HIP_CHECK(hipGetLastError());
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
}

void World::get_force_stats(uint32_t slot, uint32_t force, int32_t* iters, float* err) {
    if (slot >= fluids.size() || force >= fluids[slot].forces.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot / force index out of range");
    const FluidSlot& f = fluids[slot];
    if (iters) *iters = force < f.force_iters.size() ? (int32_t)f.force_iters[force] : 0;
    if (err) *err = force < f.force_errs.size() ? f.force_errs[force] : 0.0f;
}

// ------------------------------------------------------------------------------------------------ downloads
void World::get_fluid(uint32_t slot, float* pos, float* vel_out) {
    use_device();
    if (slot >= fluids.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot out of range");
    const uint64_t nn = fluids[slot].n, off = fluid_offset(slot);
    if (nn == 0) return;
    ensure_staging_current();
    scratch_f.ensure(3 * nn, stream, false, 1.1f);
    if (pos) {
        k_unpack_xyz<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, st_pos.p + off, scratch_f.p);
        SALVA_HIP_CHECK(hipMemcpyAsync(pos, scratch_f.p, 3 * nn * sizeof(float), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
    if (vel_out) {
        k_unpack_xyz<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, st_vel.p + off, scratch_f.p);
        SALVA_HIP_CHECK(hipMemcpyAsync(vel_out, scratch_f.p, 3 * nn * sizeof(float), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
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
    if (slot >= fluids.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot out of range");
    if (comm && dist_started) throw HipError(SALVA_HIP_E_INVALID, "host-order fluid arrays are not maintained in a multi-GPU run: use salva_hip_get_owned");
    wait_download();  // one download in flight
    const uint64_t nn = fluids[slot].n, off = fluid_offset(slot);
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

void World::get_fluid_field(uint32_t slot, int field, float* out) {
    use_device();
    if (slot >= fluids.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot out of range");
    if (!out) throw HipError(SALVA_HIP_E_INVALID, "null output");
    if (comm && dist_started) throw HipError(SALVA_HIP_E_INVALID, "per-fluid host-order access is not available in a multi-GPU run: use salva_hip_get_owned");
    const uint64_t nn = fluids[slot].n, off = fluid_offset(slot);
    if (nn == 0) return;
    const bool vec = field == SALVA_HIP_FIELD_VELOCITY_CHANGE || field == SALVA_HIP_FIELD_ACCELERATION;
    const size_t width = vec ? 3 : 1;
    scratch_f.ensure(std::max<size_t>(3 * nn, n), stream, false, 1.1f);
    auto finish = [&](const float* src) {
        SALVA_HIP_CHECK(hipMemcpyAsync(out, src, width * nn * sizeof(float), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    };
    switch (field) {
        case SALVA_HIP_FIELD_VELOCITY_CHANGE:
            ensure_staging_current();
            k_unpack_xyz<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, st_dv.p + off, scratch_f.p);
            finish(scratch_f.p);
            return;
        case SALVA_HIP_FIELD_PRESSURE:
            ensure_staging_current();
            k_unpack_w<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, st_dv.p + off, scratch_f.p);
            finish(scratch_f.p);
            return;
        case SALVA_HIP_FIELD_VOLUME:
            ensure_staging_current();
            k_unpack_w<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, st_pos.p + off, scratch_f.p);
            finish(scratch_f.p);
            return;
        case SALVA_HIP_FIELD_ACCELERATION:
            // accelerations are zero after every step (integrate_and_clear_accelerations) unless the host set them
            if (acc_user) {
                k_unpack_xyz<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, st_acc.p + off, scratch_f.p);
                finish(scratch_f.p);
            } else {
                memset(out, 0, 3 * nn * sizeof(float));
            }
            return;
        default: break;
    }
    // per-step solver scratch lives in sorted order: valid only right after a step
    if (!sorted_valid || !have_last_ctx)
        throw HipError(SALVA_HIP_E_INVALID, "solver scratch fields are only available right after a step");
    switch (field) {
        case SALVA_HIP_FIELD_DENSITY: launch_unsort_f32(n, perm[cur].p, rho.p, scratch_f.p, stream); break;
        case SALVA_HIP_FIELD_ALPHA: launch_unsort_f32(n, perm[cur].p, alpha.p, scratch_f.p, stream); break;
        case SALVA_HIP_FIELD_NUM_FLUID_CONTACTS: launch_unsort_u32_as_f32(n, perm[cur].p, nff.p, scratch_f.p, stream); break;
        case SALVA_HIP_FIELD_NUM_BOUNDARY_CONTACTS:
            if (nb == 0) { memset(out, 0, nn * sizeof(float)); return; }
            launch_unsort_u32_as_f32(n, perm[cur].p, nfb.p, scratch_f.p, stream);
            break;
        default: throw HipError(SALVA_HIP_E_INVALID, "unknown field");
    }
    finish(scratch_f.p + off);
}

void World::get_boundary(uint32_t slot, float* volumes, float* forces) {
    use_device();
    if (slot >= bounds.size()) throw HipError(SALVA_HIP_E_INVALID, "boundary slot out of range");
    const uint64_t nn = bounds[slot].n, off = boundary_offset(slot);
    if (nn == 0) return;
    if (volumes) {
        upload_tables();
        build_boundary_grid();
        scratch_f4.ensure(nb);
        scratch_f.ensure(nb, stream, false, 1.1f);
        launch_unsort_f4(nb, bperm.p, bposv.p, scratch_f4.p, stream);
        k_unpack_w<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, scratch_f4.p + off, scratch_f.p);
        SALVA_HIP_CHECK(hipMemcpyAsync(volumes, scratch_f.p, nn * sizeof(float), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
    if (forces) {
        scratch_f.ensure(3 * nn, stream, false, 1.1f);
        k_unpack_xyz<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, bforce.p + off, scratch_f.p);
        SALVA_HIP_CHECK(hipMemcpyAsync(forces, scratch_f.p, 3 * nn * sizeof(float), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
}

// ------------------------------------------------------------------------------------------------ host force callbacks
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
    if (slot >= fluids.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot out of range");
    const uint64_t nn = fluids[slot].n, off = fluid_offset(slot);
    if (nn == 0) return;
    scratch_f4.ensure(n);
    scratch_f.ensure(std::max<size_t>(3 * nn, n), stream, false, 1.1f);
    for (int k = 0; k < 2; ++k) {
        float* out = k == 0 ? positions : velocities;
        if (!out) continue;
        // fluid.velocities equal w = v + dv while the forces run (dfsph_solver.rs:688-693)
        launch_unsort_f4(n, perm[cur].p, k == 0 ? last_ctx.posm : last_ctx.w, scratch_f4.p, stream);
        k_unpack_xyz<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, scratch_f4.p + off, scratch_f.p);
        SALVA_HIP_CHECK(hipMemcpyAsync(out, scratch_f.p, 3 * nn * sizeof(float), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
    if (densities) {
        launch_unsort_f32(n, perm[cur].p, last_ctx.rho, scratch_f.p, stream);
        SALVA_HIP_CHECK(hipMemcpyAsync(densities, scratch_f.p + off, nn * sizeof(float), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
}

void World::force_add_accelerations(uint32_t slot, const float* acc_h) {
    use_device();
    if (!in_force_cb) throw HipError(SALVA_HIP_E_INVALID, "only available inside a force callback");
    if (slot >= fluids.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot out of range");
    if (!acc_h) throw HipError(SALVA_HIP_E_INVALID, "null accelerations");
    const uint64_t nn = fluids[slot].n, off = fluid_offset(slot);
    if (nn == 0) return;
    scratch_f.ensure(3 * nn, stream, false, 1.1f);
    SALVA_HIP_CHECK(hipMemcpyAsync(scratch_f.p, acc_h, 3 * nn * sizeof(float), hipMemcpyHostToDevice, stream));
    k_add_acc_from_host<<<nblk(n), BLOCK, 0, stream>>>(n, perm[cur].p, (uint32_t)off, (uint32_t)nn, scratch_f.p, last_ctx.acc);
    SALVA_HIP_CHECK(hipGetLastError());
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
}

// checkpoint restore: the two pieces of solver state that live next to the fluid arrays (velocity_changes, IISPH pressures)
void World::set_fluid_field(uint32_t slot, int field, const float* data) {
    use_device();
    if (slot >= fluids.size()) throw HipError(SALVA_HIP_E_INVALID, "fluid slot out of range");
    if (!data) throw HipError(SALVA_HIP_E_INVALID, "null data");
    if (field != SALVA_HIP_FIELD_VELOCITY_CHANGE && field != SALVA_HIP_FIELD_PRESSURE)
        throw HipError(SALVA_HIP_E_INVALID, "only velocity_changes and pressures can be set");
    const uint64_t nn = fluids[slot].n, off = fluid_offset(slot);
    if (nn == 0) return;
    ensure_staging_current();
    const size_t width = field == SALVA_HIP_FIELD_VELOCITY_CHANGE ? 3 : 1;
    scratch_f.ensure(width * nn, stream, false, 1.1f);
    SALVA_HIP_CHECK(hipMemcpyAsync(scratch_f.p, data, width * nn * sizeof(float), hipMemcpyHostToDevice, stream));
    if (field == SALVA_HIP_FIELD_VELOCITY_CHANGE) k_pack_xyz<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, scratch_f.p, st_dv.p + off, 1, 0.0f);
    else k_pack_w<<<nblk(nn), BLOCK, 0, stream>>>((uint32_t)nn, scratch_f.p, st_dv.p + off);
    SALVA_HIP_CHECK(hipGetLastError());
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    sorted_valid = false; bbox_known = false; have_last_ctx = false;
}

uint64_t World::device_bytes() const {
    uint64_t b = 0;
    auto add = [&](size_t x) { b += x; };
    add(st_pos.bytes()); add(st_vel.bytes()); add(st_dv.bytes()); add(st_acc.bytes()); add(st_model.bytes());
    for (int k = 0; k < 2; ++k) {
        add(posm[k].bytes()); add(vel[k].bytes()); add(dv[k].bytes()); add(model[k].bytes()); add(perm[k].bytes());
        for (const GridTabs& t : gtab) { add(t.keys[k].bytes()); add(t.idx[k].bytes()); }
        add(bkeys[k].bytes()); add(bidx[k].bytes());
    }
    add(acc.bytes()); add(w.bytes()); add(normal.bytes()); add(dii.bytes()); add(dijpj.bytes()); add(iisph_q.bytes()); add(iisph_pr.bytes()); add(posmr.bytes()); add(w2.bytes());
    add(rho.bytes()); add(alpha.bytes()); add(kappa.bytes()); add(kappa2.bytes()); add(rho_star.bytes()); add(aii.bytes());
    add(visc_beta.bytes()); add(visc_target.bytes()); add(visc_u0.bytes()); add(visc_u1.bytes()); add(visc_va.bytes()); add(he_colors.bytes()); add(he_gradcs.bytes());
    add(nff.bytes()); add(nfb.bytes()); add(gtab[0].cell_start_f.bytes()); add(gtab[1].cell_start_f.bytes()); add(halo_src.bytes()); add(bhalo_src.bytes());
    add(nbr_ff.bytes()); add(nbr_fb.bytes()); add(slice_near.bytes()); add(cub_temp.bytes()); add(scratch_f.bytes());
    add(scratch_f4.bytes()); add(bst_pos.bytes()); add(bst_vel.bytes()); add(bposv.bytes()); add(bvel.bytes());
    add(bforce.bytes()); add(bperm.bytes()); add(cell_start_b.bytes()); add(partials.bytes());
    return b;
}

// Average duration (microseconds) of one k_pred_density launch on the last step's lists, by HIP events on the
// world's own stream.  The kernel only rewrites scratch (kappa, partials), so the world's state is unaffected.
float World::time_pred_density(int reps) {
    use_device();
    if (!have_last_ctx || !sorted_valid || n == 0) throw HipError(SALVA_HIP_E_INVALID, "no completed step to time");
    if (reps < 1) reps = 1;
#ifdef SALVA_HIP_DIAG
    if (sw.tile_timing) tile_timing_report();
#endif
    flags_clean = false;  // (a between-step launch may raise an error flag: the next step clears them itself — ADVICE r04)
    launch_pred_density(last_ctx, lds, last_dt, stream);  // warm-up
    SALVA_HIP_CHECK(hipEventRecord(ev[0], stream));
    for (int r = 0; r < reps; ++r) launch_pred_density(last_ctx, lds, last_dt, stream);
    SALVA_HIP_CHECK(hipEventRecord(ev[1], stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    float ms = 0.0f;
    SALVA_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    return ms * 1000.0f / (float)reps;
}


// Average duration (microseconds) of one launch of a neighbour-sum kernel on the last step's lists (HIP events on the world's
// stream): 0 k_pred_density, 1 k_divergence, 2 k_iisph_next_pressure, 3 k_iisph_dij_pj.  Scratch outputs only.
void World::tile_tables(uint32_t slot, uint32_t* info, uint32_t* halo_row, uint32_t cap_row, uint32_t* counts, uint32_t cap_counts, uint32_t* entries,
                        uint32_t cap_entries) {
    use_device();
    if (!have_last_ctx || !sorted_valid || n == 0) throw HipError(SALVA_HIP_E_INVALID, "no completed step to look at");
    const StepCtx& c = last_ctx;
    if (slot >= c.nlaunch) throw HipError(SALVA_HIP_E_INVALID, "no such tile slot");
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    TileAcc a[2];
    uint4 desc;
    SALVA_HIP_CHECK(hipMemcpy(a, c.tile_off + slot, sizeof(a), hipMemcpyDeviceToHost));
    SALVA_HIP_CHECK(hipMemcpy(&desc, c.slot_desc + slot, sizeof(desc), hipMemcpyDeviceToHost));
    const uint32_t S = (uint32_t)(a[1].s - a[0].s), SB = (uint32_t)(a[1].sb - a[0].sb), own_n = desc.z - desc.y;
    const uint64_t hoff = c.halo_stride ? (uint64_t)slot * c.halo_stride : a[0].s;
    memset(info, 0, 16 * sizeof(uint32_t));
    info[0] = c.nlaunch; info[1] = desc.y; info[2] = desc.z; info[3] = S; info[4] = SB;
    info[5] = lds.max_halo_fluid; info[6] = lds.raw_slots(); info[7] = lds.sum_slots(); info[8] = lds_full.max_halo_fluid;
    info[9] = ref_last ? 1u : 0u; info[10] = (uint32_t)tally.ref_passes; info[11] = (uint32_t)tally.ref_misses;
    if (halo_row && cap_row && S)
        SALVA_HIP_CHECK(hipMemcpy(halo_row, c.halo_src + hoff, (size_t)std::min(S, cap_row) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (!own_n) return;
    std::vector<uint32_t> cnt(own_n);
    SALVA_HIP_CHECK(hipMemcpy(cnt.data(), c.nff + desc.y, (size_t)own_n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (counts) memcpy(counts, cnt.data(), (size_t)std::min(own_n, cap_counts) * sizeof(uint32_t));
    if (!entries || !cap_entries) return;
    const uint32_t nsl = (own_n + WAVE - 1) / WAVE;
    std::vector<uint32_t> blk((size_t)nsl * c.cap_ff * WAVE);
    SALVA_HIP_CHECK(hipMemcpy(blk.data(), c.nbr_ff + (size_t)a[0].nsl * c.cap_ff * WAVE, blk.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint32_t o = 0;
    for (uint32_t k = 0; k < own_n; ++k) {
        const uint32_t* p = blk.data() + (size_t)(k / WAVE) * c.cap_ff * WAVE + 4u * (k % WAVE);
        for (uint32_t e = 0; e < cnt[k] && o < cap_entries; ++e) {
            const uint32_t d = p[ellq(e >> 1)];
            entries[o++] = (e & 1u) ? (d >> 16) : (d & 0xffffu);
        }
    }
    info[12] = o;
}

float World::time_kernel(int kernel, int reps) {
    use_device();
    if (!have_last_ctx || !sorted_valid || n == 0) throw HipError(SALVA_HIP_E_INVALID, "no completed step to time");
    if (kernel == 0) return time_pred_density(reps);
    if (reps < 1) reps = 1;
    const bool iisph = prm.solver == SALVA_HIP_SOLVER_IISPH;
    if (kernel == 4 && comm) throw HipError(SALVA_HIP_E_INVALID, "not available in a multi-GPU run");
    if ((kernel == 2 || kernel == 3) && !iisph) throw HipError(SALVA_HIP_E_INVALID, "an IISPH kernel needs an IISPH world");
    if (kernel == 1 && iisph) throw HipError(SALVA_HIP_E_INVALID, "k_divergence needs a DFSPH world");
    StepCtx cd = last_ctx;
    cd.ctl = nullptr;
    flags_clean = false;  // (see time_pred_density)
    if (kernel == 6) {  // the apply pass updates w in place: let it run on a copy (w2 is free outside a speculative solve)
        if (iisph) throw HipError(SALVA_HIP_E_INVALID, "k_divergence_apply needs a DFSPH world");
        w2.ensure(n, stream, false, 1.1f);
        SALVA_HIP_CHECK(hipMemcpyAsync(w2.p, w.p, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice, stream));
        cd.w = w2.p; cd.w2 = w2.p; cd.spec_k = -1; cd.bforce = nullptr;
    }
    ElasticState* el = nullptr;
    uint32_t el_slot = 0, el_force = 0;
    DevBuf<float4> acc_copy;
    DevBuf<float> el_sig, el_F;
    bool el_swapped = false;
    struct Unswap {  // (also when a launch throws)
        ElasticState*& e; DevBuf<float>& s; DevBuf<float>& f; bool& on;
        ~Unswap() { if (on) { std::swap(e->sig.p, s.p); std::swap(e->sig.cap, s.cap); std::swap(e->F.p, f.p); std::swap(e->F.cap, f.cap); } }
    } unswap{el, el_sig, el_F, el_swapped};
    if (kernel == 7 || kernel == 8) {  // the first Becker2009Elasticity entry, on the last step's state
        for (uint32_t f = 0; f < fluids.size() && !el; ++f)
            for (uint32_t k = 0; k < fluids[f].forces.size() && !el; ++k)
                if (fluids[f].forces[k].kind == SALVA_HIP_FORCE_BECKER2009 && k < fluids[f].elastic.size() && fluids[f].elastic[k] &&
                    fluids[f].elastic[k]->list_valid && fluids[f].elastic[k]->n0 == fluids[f].n) {
                    el = fluids[f].elastic[k].get(); el_slot = f; el_force = k;
                }
        if (!el) throw HipError(SALVA_HIP_E_INVALID, "no Becker2009Elasticity entry has run");
        if (comm) throw HipError(SALVA_HIP_E_INVALID, "not available in a multi-GPU run");
        cd.gate = nullptr;
        acc_copy.ensure(n);
        SALVA_HIP_CHECK(hipMemcpyAsync(acc_copy.p, cd.acc, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice, stream));
        // the force pass reads the rotations of the step, which its completion moved into `rot`
        SALVA_HIP_CHECK(hipMemcpyAsync(el->rot_new.p, el->rot.p, 9 * el->n0 * sizeof(float), hipMemcpyDeviceToDevice, stream));
        if (kernel == 7) {  // the pass rewrites sigma and F: it runs on copies, and the state keeps what the step computed
            el_sig.ensure(6 * el->n0); el_F.ensure(9 * el->n0);
            std::swap(el->sig.p, el_sig.p); std::swap(el->sig.cap, el_sig.cap);
            std::swap(el->F.p, el_F.p); std::swap(el->F.cap, el_F.cap);
            el_swapped = true;
        }
    }
    const ElasticParams el_p = el ? elastic_params(fluids[el_slot].forces[el_force].p) : ElasticParams{};
    const uint32_t el_off = el ? (uint32_t)fluid_offset(el_slot) : 0u;
    auto launch = [&]() {
        switch (kernel) {
            case 7: launch_elastic_rot_stress(cd, *el, el_p, stream); break;  // (reads rot; writes rot_new and the copies of sigma, F)
            case 8: launch_elastic_forces(cd, el_off, *el, el_p, acc_copy.p, stream); break;
            case 1: launch_divergence(cd, lds, stream); break;
            case 6: launch_divergence_apply(cd, lds, inv_dt_prev, stream); break;
            case 2: launch_iisph_next_pressure(cd, lds, last_dt, 0.5f, kappa.p, kappa2.p, stream); break;
            case 3: launch_iisph_dij_pj(cd, lds, last_dt, kappa.p, stream); break;
            case 4:  // rebuilds the lists on the tables of the last step.  The positions have moved since those were built, so every
                     // particle's cell is taken from its sorted key (as after a DynamicContactSampling push-out): without that a
                     // particle that left its cell indexes the tile's cell table out of range and the kernel never returns.
                cd.stale_keys = G().keys[1].p;
                if (ref_last) {
                    // (the step compacted its slot tables in place: every build starts from the full box's tables again, so the
                    // figure holds the tile scan and k_tile_halo_fill as well)
                    StepCtx cf = cd;
                    cf.slot_order = nullptr; cf.ntiny = cf.nlight = 0u; cf.slot_base = 0u;
                    const size_t tb = scan_tiles_temp_bytes(ref_last_nslots_bound + 1);
                    ensure_cub_temp(tb);
                    scan_tiles(cub_temp.p, tb, G().tile_cnt.p, G().tile_off.p, ref_last_nslots_bound + 1, stream);
                    launch_tile_halo_fill(cf, halo_src.p, bhalo_src.p, slot_info.p, stream);
                    const RefBuild rb{halo_src.p, slot_info.p, G().tile_off.p, ref_last_caps, d_rb.p->max_ref};
                    launch_nbr_build(cd, lds_full, tile_list_stats.p, reinterpret_cast<unsigned long long*>(&d_rb.p->ncontacts_ff), &d_rb.p->max_cnt_ff, nullptr, stream, &rb);
                    break;
                }
                launch_nbr_build(cd, lds, tile_list_stats.p, reinterpret_cast<unsigned long long*>(&d_rb.p->ncontacts_ff), &d_rb.p->max_cnt_ff, nullptr, stream);
                break;
#ifdef SALVA_HIP_DIAG
            case 5: launch_list_schedule(cd, lds, stream); break;  // re-schedules the (already scheduled or not) lists: same work
#endif
            default: throw HipError(SALVA_HIP_E_INVALID, "unknown kernel id");
        }
    };
    launch();  // warm-up
    SALVA_HIP_CHECK(hipEventRecord(ev[0], stream));
    for (int r = 0; r < reps; ++r) launch();
    SALVA_HIP_CHECK(hipEventRecord(ev[1], stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    float ms = 0.0f;
    SALVA_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    return ms * 1000.0f / (float)reps;
}

}  // namespace salva

// world_coupling.hip — rigid-body coupling of libsalva_hip (integrations/rapier/fluids_pipeline.rs): the sampling methods of a
// boundary and their registration, poses in and wrenches out, and DynamicContactSampling inside the step (kernels: dcs.hip).
#include "world.h"
#include "dcs.h"
#include "pose.h"

#include <algorithm>
#include <cmath>

namespace salva {

// ------------------------------------------------------------------------------------------------ rigid-body coupling
// integrations/rapier/fluids_pipeline.rs, StaticSampling arm.  q * v of nalgebra's UnitQuaternion (geometry/
// quaternion_ops.rs): t = 2 q.vec x v; v' = v + w t + q.vec x t.
__device__ __forceinline__ void boundary_pose_row(const float4 pt, const SalvaHipRigidPose& p, float4& pos_io, float4& vel_io) {
    float4 o = pos_io;  // .w (volume slot) untouched
    pose_point(p.rotation[0], p.rotation[1], p.rotation[2], p.rotation[3], p.translation[0], p.translation[1], p.translation[2], pt.x, pt.y,
               pt.z, o.x, o.y, o.z);  // (pose.h: shared with the shape sampler's emit kernel)
    pos_io = o;
    float4 v = vel_io;  // .w carries the boundary's model id
    if (p.has_body) {
        // body.velocity_at_point(pt) with the local point, as the reference writes it (:183)
        const float dx = pt.x - p.world_com[0], dy = pt.y - p.world_com[1], dz = pt.z - p.world_com[2];
        v.x = p.linvel[0] + (opaque(p.angvel[1] * dz) - opaque(p.angvel[2] * dy));
        v.y = p.linvel[1] + (opaque(p.angvel[2] * dx) - opaque(p.angvel[0] * dz));
        v.z = p.linvel[2] + (opaque(p.angvel[0] * dy) - opaque(p.angvel[1] * dx));
    } else {
        v.x = v.y = v.z = 0.0f;
    }
    vel_io = v;
}
__global__ void k_boundary_pose(uint32_t n, const float4* __restrict__ local, SalvaHipRigidPose p, float4* __restrict__ pos,
                                float4* __restrict__ vel) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    boundary_pose_row(local[i], p, pos[i], vel[i]);
}
// salva_hip_update_boundary_poses: the statically sampled boundaries of one call as one launch over their concatenated rows
// (`first`: the entry's first row in that concatenation, ascending); the force rows are cleared on the way (clear_forces(true) :262)
struct PoseEntry { SalvaHipRigidPose pose; const float4* local; uint32_t first, n, off, pad; };
__global__ void k_boundary_poses(uint32_t total, uint32_t nent, const PoseEntry* __restrict__ ent, float4* __restrict__ pos,
                                 float4* __restrict__ vel, float4* __restrict__ force) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    uint32_t lo = 0, hi = nent;  // the last entry with first <= i
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) / 2u; if (ent[mid].first <= i) lo = mid; else hi = mid; }
    const PoseEntry& e = ent[lo];
    const uint32_t j = i - e.first, row = e.off + j;
    boundary_pose_row(e.local[j], e.pose, pos[row], vel[row]);
    force[row] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// per-block partial sums of f and (x - c) x f in f64 (6 doubles per block)
// block `lb` of `nblocks` over one boundary's rows (grid stride): the one copy of k_boundary_wrench / k_boundary_wrenches
__device__ __forceinline__ void boundary_wrench_block(uint32_t n, const float4* __restrict__ pos, const float4* __restrict__ force, float cx,
                                                      float cy, float cz, uint32_t lb, uint32_t nblocks, double* __restrict__ partial) {
    double a[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t i = lb * blockDim.x + threadIdx.x; i < n; i += nblocks * blockDim.x) {
        const float4 p = pos[i], f = force[i];
        const float rx = p.x - cx, ry = p.y - cy, rz = p.z - cz;
        a[0] += f.x; a[1] += f.y; a[2] += f.z;
        a[3] += (double)(ry * f.z - rz * f.y); a[4] += (double)(rz * f.x - rx * f.z); a[5] += (double)(rx * f.y - ry * f.x);
    }
    __shared__ double sh[BLOCK / WAVE][6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double v = a[k];
        for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, WAVE);
        if ((threadIdx.x & (WAVE - 1)) == 0) sh[threadIdx.x / WAVE][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double v = 0;
        for (uint32_t w = 0; w < blockDim.x / WAVE; ++w) v += sh[w][threadIdx.x];
        partial[threadIdx.x] = v;
    }
}
__global__ void k_boundary_wrench(uint32_t n, const float4* __restrict__ pos, const float4* __restrict__ force, float cx, float cy,
                                  float cz, double* __restrict__ partial) {
    boundary_wrench_block(n, pos, force, cx, cy, cz, blockIdx.x, gridDim.x, partial + (size_t)blockIdx.x * 6);
}
// salva_hip_get_boundary_wrenches: every listed boundary keeps the partition of k_boundary_wrench — its own min(nblk(n), 256) blocks,
// `block0` the first of them in this launch (ascending) — so that its partial sums are the single call's, bit for bit
struct WrenchEntry { uint32_t off, n, block0, nblocks; float c[3]; uint32_t pad; };
__global__ void k_boundary_wrenches(uint32_t nent, const WrenchEntry* __restrict__ ent, const float4* __restrict__ pos,
                                    const float4* __restrict__ force, double* __restrict__ partial) {
    uint32_t lo = 0, hi = nent;  // the last entry with block0 <= blockIdx.x
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) / 2u; if (ent[mid].block0 <= blockIdx.x) lo = mid; else hi = mid; }
    const WrenchEntry e = ent[lo];
    boundary_wrench_block(e.n, pos + e.off, force + e.off, e.c[0], e.c[1], e.c[2], blockIdx.x - e.block0, e.nblocks, partial + (size_t)blockIdx.x * 6);
}

void World::set_boundary_sampling(uint32_t slot, uint64_t nn, const float* local_points, uint32_t memberships, uint32_t filter,
                                  const std::function<void(float4*)>* fill_dev) {
    const bool keep_forces = slot < bounds.size() ? bounds[slot].wants_forces : false;
    set_boundary_from(slot, nn, local_points, nullptr, memberships, filter, keep_forces, fill_dev);
    auto buf = std::make_shared<DevBuf<float4>>();
    buf->ensure(nn ? nn : 1);
    if (nn) {
        SALVA_HIP_CHECK(hipMemcpyAsync(buf->p, bst_pos.p + boundary_offset(slot), nn * sizeof(float4), hipMemcpyDeviceToDevice, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
    bounds[slot].sampling = buf;
}

// What salva_hip_update_boundary_pose(s) checks before anything changes ...
void World::check_pose_target(uint32_t slot, const SalvaHipRigidPose& pose) const {
    if (slot >= bounds.size()) throw HipError(SALVA_HIP_E_INVALID, "boundary slot out of range");
    const BoundarySlot& b = bounds[slot];
    if (!b.sampling && !b.dyn)
        throw HipError(SALVA_HIP_E_INVALID, "boundary has no sampling method (salva_hip_set_boundary_sampling / _dynamic_sampling)");
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(pose.rotation[k])) throw HipError(SALVA_HIP_E_INVALID, "non-finite pose");
}
// ... and what accepting the pose does to the slot.  A dynamically sampled boundary stores it: the projection itself runs inside the
// step, where the reference runs it.  true: a statically sampled boundary, whose rows the caller writes now.
bool World::accept_pose(BoundarySlot& b, const SalvaHipRigidPose& pose) {
    if (pose.has_body) {
        const bool wants = pose.is_dynamic != 0;
        if (wants != b.wants_forces) { b.wants_forces = wants; tables_dirty = true; }
    }
    if (b.dyn) { b.dyn->pose = pose; return false; }
    b_dirty = true; have_last_ctx = false;
    return true;
}

void World::update_boundary_pose(uint32_t slot, const SalvaHipRigidPose& pose) {
    use_device();
    check_pose_target(slot, pose);
    BoundarySlot& b = bounds[slot];
    if (!accept_pose(b, pose) || !b.n) return;
    const uint64_t off = boundary_offset(slot);
    k_boundary_pose<<<nblk(b.n), BLOCK, 0, stream>>>((uint32_t)b.n, b.sampling->p, pose, bst_pos.p + off, bst_vel.p + off);
    SALVA_HIP_CHECK(hipGetLastError());
    SALVA_HIP_CHECK(hipMemsetAsync(bforce.p + off, 0, b.n * sizeof(float4), stream));  // boundary.clear_forces(true) :262
}

// `count` calls of update_boundary_pose in order, validated as a whole before anything changes: the dynamically sampled slots store
// their pose, the statically sampled ones share one launch (a slot listed twice: its last pose is the one that stays, as in order)
void World::update_boundary_poses(uint32_t count, const uint32_t* slots, const SalvaHipRigidPose* poses) {
    use_device();
    for (uint32_t k = 0; k < count; ++k) check_pose_target(slots[k], poses[k]);
    std::vector<uint32_t> launch;  // the entries that write rows
    for (uint32_t k = 0; k < count; ++k) {
        BoundarySlot& b = bounds[slots[k]];
        if (!accept_pose(b, poses[k]) || !b.n) continue;
        bool last = true;
        for (uint32_t j = k + 1; j < count; ++j) if (slots[j] == slots[k]) last = false;
        if (last) launch.push_back(k);
    }
    if (launch.empty()) return;
    PoseEntry* ent_h = reinterpret_cast<PoseEntry*>(cpl.pose_stage.acquire(launch.size() * sizeof(PoseEntry)));
    uint64_t total = 0;
    for (size_t e = 0; e < launch.size(); ++e) {
        const uint32_t k = launch[e];
        const BoundarySlot& b = bounds[slots[k]];
        ent_h[e] = PoseEntry{poses[k], b.sampling->p, (uint32_t)total, (uint32_t)b.n, (uint32_t)boundary_offset(slots[k]), 0u};
        total += b.n;
    }
    if (total >= 0xfffffff0ull) throw HipError(SALVA_HIP_E_CAPACITY, "too many boundary particles");
    cpl.pose_tab.ensure(launch.size() * sizeof(PoseEntry), stream, false, 1.5f);
    SALVA_HIP_CHECK(hipMemcpyAsync(cpl.pose_tab.p, ent_h, launch.size() * sizeof(PoseEntry), hipMemcpyHostToDevice, stream));
    k_boundary_poses<<<nblk(total), BLOCK, 0, stream>>>((uint32_t)total, (uint32_t)launch.size(), reinterpret_cast<const PoseEntry*>(cpl.pose_tab.p),
                                                        bst_pos.p, bst_vel.p, bforce.p);
    SALVA_HIP_CHECK(hipGetLastError());
    cpl.pose_stage.release(stream);
}

// ------------------------------------------------------------------------------------------------ DynamicContactSampling
// ColliderCouplingSet::register_coupling(boundary, collider, ColliderSampling::DynamicContactSampling) (fluids_pipeline.rs:42-43,
// 96-114): the boundary starts empty; every step re-emits its particles from the fluid near the collider.  The one registration
// behind the two setters below: the slot keeps whether it wants forces and carries the description from now on (identity pose, no
// rows emitted yet).
void World::register_dynamic_sampling(uint32_t slot, std::shared_ptr<DynSampling> d, uint32_t memberships, uint32_t filter) {
    const bool keep_forces = slot < bounds.size() ? bounds[slot].wants_forces : false;
    set_boundary(slot, 0, nullptr, nullptr, memberships, filter, keep_forces);
    bounds[slot].sampling.reset();
    bounds[slot].dyn = std::move(d);
}

// A collider that is a built-in shape, or a triangle mesh or a height field of this world (mesh.hip) or a compound (compound.hip):
// gather, projection and apply all stay on the device, and the pose handed to salva_hip_update_boundary_pose places the collider.
void World::set_boundary_dynamic_sampling(uint32_t slot, const GeomArg& geom, uint32_t memberships, uint32_t filter) {
    if (geom.shape) check_shape_params(*geom.shape, "shape parameters must be positive");
    refuse_handle_when_decomposed(geom);
    auto d = std::make_shared<DynSampling>();
    d->geom = geom_of(geom);
    register_dynamic_sampling(slot, std::move(d), memberships, filter);
}

void World::set_boundary_dynamic_sampling_host(uint32_t slot, const SalvaHipHostShape& shape, uint32_t memberships, uint32_t filter) {
    if (!shape.aabb || !shape.project) throw HipError(SALVA_HIP_E_INVALID, "a host shape needs both callbacks");
    auto d = std::make_shared<DynSampling>();
    d->geom.kind = SALVA_HIP_SHAPE_HOST;
    d->host = shape;
    register_dynamic_sampling(slot, std::move(d), memberships, filter);
}

// unregister_coupling (fluids_pipeline.rs:116-125): the boundary stays, with the particles it holds now, as a plain boundary;
// nothing of the sampling method — in particular no host callback or user pointer — is kept
void World::clear_boundary_sampling(uint32_t slot) {
    if (slot >= bounds.size()) throw HipError(SALVA_HIP_E_INVALID, "boundary slot out of range");
    BoundarySlot& b = bounds[slot];
    b.sampling.reset();
    b.dyn.reset();
    // the particles keep the velocities k_boundary_pose / k_dcs_emit wrote for the moving collider (the reference keeps them after
    // unregister_coupling too): from now on make_ctx must not take the upload's "at rest" for them
    if (b.n) b.vel_zero = false;
}

// The two places that know what each kind of collider needs (world.h DynSampling).
DcsParams DynSampling::params(float h, float particle_radius, float dt) const {
    if (geom.kind == SALVA_HIP_SHAPE_HOST) {
        float mins[3], maxs[3];
        host.aabb(host.user, mins, maxs);
        for (int a = 0; a < 3; ++a)
            if (!(mins[a] <= maxs[a])) throw HipError(SALVA_HIP_E_INVALID, "host shape: the aabb callback returned an empty or NaN box");
        return dcs_params_host(mins, maxs, h, particle_radius, dt);
    }
    if (geom.compound) return dcs_params_compound(*geom.compound, pose, h, particle_radius, dt);
    if (geom.mesh) return dcs_params_mesh(geom.mins(), geom.maxs(), pose, h, particle_radius, dt);
    return dcs_params(geom.shape, pose, h, particle_radius, dt);
}
void DynSampling::fill_entry(DcsbEntry& e) const {
    if (geom.mesh) {
        e.mesh = geom.mesh->dev();
    } else if (geom.compound) {
        e.parts = geom.parts();
        e.nparts = geom.nparts();
    }
    e.pose = pose;
}

// parameters of a built-in collider shape (include/salva_hip.h); throws for any other kind
int shape_param_count(int kind) {
    switch (kind) {
        case SALVA_HIP_SHAPE_BALL: return 1;
        case SALVA_HIP_SHAPE_CUBOID: return 3;
        case SALVA_HIP_SHAPE_CAPSULE: case SALVA_HIP_SHAPE_CYLINDER: return 2;
        default: throw HipError(SALVA_HIP_E_INVALID, "unknown shape kind (ball, cuboid, capsule (y) and cylinder (y) are built in; other parry shapes belong to the host)");
    }
}

void check_shape_params(const SalvaHipShape& shape, const char* message) {
    const int np = shape_param_count(shape.kind);
    for (int a = 0; a < np; ++a)
        if (!(shape.params[a] > 0.0f) || !std::isfinite(shape.params[a])) throw HipError(SALVA_HIP_E_INVALID, message);
}

bool World::has_dynamic_sampling() const {
    for (const BoundarySlot& b : bounds) if (b.dyn) return true;
    return false;
}

uint64_t World::boundary_len(uint32_t slot) const {
    if (slot >= bounds.size()) throw HipError(SALVA_HIP_E_INVALID, "boundary slot out of range");
    return bounds[slot].n;
}

// The DynamicContactSampling arm of ColliderCouplingManager::update_boundaries (fluids_pipeline.rs:193-259, :262) for every
// boundary registered with it, in slot order, at the reference's point of the substep: the fluid cell keys exist (grid
// insertion, liquid_world.rs:90-91), the boundaries are not in the grid yet (:106).  Works on the sorted working set of the
// previous step (posm[cur] / vel[cur], G().keys[0] = this step's keys in that order).
void World::run_dynamic_sampling() {
    const TileGrid gv = gf.device(nullptr);
    // Maximal runs of consecutive dynamically sampled slots whose shape is on the device go through ONE pass over the fluid
    // (run_dynamic_sampling_batch).  Slots that are not dynamically sampled do not break a run; a host shape does, and
    // runs at its place in slot order, so that the pushes keep their order.  A run of one, an empty fluid and every decomposed world
    // (whose emitted rows go through a collective per collider) take the per-collider path.
    std::vector<uint32_t> run;
    for (uint32_t slot = 0; slot < bounds.size();) {
        if (!bounds[slot].dyn) { ++slot; continue; }
        run.clear();
        if (!comm && !sw.dcs_batch_off && n)
            for (uint32_t s = slot; s < bounds.size() && !(bounds[s].dyn && bounds[s].dyn->geom.kind == SALVA_HIP_SHAPE_HOST); ++s)
                if (bounds[s].dyn) run.push_back(s);
        if (run.size() >= DCS_BATCH_MIN_RUN) {
            run_dynamic_sampling_batch(run, gv);
            slot = run.back() + 1;
        } else {
            run_dynamic_sampling_slot(slot, gv);
            ++slot;
        }
    }
}

// compact `count` rows by cpl.dcs_flag, read how many stayed, wait for it (`tb`: select_flagged_temp_bytes, held by cub_temp)
uint32_t World::compact_and_count(size_t tb, const float4* in, float4* out, uint32_t count) {
    select_flagged_f4(cub_temp.p, tb, in, cpl.dcs_flag.p, out, cpl.dcs_num.p, count, stream);
    SALVA_HIP_CHECK(hipMemcpyAsync(&h_rb->dcs_count, cpl.dcs_num.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    wait_stream(); ++dcs_stats[1];
    return h_rb->dcs_count;
}

void World::run_dynamic_sampling_slot(uint32_t slot, const TileGrid& gv) {
    BoundarySlot& b = bounds[slot];
    DynSampling& d = *b.dyn;
    uint32_t cnt = 0;
    const float4* emit_src = nullptr;  // the compacted (projection, source particle) rows
    // (decomposed run: a failure of the rank-local part must not leave the other ranks waiting in the collective below —
    // it is parked and travels with the counts, dist_gather_emitted)
    HipError local_error(SALVA_HIP_E_INVALID, "");
    bool local_failed = false;
    try {
        if (n) {
            // A built-in shape projects inside the pass over the fluid.  The host's shape: box tests on the device, the projections
            // on the host, the rest of the loop body on the device; a mesh or a compound: the same passes with the projections on the
            // device as well (k_dcs_project_mesh, k_dcs_compound_project).
            const DcsParams prm_d = d.params(sc.h, prm.particle_radius, dt_prev);
            cpl.dcs_cand.ensure(n, stream, false, 1.1f); cpl.dcs_out.ensure(n, stream, false, 1.1f); cpl.dcs_flag.ensure(n, stream, false, 1.1f);
            cpl.dcs_num.ensure(1);
            if (d.built_in())
                launch_dcs_project(n, posm[cur].p, vel[cur].p, G().keys[0].p, perm[cur].p, comm ? gtag[cur].p : nullptr, gv, prm_d, cpl.dcs_cand.p,
                                   cpl.dcs_flag.p, stream);
            else
                launch_dcs_gather(n, posm[cur].p, vel[cur].p, G().keys[0].p, gv, prm_d, cpl.dcs_cand.p, cpl.dcs_flag.p, stream);
            ++dcs_stats[0];
            const size_t tb = select_flagged_temp_bytes(n);
            ensure_cub_temp(tb);
            const uint32_t ng = compact_and_count(tb, cpl.dcs_cand.p, cpl.dcs_out.p, n);
            if (d.built_in()) {
                cnt = ng;
                emit_src = cpl.dcs_out.p;
            } else if (ng) {
                cpl.dcs_proj.ensure(ng, stream, false, 1.5f); cpl.dcs_cand2.ensure(ng, stream, false, 1.5f);
                if (d.geom.kind == SALVA_HIP_SHAPE_HOST) {
                    std::vector<float4>& f4 = cpl.dcs_h_f4;
                    std::vector<float>& pts = cpl.dcs_h_pts;
                    std::vector<float>& proj = cpl.dcs_h_proj;
                    f4.resize(ng); pts.resize(3 * (size_t)ng); proj.assign(3 * (size_t)ng, 0.0f); cpl.dcs_h_inside.assign(ng, 0);
                    SALVA_HIP_CHECK(hipMemcpyAsync(f4.data(), cpl.dcs_out.p, (size_t)ng * sizeof(float4), hipMemcpyDeviceToHost, stream));
                    wait_stream(); ++dcs_stats[1];
                    for (uint32_t k = 0; k < ng; ++k) { pts[3 * k] = f4[k].x; pts[3 * k + 1] = f4[k].y; pts[3 * k + 2] = f4[k].z; }
                    d.host.project(d.host.user, ng, pts.data(), proj.data(), cpl.dcs_h_inside.data());
                    for (uint32_t k = 0; k < ng; ++k)
                        f4[k] = make_float4(proj[3 * k], proj[3 * k + 1], proj[3 * k + 2], cpl.dcs_h_inside[k] ? 1.0f : 0.0f);
                    SALVA_HIP_CHECK(hipMemcpyAsync(cpl.dcs_proj.p, f4.data(), (size_t)ng * sizeof(float4), hipMemcpyHostToDevice, stream));
                } else if (d.geom.compound) {
                    launch_dcs_compound_project(ng, cpl.dcs_out.p, d.geom.parts(), d.geom.nparts(), prm_d, cpl.dcs_proj.p, stream);
                } else {
                    launch_dcs_project_mesh(ng, cpl.dcs_out.p, d.geom.mesh->dev(), prm_d, cpl.dcs_proj.p, stream);
                }
                // (dcs_out holds the gathered candidates; its compaction goes back into dcs_cand, which is free again)
                launch_dcs_apply(ng, cpl.dcs_out.p, cpl.dcs_proj.p, posm[cur].p, vel[cur].p, perm[cur].p, comm ? gtag[cur].p : nullptr, prm_d,
                                 cpl.dcs_cand2.p, cpl.dcs_flag.p, stream);
                cnt = compact_and_count(tb, cpl.dcs_cand2.p, cpl.dcs_cand.p, ng);  // (its wait also: dcs_h_f4 has been read)
                emit_src = cpl.dcs_cand.p;
            }
        }
    } catch (const HipError& e) {
        if (!comm) throw;
        local_failed = true; local_error = e; cnt = 0; emit_src = nullptr;
    } catch (const std::exception& e) {
        if (!comm) throw;
        local_failed = true; local_error = HipError(SALVA_HIP_E_INVALID, e.what()); cnt = 0; emit_src = nullptr;
    }
    // Decomposed run: each rank has emitted for the particles it OWNS; every rank then holds every rank's points (a collider's
    // contact layer: thousands of rows), so a boundary particle near a slab face has its whole boundary neighbourhood — its
    // volume — and acts on the fluid of both slabs, wherever its source particle lives.  (Mirroring more ghost planes instead
    // has no bound that holds: the point is the projection of the PREDICTED position, |v| dt + 1.5 h + the penetration depth
    // from its source.)  Each rank's force accumulator receives what its own fluid exerts: the rows are the same on every
    // rank, the per-rank forces add up.
    const uint32_t* emit_models = nullptr;
    if (comm) cnt = dist_gather_emitted(emit_src, cnt, &emit_src, &emit_models, local_failed ? &local_error : nullptr);
    const uint64_t rows = cnt;
    relayout_boundaries(&slot, 1, &rows);
    b_dirty = true;  // same count, new positions
    dcs_stats[3] += cnt;
    if (cnt) {
        const uint64_t off = boundary_offset(slot);
        d.src.ensure(cnt, stream, false, 1.5f);
        launch_dcs_emit(cnt, emit_src, d.pose, slot, bst_pos.p + off, bst_vel.p + off, d.src.p, stream);
        if (emit_models) {
            d.src_model.ensure(cnt, stream, false, 1.5f);
            SALVA_HIP_CHECK(hipMemcpyAsync(d.src_model.p, emit_models, (size_t)cnt * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        }
        SALVA_HIP_CHECK(hipMemsetAsync(bforce.p + off, 0, (size_t)cnt * sizeof(float4), stream));  // clear_forces(true) :262
    }
}

// One run of device-shape colliders (`run`: their slots, ascending, at least two) in one pass over the fluid; dcs.hip "batched runs".
//   table up -> k_dcsb_project (writes records, the push list and the counts; no particle) -> counts down, ONE wait
//   -> too small: grow, repeat from the unmodified state -> k_dcsb_push -> sort the record keys -> lay the boundary arrays out once
//   -> table up again (first row / first record / source array per collider) -> k_dcsb_emit
void World::run_dynamic_sampling_batch(const std::vector<uint32_t>& run, const TileGrid& gv) {
    const uint32_t ncol = (uint32_t)run.size();
    const size_t tab_bytes = (size_t)ncol * sizeof(DcsbEntry), cnt_bytes = ((size_t)ncol + 2) * sizeof(unsigned long long);
    // (pinned: neither copy makes the host wait; the previous batch's second upload is long done — acquire() checks)
    char* stage = cpl.dcsb_stage.acquire(tab_bytes + cnt_bytes);
    DcsbEntry* tab_h = reinterpret_cast<DcsbEntry*>(stage);
    const unsigned long long* cnt_h = reinterpret_cast<const unsigned long long*>(stage + tab_bytes);
    bool has_compound = false;
    for (uint32_t c = 0; c < ncol; ++c) {
        const DynSampling& d = *bounds[run[c]].dyn;
        DcsbEntry e{};
        e.s = d.params(sc.h, prm.particle_radius, dt_prev);
        d.fill_entry(e);
        e.slot = run[c];
        tab_h[c] = e;
        if (d.geom.compound) has_compound = true;
    }
    cpl.dcsb_tab.ensure(ncol, stream, false, 1.5f);
    cpl.dcsb_counts.ensure((size_t)ncol + 2, stream, false, 1.5f);
    SALVA_HIP_CHECK(hipMemcpyAsync(cpl.dcsb_tab.p, tab_h, tab_bytes, hipMemcpyHostToDevice, stream));
    int nbits = 1;
    while (nbits < 32 && ((uint64_t)1 << nbits) < (uint64_t)n) ++nbits;
    int cbits = 1;
    while (((uint64_t)1 << cbits) < (uint64_t)ncol) ++cbits;
    const uint32_t shift = (uint32_t)nbits;
    // the first capacity is a guess (an eighth of the fluid, or SALVA_HIP_DCSB_CAP0 for the tests); afterwards what the fullest pass
    // so far needed, with half as much again
    if (cpl.dcsb_cap == 0) cpl.dcsb_cap = sw.dcsb_cap0 ? sw.dcsb_cap0 : std::max<uint32_t>(n / 8u, 4096u);
    uint64_t total = 0, npush = 0;
    for (;;) {
        for (int k = 0; k < 2; ++k) { cpl.dcsb_key[k].ensure(cpl.dcsb_cap, stream); cpl.dcsb_idx[k].ensure(cpl.dcsb_cap, stream); }
        cpl.dcsb_rec.ensure(cpl.dcsb_cap, stream); cpl.dcsb_push_idx.ensure(cpl.dcsb_cap, stream); cpl.dcsb_push_pos.ensure(cpl.dcsb_cap, stream); cpl.dcsb_push_vel.ensure(cpl.dcsb_cap, stream);
        SALVA_HIP_CHECK(hipMemsetAsync(cpl.dcsb_counts.p, 0, cnt_bytes, stream));
        if (!has_compound) {
            launch_dcsb_project(n, posm[cur].p, vel[cur].p, G().keys[0].p, perm[cur].p, gv, cpl.dcsb_tab.p, ncol, cpl.dcsb_cap, shift, cpl.dcsb_counts.p,
                                cpl.dcsb_key[0].p, cpl.dcsb_idx[0].p, cpl.dcsb_rec.p, cpl.dcsb_push_idx.p, cpl.dcsb_push_pos.p, cpl.dcsb_push_vel.p, stream);
        } else {
            // compounds project in launches of their own (dcs.hip k_dcsb_segment): one launch per stretch of colliders of one class
            cpl.dcsb_st_pos.ensure(n, stream, false, 1.1f); cpl.dcsb_st_vel.ensure(n, stream, false, 1.1f); cpl.dcsb_st_moved.ensure(n, stream, false, 1.1f);
            for (uint32_t c0 = 0; c0 < ncol;) {
                const bool compound = tab_h[c0].s.kind == SALVA_HIP_SHAPE_COMPOUND;
                uint32_t c1 = c0 + 1;
                while (c1 < ncol && (tab_h[c1].s.kind == SALVA_HIP_SHAPE_COMPOUND) == compound) ++c1;
                launch_dcsb_segment(compound, n, posm[cur].p, vel[cur].p, G().keys[0].p, perm[cur].p, gv, cpl.dcsb_tab.p, ncol, c0, c1, cpl.dcsb_cap, shift,
                                    cpl.dcsb_counts.p, cpl.dcsb_key[0].p, cpl.dcsb_idx[0].p, cpl.dcsb_rec.p, cpl.dcsb_push_idx.p, cpl.dcsb_push_pos.p, cpl.dcsb_push_vel.p,
                                    cpl.dcsb_st_pos.p, cpl.dcsb_st_vel.p, cpl.dcsb_st_moved.p, stream);
                c0 = c1;
            }
        }
        SALVA_HIP_CHECK(hipMemcpyAsync(stage + tab_bytes, cpl.dcsb_counts.p, cnt_bytes, hipMemcpyDeviceToHost, stream));
        wait_stream();
        ++dcs_stats[0]; ++dcs_stats[1];
        total = cnt_h[ncol]; npush = cnt_h[ncol + 1];
        if (total <= cpl.dcsb_cap) break;
        // nothing has been written but the scratch of this pass: a larger buffer, the same pass again
        if (total >= 0xfffffff0ull) throw HipError(SALVA_HIP_E_CAPACITY, "too many boundary particles");
        cpl.dcsb_cap = (uint32_t)std::min<uint64_t>(total + total / 2, 0xfffffff0ull);
    }
    launch_dcsb_push((uint32_t)npush, cpl.dcsb_push_idx.p, cpl.dcsb_push_pos.p, cpl.dcsb_push_vel.p, posm[cur].p, vel[cur].p, stream);
    std::vector<uint64_t> counts(ncol);
    for (uint32_t c = 0; c < ncol; ++c) counts[c] = cnt_h[c];
    relayout_boundaries(run.data(), run.size(), counts.data());
    b_dirty = true;  // same counts, new positions
    dcs_stats[2] += ncol; dcs_stats[3] += total;
    if (total) {
        const size_t tb = sort_pairs_u64_temp_bytes((uint32_t)total, nbits + cbits);
        ensure_cub_temp(tb);
        sort_pairs_u64(cub_temp.p, tb, cpl.dcsb_key[0].p, cpl.dcsb_key[1].p, cpl.dcsb_idx[0].p, cpl.dcsb_idx[1].p, (uint32_t)total, nbits + cbits, stream);
        uint64_t rec0 = 0;
        for (uint32_t c = 0; c < ncol; ++c) {
            BoundarySlot& b = bounds[run[c]];
            if (counts[c]) b.dyn->src.ensure(counts[c], stream, false, 1.5f);
            tab_h[c].row0 = (uint32_t)boundary_offset(run[c]);
            tab_h[c].rec0 = (uint32_t)rec0;
            tab_h[c].src = b.dyn->src.p;
            rec0 += counts[c];
        }
        SALVA_HIP_CHECK(hipMemcpyAsync(cpl.dcsb_tab.p, tab_h, tab_bytes, hipMemcpyHostToDevice, stream));
        launch_dcsb_emit((uint32_t)total, cpl.dcsb_key[1].p, cpl.dcsb_idx[1].p, cpl.dcsb_rec.p, cpl.dcsb_tab.p, shift, bst_pos.p, bst_vel.p, bforce.p, stream);
    }
    cpl.dcsb_stage.release(stream);
}

// New particle counts for the slots of `run` (ascending; a run of one: the per-collider path) in one go.  The rows behind the run's
// first slot go through scratch once; of them, every stretch of consecutive slots outside the run that moves — it stays contiguous —
// comes back in one copy.  The run's own rows are left for the caller to fill.  No allocation once the buffers have grown.
void World::relayout_boundaries(const uint32_t* run, size_t nrun, const uint64_t* counts) {
    uint64_t new_total = nb;
    bool changed = false;
    for (size_t c = 0; c < nrun; ++c) {
        new_total = new_total - bounds[run[c]].n + counts[c];
        if (counts[c] != bounds[run[c]].n) changed = true;
    }
    if (!changed) return;
    if (new_total >= 0xfffffff0ull) throw HipError(SALVA_HIP_E_CAPACITY, "too many boundary particles");
    const uint64_t tail_src = boundary_offset(run[0]) + bounds[run[0]].n, tail_len = nb - tail_src;
    DevBuf<float4>* bufs[3] = {&bst_pos, &bst_vel, &bforce};
    for (DevBuf<float4>* buf : bufs) {
        buf->ensure(std::max<uint64_t>(new_total, 1), stream, true, 1.5f);
        struct Seg { uint64_t src, dst, len; } seg{0, 0, 0};
        bool staged = false;
        auto flush = [&]() {
            if (!seg.len) return;
            if (!staged) {
                scratch_f4.ensure(tail_len, stream, false, 1.5f);
                SALVA_HIP_CHECK(hipMemcpyAsync(scratch_f4.p, buf->p + tail_src, tail_len * sizeof(float4), hipMemcpyDeviceToDevice, stream));
                staged = true;
            }
            SALVA_HIP_CHECK(hipMemcpyAsync(buf->p + seg.dst, scratch_f4.p + (seg.src - tail_src), seg.len * sizeof(float4), hipMemcpyDeviceToDevice, stream));
            seg.len = 0;
        };
        uint64_t src = tail_src, dst = tail_src - bounds[run[0]].n + counts[0];  // where the next slot's rows are / go
        size_t c = 1;
        for (size_t s = (size_t)run[0] + 1; s < bounds.size(); ++s) {
            const uint64_t len = bounds[s].n;
            if (c < nrun && run[c] == s) { src += len; dst += counts[c++]; continue; }
            if (len && src != dst) {
                if (seg.len && seg.src + seg.len == src && seg.dst + seg.len == dst) seg.len += len;
                else { flush(); seg = Seg{src, dst, len}; }
            }
            src += len; dst += len;
        }
        flush();
    }
    for (size_t c = 0; c < nrun; ++c) bounds[run[c]].n = counts[c];
    nb = (uint32_t)new_total;
    b_dirty = true; have_last_ctx = false;
}

// (fluid slot, index) of the fluid particle each point of a dynamically sampled boundary was projected from
void World::get_boundary_sources(uint32_t slot, uint32_t* fluid_slots, uint32_t* indices) {
    use_device();
    if (slot >= bounds.size()) throw HipError(SALVA_HIP_E_INVALID, "boundary slot out of range");
    const BoundarySlot& b = bounds[slot];
    if (!b.dyn) throw HipError(SALVA_HIP_E_INVALID, "boundary is not dynamically sampled");
    if (!b.n) return;
    std::vector<uint32_t> src(b.n);
    SALVA_HIP_CHECK(hipMemcpyAsync(src.data(), b.dyn->src.p, b.n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (comm) {  // decomposed run: the global id of the source particle (salva_hip_get_local's `ids`) and its fluid
        if (indices) SALVA_HIP_CHECK(hipMemcpyAsync(indices, b.dyn->src.p, b.n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        if (fluid_slots) SALVA_HIP_CHECK(hipMemcpyAsync(fluid_slots, b.dyn->src_model.p, b.n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
        return;
    }
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    for (uint64_t k = 0; k < b.n; ++k) {
        uint32_t f = 0;
        uint64_t o = 0;
        while (f + 1 < fluids.size() && src[k] >= o + fluids[f].n) { o += fluids[f].n; ++f; }
        if (fluid_slots) fluid_slots[k] = f;
        if (indices) indices[k] = (uint32_t)(src[k] - o);
    }
}

void World::get_boundary_wrench(uint32_t slot, const float point[3], float force[3], float torque[3]) {
    use_device();
    if (slot >= bounds.size()) throw HipError(SALVA_HIP_E_INVALID, "boundary slot out of range");
    const BoundarySlot& b = bounds[slot];
    for (int k = 0; k < 3; ++k) force[k] = torque[k] = 0.0f;
    if (!b.n || !b.wants_forces) return;
    const uint64_t off = boundary_offset(slot);
    const uint32_t nblocks = (uint32_t)std::min<uint64_t>(nblk(b.n), 256);
    cpl.wrench_partial.ensure((size_t)256 * 6);  // per-step call in a coupled run: no allocation on the way
    k_boundary_wrench<<<nblocks, BLOCK, 0, stream>>>((uint32_t)b.n, bst_pos.p + off, bforce.p + off, point[0], point[1], point[2], cpl.wrench_partial.p);
    SALVA_HIP_CHECK(hipGetLastError());
    std::vector<double> h((size_t)nblocks * 6);
    SALVA_HIP_CHECK(hipMemcpyAsync(h.data(), cpl.wrench_partial.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t k = 0; k < nblocks; ++k)
        for (int j = 0; j < 6; ++j) acc[j] += h[(size_t)k * 6 + j];
    for (int k = 0; k < 3; ++k) { force[k] = (float)acc[k]; torque[k] = (float)acc[3 + k]; }
}

// `count` calls of get_boundary_wrench with one launch, one copy and one wait (points / forces / torques: 3 floats per entry)
void World::get_boundary_wrenches(uint32_t count, const uint32_t* slots, const float* points, float* forces, float* torques) {
    use_device();
    for (uint32_t k = 0; k < count; ++k)
        if (slots[k] >= bounds.size()) throw HipError(SALVA_HIP_E_INVALID, "boundary slot out of range");
    std::vector<uint32_t> live;  // the entries with something to sum
    uint64_t nblocks = 0;
    for (uint32_t k = 0; k < count; ++k) {
        const BoundarySlot& b = bounds[slots[k]];
        for (int a = 0; a < 3; ++a) forces[3 * (size_t)k + a] = torques[3 * (size_t)k + a] = 0.0f;
        if (!b.n || !b.wants_forces) continue;
        live.push_back(k);
        nblocks += std::min<uint64_t>(nblk(b.n), 256);
    }
    if (live.empty()) return;
    const size_t ent_bytes = live.size() * sizeof(WrenchEntry), part_bytes = (size_t)nblocks * 6 * sizeof(double);
    char* stage = cpl.wrench_stage.acquire(ent_bytes + part_bytes);
    WrenchEntry* ent_h = reinterpret_cast<WrenchEntry*>(stage);
    uint32_t block0 = 0;
    for (size_t e = 0; e < live.size(); ++e) {
        const uint32_t k = live[e];
        const BoundarySlot& b = bounds[slots[k]];
        const uint32_t nbk = (uint32_t)std::min<uint64_t>(nblk(b.n), 256);
        ent_h[e] = WrenchEntry{(uint32_t)boundary_offset(slots[k]), (uint32_t)b.n, block0, nbk, {points[3 * (size_t)k], points[3 * (size_t)k + 1], points[3 * (size_t)k + 2]}, 0u};
        block0 += nbk;
    }
    cpl.wrench_tab.ensure(ent_bytes, stream, false, 1.5f);
    cpl.wrenches_partial.ensure((size_t)nblocks * 6, stream, false, 1.5f);
    SALVA_HIP_CHECK(hipMemcpyAsync(cpl.wrench_tab.p, ent_h, ent_bytes, hipMemcpyHostToDevice, stream));
    k_boundary_wrenches<<<(uint32_t)nblocks, BLOCK, 0, stream>>>((uint32_t)live.size(), reinterpret_cast<const WrenchEntry*>(cpl.wrench_tab.p), bst_pos.p,
                                                                 bforce.p, cpl.wrenches_partial.p);
    SALVA_HIP_CHECK(hipGetLastError());
    SALVA_HIP_CHECK(hipMemcpyAsync(stage + ent_bytes, cpl.wrenches_partial.p, part_bytes, hipMemcpyDeviceToHost, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    const double* h = reinterpret_cast<const double*>(stage + ent_bytes);
    for (size_t e = 0; e < live.size(); ++e) {
        double acc[6] = {0, 0, 0, 0, 0, 0};
        for (uint32_t k = 0; k < ent_h[e].nblocks; ++k)
            for (int j = 0; j < 6; ++j) acc[j] += h[(size_t)(ent_h[e].block0 + k) * 6 + j];
        for (int a = 0; a < 3; ++a) { forces[3 * (size_t)live[e] + a] = (float)acc[a]; torques[3 * (size_t)live[e] + a] = (float)acc[3 + a]; }
    }
}

void World::clear_boundary_forces(uint32_t slot) {
    use_device();
    if (slot >= bounds.size()) throw HipError(SALVA_HIP_E_INVALID, "boundary slot out of range");
    const uint64_t nn = bounds[slot].n, off = boundary_offset(slot);
    if (nn) {
        SALVA_HIP_CHECK(hipMemsetAsync(bforce.p + off, 0, nn * sizeof(float4), stream));
        SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    }
}

}  // namespace salva

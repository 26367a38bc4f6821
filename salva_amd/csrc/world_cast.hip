// world_cast.hip — rays cast at the fluid's particles (salva_hip_cast_rays / _cast_rays_camera): what a call must be, the
// box B of the call (the clip box, or the fluids' own box reduced on the device), the evaluator's cell table over it with the host-order
// row of every sorted row, the buffers of the caller, and the one kernel of fluidcast.hip.  Nothing here writes anything a step reads.
#include "world.h"
#include "dcs.h"

#include <cmath>
#include <cstring>

namespace salva {

static_assert(SALVA_HIP_RAY_RAYS_ON_DEVICE == SALVA_HIP_FIELD_POINTS_ON_DEVICE && SALVA_HIP_RAY_OUT_ON_DEVICE == SALVA_HIP_FIELD_OUT_ON_DEVICE,
              "World::field_begin checks the flags of both families");
static_assert(sizeof(SalvaHipRayParams) == SALVA_HIP_RAY_PARAMS_BYTES && sizeof(SalvaHipRayCamera) == SALVA_HIP_RAY_CAMERA_BYTES, "as the header says");

// count_walk: 0 - a cast; 1 / 2 - salva_hip_count_ray_candidates of the first-hit / the thickness walk, into `tested` (out: all null)
void World::cast_run(uint32_t fluid_mask, const SalvaHipRayParams* params, CastRays rays, uint32_t flags, const SalvaHipRayOut& out, const char* what,
                     int count_walk, uint32_t* tested) {
    const std::string w(what);
    const FieldFluids f = field_begin(fluid_mask, flags, what);
    if (!params) throw HipError(SALVA_HIP_E_INVALID, w + ": null params");
    if (params->struct_size != SALVA_HIP_RAY_PARAMS_BYTES || params->version != SALVA_HIP_RAY_VERSION)
        throw HipError(SALVA_HIP_E_INVALID, w + ": struct_size / version are not this library's SalvaHipRayParams (SALVA_HIP_RAY_PARAMS_BYTES, SALVA_HIP_RAY_VERSION)");
    const float R = params->radius;
    if (!(std::isfinite(R) && R > 0.0f && R <= 0.5f * sc.h)) throw HipError(SALVA_HIP_E_INVALID, w + ": radius must be finite, > 0 and at most h / 2");
    if (!(params->tmax >= 0.0f)) throw HipError(SALVA_HIP_E_INVALID, w + ": tmax must be >= 0 (+inf allowed)");
    if (params->has_clip > 1u) throw HipError(SALVA_HIP_E_INVALID, w + ": has_clip must be 0 or 1");
    if (params->has_clip)
        for (int a = 0; a < 3; ++a)
            if (!(std::isfinite(params->clip_lo[a]) && std::isfinite(params->clip_hi[a]) && params->clip_lo[a] <= params->clip_hi[a]))
                throw HipError(SALVA_HIP_E_INVALID, w + ": the clip box must be finite with clip_lo <= clip_hi");
    const uint64_t m = rays.nrays;
    if (m > (1ull << 32)) throw HipError(SALVA_HIP_E_CAPACITY, w + ": more than 2^32 rays: split the call");
    if (m == 0) return;

    // the caller's buffers
    const bool out_dev = (flags & SALVA_HIP_RAY_OUT_ON_DEVICE) != 0u, rays_dev = (flags & SALVA_HIP_RAY_RAYS_ON_DEVICE) != 0u;
    QueryOut o{{{out.t, m}, {out.fluid, m}, {out.index, m}, {out.normal, 3 * m}, {out.thickness, m}, {tested, m}}};
    query_place(o, out_dev);
    const bool hit = count_walk ? count_walk == 1 : o.any(0, 4), thick = count_walk ? count_walk == 2 : o.f32(4) != nullptr;
    if (!hit && !thick) return;
    const CastOutDev od{o.f32(0), o.u32(1), o.u32(2), o.f32(3), o.f32(4), o.u32(5)};

    // the box B
    CastParams P{};
    P.radius = R; P.tmax = params->tmax;
    bool any = true;
    if (params->has_clip) {
        for (int a = 0; a < 3; ++a) { P.blo[a] = params->clip_lo[a]; P.bhi[a] = params->clip_hi[a]; }
    } else {
        uint64_t nfinite = 0;
        get_fluid_bounds(f.mask, P.blo, P.bhi, &nfinite);
        any = nfinite != 0;
    }
    if (!any) {
        launch_fluid_cast_miss(m, od, stream);
    } else {
        // B grown by one cell, as field_candidates will cut it
        int clo[3], chi[3];
        cell_range(P.blo, P.bhi, sc.h, clo, chi);
        uint64_t ncells = 1;
        bool over = false;
        for (int a = 0; a < 3; ++a) {
            const uint64_t d = (uint64_t)((int64_t)chi[a] - (int64_t)clo[a] + 3);
            over = over || d > CAST_MAX_AXIS_CELLS;
            ncells = ncells * d > FIELD_MAX_CELLS ? FIELD_MAX_CELLS + 1 : ncells * d;
        }
        if (over || ncells > FIELD_MAX_CELLS)
            throw HipError(SALVA_HIP_E_CAPACITY, w + ": the box of the particles exceeds 2^27 cells of width h, or 2^16 on an axis: give a clip box");
        for (int a = 0; a < 3; ++a) { P.glo[a] = P.blo[a] - R; P.ghi[a] = P.bhi[a] + R; }
        P.eps = cast_eps(P.glo, P.ghi);
        if (rays.origins && !rays_dev) {
            cst.rays.ensure(6 * m, stream, false, 1.1f);
            SALVA_HIP_CHECK(hipMemcpyAsync(cst.rays.p, rays.origins, 3 * m * sizeof(float), hipMemcpyHostToDevice, stream));
            SALVA_HIP_CHECK(hipMemcpyAsync(cst.rays.p + 3 * m, rays.directions, 3 * m * sizeof(float), hipMemcpyHostToDevice, stream));
            rays.origins = cst.rays.p; rays.directions = cst.rays.p + 3 * m;
        }
        FieldGrid g{};
        const FieldCandidates cand = field_candidates(f, P.blo, P.bhi, false, g, true);
        CastTable tab{};
        tab.cells = cand.cells; tab.rec0 = cand.rec0; tab.rows = fld.rows.p; tab.st_model = st_model.p;
        for (uint32_t s = 0; s < fluids.size() && s < FIELD_MAX_SLOTS; ++s) tab.first[s] = (uint32_t)fluid_offset(s);
        // a clip box may hold no particle at all: then every ray misses and the walk does not run
        uint32_t kept = 1u;
        if (params->has_clip) {
            SALVA_HIP_CHECK(hipMemcpyAsync(&kept, cand.cells + g.ncells, sizeof(kept), hipMemcpyDeviceToHost, stream));
            SALVA_HIP_CHECK(hipStreamSynchronize(stream));
        }
        if (kept) launch_fluid_cast(rays, P, g, tab, od, hit, thick, stream);
        else launch_fluid_cast_miss(m, od, stream);
    }
    query_finish(o);  // (it waits: the results are complete, and staged rays are free again)
}

static CastRays camera_rays(const SalvaHipRayCamera& camera, const std::string& w) {
    if (camera.struct_size != SALVA_HIP_RAY_CAMERA_BYTES || camera.version != SALVA_HIP_RAY_VERSION)
        throw HipError(SALVA_HIP_E_INVALID, w + ": struct_size / version are not this library's SalvaHipRayCamera (SALVA_HIP_RAY_CAMERA_BYTES, SALVA_HIP_RAY_VERSION)");
    if (!camera.width || !camera.height) throw HipError(SALVA_HIP_E_INVALID, w + ": width and height must be at least 1");
    CastRays r{};
    r.nrays = (uint64_t)camera.width * camera.height;
    for (int a = 0; a < 3; ++a) { r.cam_o[a] = camera.origin[a]; r.cam_f[a] = camera.forward[a]; r.cam_r[a] = camera.right[a]; r.cam_u[a] = camera.up[a]; }
    r.width = camera.width; r.height = camera.height;
    return r;
}

void World::cast_rays(uint32_t fluid_mask, const SalvaHipRayParams* params, uint64_t nrays, const float* origins_xyz, const float* directions_xyz,
                      uint32_t flags, const SalvaHipRayOut& out) {
    const char* what = "salva_hip_cast_rays";
    if (nrays && (!origins_xyz || !directions_xyz)) {
        field_begin(fluid_mask, flags, what);  // (the refusals that come first)
        throw HipError(SALVA_HIP_E_INVALID, std::string(what) + ": null origins or directions");
    }
    CastRays r{};
    r.origins = origins_xyz; r.directions = directions_xyz; r.nrays = nrays;
    cast_run(fluid_mask, params, r, flags, out, what);
}

void World::count_ray_candidates(uint32_t fluid_mask, const SalvaHipRayParams* params, const SalvaHipRayCamera* camera, uint64_t nrays,
                                 const float* origins_xyz, const float* directions_xyz, uint32_t flags, uint32_t thickness_walk, uint32_t* tested) {
    const std::string w = "salva_hip_count_ray_candidates";
    if (thickness_walk > 1u) throw HipError(SALVA_HIP_E_INVALID, w + ": thickness_walk must be 0 or 1");
    const SalvaHipRayOut none{nullptr, nullptr, nullptr, nullptr, nullptr};
    CastRays r{};
    if (camera) {
        if (flags & SALVA_HIP_RAY_RAYS_ON_DEVICE) throw HipError(SALVA_HIP_E_INVALID, w + ": unknown flag (a camera has no ray arrays)");
        r = camera_rays(*camera, w);
    } else {
        if (nrays && (!origins_xyz || !directions_xyz)) {
            field_begin(fluid_mask, flags, w.c_str());  // (the refusals that come first)
            throw HipError(SALVA_HIP_E_INVALID, w + ": null origins or directions");
        }
        r.origins = origins_xyz; r.directions = directions_xyz; r.nrays = nrays;
    }
    cast_run(fluid_mask, params, r, flags, none, w.c_str(), thickness_walk ? 2 : 1, tested);
}

void World::cast_rays_camera(uint32_t fluid_mask, const SalvaHipRayParams* params, const SalvaHipRayCamera* camera, uint32_t flags,
                             const SalvaHipRayOut& out) {
    const std::string w = "salva_hip_cast_rays_camera";
    if (flags & SALVA_HIP_RAY_RAYS_ON_DEVICE) throw HipError(SALVA_HIP_E_INVALID, w + ": unknown flag (a camera has no ray arrays)");
    cast_run(fluid_mask, params, camera_rays(*camera, w), flags, out, w.c_str());
}

}  // namespace salva

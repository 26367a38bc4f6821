// compound.hip — the host side of a device-resident compound collider (compound.h): validation, the parts' table with
// parry's per-part boxes, and the world's compound table.
#include <algorithm>
#include <cmath>

#include "compound.h"
#include "world.h"

namespace salva {

void compound_build_table(const SalvaHipCompoundPart* parts, uint32_t nparts, const std::vector<const MeshRes*>& part_meshes,
                          std::vector<CompoundPartDev>& table, float mins[3], float maxs[3]) {
    if (!parts) throw HipError(SALVA_HIP_E_INVALID, "compound: null parts");
    if (nparts == 0 || nparts > (uint32_t)SALVA_HIP_COMPOUND_MAX_PARTS) throw HipError(SALVA_HIP_E_INVALID, "compound: between 1 and 64 parts");
    table.assign(nparts, CompoundPartDev{});
    for (int a = 0; a < 3; ++a) { mins[a] = INFINITY; maxs[a] = -INFINITY; }
    float maxabs = 0.0f;
    for (uint32_t k = 0; k < nparts; ++k) {
        const SalvaHipCompoundPart& in = parts[k];
        CompoundPartDev& d = table[k];
        const bool is_mesh = in.kind == SALVA_HIP_SHAPE_MESH;
        SalvaHipShape sh{};
        sh.kind = in.kind;
        for (int a = 0; a < 3; ++a) sh.params[a] = in.params[a];
        if (!is_mesh) {
            try { shape_param_count(in.kind); }
            catch (const HipError&) { throw HipError(SALVA_HIP_E_INVALID, "compound: a part is a ball, a cuboid, a capsule, a cylinder or a mesh (no nesting, no host parts)"); }
            check_shape_params(sh, "compound: shape parameters must be positive and finite");
        } else if (part_meshes[k] == nullptr) {
            throw HipError(SALVA_HIP_E_INVALID, "no such mesh");
        }
        float qn = 0.0f;
        for (int a = 0; a < 4; ++a) {
            if (!std::isfinite(in.rotation_ijkw[a])) throw HipError(SALVA_HIP_E_INVALID, "compound: non-finite part rotation");
            qn += in.rotation_ijkw[a] * in.rotation_ijkw[a];
        }
        if (std::fabs(qn - 1.0f) > 1.0e-3f) throw HipError(SALVA_HIP_E_INVALID, "compound: a part's rotation must be a unit quaternion (x, y, z, w)");
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(in.translation[a])) throw HipError(SALVA_HIP_E_INVALID, "compound: non-finite part translation");
        d.kind = in.kind;
        d.eps = 1.1920929e-7f;
        for (int a = 0; a < 3; ++a) { d.p[a] = is_mesh ? 0.0f : in.params[a]; d.t[a] = in.translation[a]; }
        for (int a = 0; a < 4; ++a) d.q[a] = in.rotation_ijkw[a];
        // parry's part.compute_aabb(part_pos)
        if (is_mesh) {
            aabb_transform_by(part_meshes[k]->mins, part_meshes[k]->maxs, d.t, d.q, d.lo, d.hi);
            d.mesh = part_meshes[k]->dev();
        } else {
            float ext[3];
            shape_world_extent(sh, d.q, ext);
            for (int a = 0; a < 3; ++a) { d.lo[a] = d.t[a] - ext[a]; d.hi[a] = d.t[a] + ext[a]; }
        }
        for (int a = 0; a < 3; ++a) {
            mins[a] = std::min(mins[a], d.lo[a]); maxs[a] = std::max(maxs[a], d.hi[a]);
            maxabs = std::max(maxabs, std::max(std::fabs(d.lo[a]), std::fabs(d.hi[a])));
        }
    }
    // (mesh.hip's rule: a projection is a rounded combination of the part's data and may leave its exact box by an ulp or two)
    const float margin = std::max(maxabs * 3.814697265625e-6f, 1e-30f);
    for (CompoundPartDev& d : table)
        for (int a = 0; a < 3; ++a) { d.lo[a] -= margin; d.hi[a] += margin; }
}

// ------------------------------------------------------------------------------------------------ the world's compound table
uint32_t World::create_compound(const SalvaHipCompoundPart* parts, uint32_t nparts) {
    use_device();
    if (!parts) throw HipError(SALVA_HIP_E_INVALID, "compound: null parts");
    if (nparts == 0 || nparts > (uint32_t)SALVA_HIP_COMPOUND_MAX_PARTS) throw HipError(SALVA_HIP_E_INVALID, "compound: between 1 and 64 parts");
    auto c = std::make_shared<CompoundRes>();
    std::vector<const MeshRes*> part_meshes(nparts, nullptr);
    for (uint32_t k = 0; k < nparts; ++k)
        if (parts[k].kind == SALVA_HIP_SHAPE_MESH) {
            const std::shared_ptr<MeshRes>& m = mesh_at(parts[k].mesh);
            part_meshes[k] = m.get();
            c->meshes.push_back(m);
            if (!(m->flags & SALVA_HIP_MESH_ORIENTED)) c->solid = false;
        }
    std::vector<CompoundPartDev> table;
    compound_build_table(parts, nparts, part_meshes, table, c->mins, c->maxs);
    c->nparts = nparts;
    c->parts.ensure(nparts);
    SALVA_HIP_CHECK(hipMemcpyAsync(c->parts.p, table.data(), (size_t)nparts * sizeof(CompoundPartDev), hipMemcpyHostToDevice, stream));
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));  // (the host table leaves scope)
    for (uint32_t k = 0; k < compounds.size(); ++k)
        if (!compounds[k]) { compounds[k] = c; return k; }
    compounds.push_back(c);
    return (uint32_t)compounds.size() - 1;
}

const std::shared_ptr<CompoundRes>& World::compound_at(uint32_t compound) const {
    if (compound >= compounds.size() || !compounds[compound]) throw HipError(SALVA_HIP_E_INVALID, "no such compound");
    return compounds[compound];
}

void World::destroy_compound(uint32_t compound) {
    use_device();
    if (compound_at(compound).use_count() > 1)
        throw HipError(SALVA_HIP_E_INVALID, "the compound is the collider of a dynamically sampled boundary (salva_hip_clear_boundary_sampling releases it) or the region of a sink (salva_hip_remove_sink releases it)");
    SALVA_HIP_CHECK(hipStreamSynchronize(stream));
    compounds[compound].reset();
}

}  // namespace salva

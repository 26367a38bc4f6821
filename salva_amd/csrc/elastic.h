// elastic.h — the state of one Becker2009Elasticity entry (solver/elasticity/becker2009_elasticity.rs) and the launchers of
// elastic.hip.  Everything per particle is in the fluid's HOST order (the reference never permutes it: apply_permutation is dead
// upstream); the step's passes reach it from the cell-sorted working set through StepCtx::perm.
#pragma once
#include "common.h"
#include "device_types.h"

namespace salva {

struct ElasticState {
    uint64_t n0 = 0;          // positions0.len(): the rest state is re-initialised when the fluid's count differs (:84-112)
    bool list_valid = false;  // the rest lists match positions0 (false after salva_hip_set_elasticity_state)
    uint64_t nnz = 0;         // rest contacts, self pairs included
    DevBuf<float4> p0;        // [n0] positions0 (xyz, 0)
    DevBuf<float> vol0;       // [n0] volumes0
    DevBuf<float> rot;        // [9 n0] rotations, row-major: the last completed step's (the warm start of the next extraction)
    DevBuf<float> rot_new;    // [9 n0] this step's, swapped into `rot` when the step completes (World::commit_elastic): a pass
                              // that is discarded and repeated, or continued after a broken chain, extracts from the same start
    bool ran = false;         // rot_new holds this step's rotations
    DevBuf<float> sig;        // [6 n0] stress (xx, yy, zz, xy, xz, yz)
    DevBuf<float> F;          // [9 n0] deformation_gradient_tr, row-major (m_rc = F[3 r + c])
    DevBuf<float4> hp;        // [n0] this step's positions in host order (xyz, mass)
    DevBuf<uint32_t> off;     // [n0 + 1] rest lists as CSR, each row ascending in j
    DevBuf<uint32_t> nbr;     // [nnz]
};

// The force's coefficients (p[] of SALVA_HIP_FORCE_BECKER2009) and its own KernelDensity / KernelGradient.
struct ElasticParams {
    float d0, d1, d2;
    int nonlinear;
    int kd, kg;  // SALVA_HIP_KERNEL_* (0 = CubicSplineKernel)
};
ElasticParams elastic_params(const float p[7]);

// `positions0 = fluid.positions` and the rest lists (compute_self_contacts, contacts.rs:403-446) from e.p0, then — unless
// `lists_only` — volumes0 with the reference's accumulation (quirks 1 and 2 in DESIGN.md §12).  Synchronises the stream.
void elastic_build_rest(ElasticState& e, const SphConsts& sc, const ElasticParams& ep, bool lists_only, hipStream_t s);
// this step's positions and masses of fluid particles [off, off + nn) into host order: e.hp
void launch_elastic_gather(const StepCtx& c, uint32_t off, ElasticState& e, hipStream_t s);
// p0 := hp (the positions of an initialising step)
void launch_elastic_take_rest(ElasticState& e, hipStream_t s);
// rotations, deformation gradients and stresses (compute_rotations + compute_stresses, :115-262), one pass
void launch_elastic_rot_stress(const StepCtx& c, ElasticState& e, const ElasticParams& ep, hipStream_t s);
// accelerations of the fluid's particles (:268-334), added to c.acc in sorted order
void launch_elastic_forces(const StepCtx& c, uint32_t off, ElasticState& e, const ElasticParams& ep, float4* acc, hipStream_t s);
// rotations [from, to) := identity
void launch_elastic_identity(ElasticState& e, uint64_t from, uint64_t to, hipStream_t s);

}  // namespace salva

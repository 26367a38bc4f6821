// pose.h — the one place a collider-local point is carried into world space on the device (k_boundary_pose in world_coupling.hip,
// k_sample_emit in sample.hip): two paths that pose the same point must produce the same bits.
#pragma once
#include "common.h"
#include "sph_math.h"

namespace salva {

#ifdef __HIPCC__
// q * v + t of nalgebra's UnitQuaternion (geometry/quaternion_ops.rs): u = 2 q.vec x v; v' = v + w u + q.vec x u.
// Every product is rounded on its own (no FMA contraction): these positions feed the exact d^2 <= h^2 contact test, and
// sample points 2r apart make pairs that sit exactly on d = h (found by the literal basic3 scene: 250 boundary-boundary
// contacts fewer than the CPU with contracted products)
__device__ __forceinline__ void pose_point(float qx, float qy, float qz, float qw, float t0, float t1, float t2, float px, float py,
                                           float pz, float& ox, float& oy, float& oz) {
    const float tx = (opaque(qy * pz) - opaque(qz * py)) * 2.0f, ty = (opaque(qz * px) - opaque(qx * pz)) * 2.0f,
                tz = (opaque(qx * py) - opaque(qy * px)) * 2.0f;
    const float cx = opaque(qy * tz) - opaque(qz * ty), cy = opaque(qz * tx) - opaque(qx * tz), cz = opaque(qx * ty) - opaque(qy * tx);
    ox = ((opaque(tx * qw) + cx) + px) + t0;
    oy = ((opaque(ty * qw) + cy) + py) + t1;
    oz = ((opaque(tz * qw) + cz) + pz) + t2;
}
#endif

}  // namespace salva

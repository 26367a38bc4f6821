// salva_hip_device.h — what a user's kernel needs to be a `NonPressureForce` (solver/nonpressure_force.rs:10-30) on the device.
//
// HIP, for user kernels; the C ABI is include/salva_hip.h and stays free of HIP.  A force of kind SALVA_HIP_FORCE_DEVICE gets a
// SalvaHipDeviceView from the callback of salva_hip_set_device_force_callback; the callback launches a kernel on
// salva_dev_stream(view) with the view (by value: it is 240 bytes of pointers and scalars) and returns.  A kernel may read every
// array of the view, add to `acc`, and hand a reaction force to a boundary particle with salva_dev_boundary_add_force; it touches
// rows below `n` / `nb` only.  examples/device_forces3.hip is the worked example.
//
// 4-vectors: the view declares them as packed floats (the C header knows no float4); salva_dev_f4 reads row i as one 16-byte load.
#ifndef SALVA_HIP_DEVICE_H
#define SALVA_HIP_DEVICE_H

#include <hip/hip_runtime.h>

#include "salva_hip.h"

inline hipStream_t salva_dev_stream(const SalvaHipDeviceView* view) { return (hipStream_t)view->stream; }

// the user's parameter k (0 ... 5) of the force entry: params[0] carries the SALVA_HIP_DEVICE_NEEDS_* bits, the user's follow it
__host__ __device__ inline float salva_dev_param(const SalvaHipDeviceView& view, int k) { return view.params[1 + k]; }

__device__ __forceinline__ float4 salva_dev_f4(const float* base, unsigned long long row) {
    return reinterpret_cast<const float4*>(base)[row];
}

// ---- the reference's kernels (src/kernel/{cubic_spline,poly6,spiky,viscosity}_kernel.rs), support radius h, `kind` = SALVA_HIP_KERNEL_*.
// salva_dev_w = Kernel::scalar_apply(r, h); salva_dev_grad = Kernel::apply_diff(d, h) for d = x_i - x_j (kernel.rs:13-24): zero for
// |d|^2 <= f32::EPSILON^2.  The contact tables carry both for the world's own kernel pair (ff_kern / fb_kern); these are for a
// force with a kernel of its own choice, like the reference's forces with their own type parameters.
__device__ __forceinline__ float salva_dev_w(int kind, float r, float h) {
    const float pi = 3.14159265358979323846f;
    if (!(r <= h)) return 0.0f;
    const float h3 = h * h * h;
    if (kind == SALVA_HIP_KERNEL_POLY6) { const float d = h * h - r * r; return (315.0f / 64.0f) / (pi * (h3 * h3 * h3)) * (d * d * d); }
    if (kind == SALVA_HIP_KERNEL_SPIKY) { const float d = h - r; return 15.0f / (pi * (h3 * h3)) * (d * d * d); }
    if (kind == SALVA_HIP_KERNEL_VISCOSITY) {
        if (!(r > 0.0f)) return 0.0f;
        return 15.0f / (2.0f * pi * h3) * (r * r / (h * h) * (1.0f - r / (2.0f * h)) + h / (2.0f * r) - 1.0f);
    }
    const float q = r / h, norm = 8.0f / (pi * h3);
    if (q <= 0.5f) return norm * (1.0f + (q * q * q - q * q) * 6.0f);
    const float omq = 1.0f - q;
    return norm * (omq * omq * omq * 2.0f);
}
// dW/dr
__device__ __forceinline__ float salva_dev_dw(int kind, float r, float h) {
    const float pi = 3.14159265358979323846f;
    if (!(r <= h)) return 0.0f;
    const float h3 = h * h * h;
    if (kind == SALVA_HIP_KERNEL_POLY6) { const float d = h * h - r * r; return (315.0f / 64.0f) / (pi * (h3 * h3 * h3)) * (d * d) * r * -6.0f; }
    if (kind == SALVA_HIP_KERNEL_SPIKY) { const float d = h - r; return -(15.0f / (pi * (h3 * h3))) * (d * d) * 3.0f; }
    if (kind == SALVA_HIP_KERNEL_VISCOSITY) {
        if (!(r > 0.0f)) return 0.0f;
        const float rr = r * r, hh = h * h;
        return 15.0f / (2.0f * pi * h3) * (-3.0f * rr / (2.0f * h3) + 2.0f * r / hh - h / (2.0f * rr));
    }
    const float q = r / h, norm = 8.0f / (pi * h3) / h;
    if (q <= 1.0e-5f) return 0.0f;  // cubic_spline_kernel.rs:63-65
    if (q <= 0.5f) return norm * ((q * 3.0f - 2.0f) * q * 6.0f);
    const float omq = 1.0f - q;
    return norm * (-omq * omq * 6.0f);
}
__device__ __forceinline__ float3 salva_dev_grad(int kind, float dx, float dy, float dz, float h) {
    const float r2 = dx * dx + dy * dy + dz * dz;
    if (!(r2 > 1.1920929e-7f * 1.1920929e-7f)) return make_float3(0.0f, 0.0f, 0.0f);
    const float r = sqrtf(r2), g = salva_dev_dw(kind, r, h) / r;
    return make_float3(g * dx, g * dy, g * dz);
}

// fluid.volumes[i] of row i: the mass over the fluid's density0 (fluid.rs:183-185)
__device__ __forceinline__ float salva_dev_volume(const SalvaHipDeviceView& view, unsigned int i) {
    return view.posm[4ull * i + 3] / view.rho0[view.model[i]];
}

// Boundary::apply_force (boundary.rs:62-67) for the boundary particle in sorted row b, as the built-in kernels do it: three 64-bit
// fixed-point atomic adds into the particle's accumulator in host order (integer sums do not depend on the order of arrival), skipped
// when no boundary, or not this one, asked for forces.
__device__ __forceinline__ void salva_dev_boundary_add_force(const SalvaHipDeviceView& view, unsigned int b, float fx, float fy, float fz) {
    if (view.bforce_fx == nullptr || !view.bwants[__float_as_uint(view.bvel[4ull * b + 3])]) return;
    unsigned long long* f = reinterpret_cast<unsigned long long*>(view.bforce_fx) + 3ull * view.bid[b];
    atomicAdd(f + 0, (unsigned long long)__float2ll_rn(fx * view.bforce_scale));
    atomicAdd(f + 1, (unsigned long long)__float2ll_rn(fy * view.bforce_scale));
    atomicAdd(f + 2, (unsigned long long)__float2ll_rn(fz * view.bforce_scale));
}

#endif  // SALVA_HIP_DEVICE_H

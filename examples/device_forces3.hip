// device_forces3.hip — user-defined NonPressureForces as kernels (SALVA_HIP_FORCE_DEVICE; include/salva_hip_device.h).
//
// One source, two products (examples/Makefile):
//   libdevice_forces3.so   a plugin: `int symbol(const SalvaHipDeviceView*)` entry points that enqueue a kernel on the view's stream,
//                          what salva_amd.PluginForce loads and what a Rust user links
//       df3_field   the force field of examples3d/custom_forces3.rs:67-90: acc += dir / dist towards the point in the
//                   user's parameters 0 .. 2, where dist > 0.1
//       df3_xsph    XSPHViscosity::solve (solver/viscosity/xsph_viscosity.rs:31-95) over the view's contact tables and
//                   kernel values: user parameter 0 = fluid coefficient, 1 = boundary coefficient; needs = FF | FB | KERNEL
//   device_forces3         (-DDF3_MAIN) the custom_forces3 scene — a 10^3 block, no gravity, one field on either side — through the
//                          C++ mirror, with df3_field as a salva::DeviceForce
#include <hip/hip_runtime.h>

#include "../include/salva_hip_device.h"

namespace {

constexpr int DF3_BLOCK = 256;

__global__ __launch_bounds__(DF3_BLOCK) void k_df3_field(SalvaHipDeviceView v) {
    const unsigned i = blockIdx.x * DF3_BLOCK + threadIdx.x;
    if (i >= v.n || v.model[i] != v.fluid_slot) return;  // (the working set holds every fluid: this force belongs to one)
    const float4 p = salva_dev_f4(v.posm, i);
    const float dx = salva_dev_param(v, 0) - p.x, dy = salva_dev_param(v, 1) - p.y, dz = salva_dev_param(v, 2) - p.z;
    const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
    if (!(dist > 0.1f)) return;  // Unit::try_new_and_get(v, 0.1)
    float4* acc = reinterpret_cast<float4*>(v.acc) + i;
    float4 a = *acc;
    a.x += dx / dist / dist; a.y += dy / dist / dist; a.z += dz / dist / dist;
    *acc = a;
}

// one thread per particle over its two rows; W_ij comes from the tables (the fourth component of a kernel entry)
__global__ __launch_bounds__(DF3_BLOCK) void k_df3_xsph(SalvaHipDeviceView v) {
    const unsigned i = blockIdx.x * DF3_BLOCK + threadIdx.x;
    if (i >= v.n || v.model[i] != v.fluid_slot) return;
    const float fc = salva_dev_param(v, 0), bc = salva_dev_param(v, 1);
    const float4 vi = salva_dev_f4(v.vel, i);
    const float rho0 = v.rho0[v.fluid_slot];
    float fx = 0.0f, fy = 0.0f, fz = 0.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
    if (fc != 0.0f)
        for (unsigned long long e = v.ff_off[i]; e < v.ff_off[i + 1]; ++e) {
            const unsigned j = v.ff_j[e];
            if (v.model[j] != v.fluid_slot) continue;  // c.i_model == c.j_model
            const float4 vj = salva_dev_f4(v.vel, j);
            const float s = fc * v.ff_kern[4 * e + 3] * v.posm[4ull * j + 3] / v.rho[j];  // coeff W_ij m_j / rho_j
            fx += (vj.x - vi.x) * s; fy += (vj.y - vi.y) * s; fz += (vj.z - vi.z) * s;
        }
    if (bc != 0.0f) {
        const float mi = v.posm[4ull * i + 3], ri = v.rho[i];
        for (unsigned long long e = v.fb_off[i]; e < v.fb_off[i + 1]; ++e) {
            const unsigned b = v.fb_j[e];
            const float4 vb = salva_dev_f4(v.bvel, b);
            const float s = bc * v.fb_kern[4 * e + 3] * v.bposv[4ull * b + 3] * rho0 / ri;  // coeff W_ib V_b rho0 / rho_i
            const float ex = (vb.x - vi.x) * s, ey = (vb.y - vi.y) * s, ez = (vb.z - vi.z) * s;
            bx += ex; by += ey; bz += ez;
            const float fs = -mi * v.inv_dt;  // the reaction: delta * (-m_i inv_dt)
            salva_dev_boundary_add_force(v, b, ex * fs, ey * fs, ez * fs);
        }
    }
    float4* acc = reinterpret_cast<float4*>(v.acc) + i;
    float4 a = *acc;
    a.x += fx * v.inv_dt + bx * v.inv_dt; a.y += fy * v.inv_dt + by * v.inv_dt; a.z += fz * v.inv_dt + bz * v.inv_dt;
    *acc = a;
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : 1; }

}  // namespace

extern "C" int df3_field(const SalvaHipDeviceView* view) {
    if (!view || view->struct_size < sizeof(SalvaHipDeviceView) || view->version != SALVA_HIP_DEVICE_VIEW_VERSION) return 1;
    if (view->n == 0) return 0;
    k_df3_field<<<(view->n + DF3_BLOCK - 1) / DF3_BLOCK, DF3_BLOCK, 0, salva_dev_stream(view)>>>(*view);
    return launched();
}

extern "C" int df3_xsph(const SalvaHipDeviceView* view) {
    if (!view || view->struct_size < sizeof(SalvaHipDeviceView) || view->version != SALVA_HIP_DEVICE_VIEW_VERSION) return 1;
    const unsigned want = SALVA_HIP_DEVICE_NEEDS_FF | SALVA_HIP_DEVICE_NEEDS_FB | SALVA_HIP_DEVICE_NEEDS_KERNEL;
    if ((view->needs & want) != want) return 1;  // (the entry must ask for both lists and their kernel values)
    if (view->n == 0) return 0;
    k_df3_xsph<<<(view->n + DF3_BLOCK - 1) / DF3_BLOCK, DF3_BLOCK, 0, salva_dev_stream(view)>>>(*view);
    return launched();
}

#ifdef DF3_MAIN
#include <cstdio>
#include <cstdlib>

#include "../include/salva_hip.hpp"

using namespace salva;

int main(int argc, char** argv) {
    const int nsteps = argc > 1 ? atoi(argv[1]) : 200;
    const Real r = 0.025f;
    try {
        LiquidWorld world(DFSPHSolver(), r, 2.0f);
        const size_t np = 10;
        std::vector<Vec3> points;
        for (size_t i = 0; i < np; ++i)
            for (size_t j = 0; j < np; ++j)
                for (size_t k = 0; k < np; ++k)
                    points.push_back(Vec3{(Real)i * 2 * r + r - (Real)np * r, (Real)j * 2 * r + r - (Real)np * r, (Real)k * 2 * r + r - (Real)np * r});
        Fluid fluid(points, r, 1000.0f, InteractionGroups{});
        auto field = [](const SalvaHipDeviceView& v) { return df3_field(&v); };
        fluid.nonpressure_forces.push_back(std::make_shared<DeviceForce>(0u, field, std::array<Real, 6>{1.0f, 0.0f, 0.0f}));
        fluid.nonpressure_forces.push_back(std::make_shared<DeviceForce>(0u, field, std::array<Real, 6>{-1.0f, 0.0f, 0.0f}));
        const FluidHandle fh = world.add_fluid(std::move(fluid));
        const Vec3 gravity{0.0f, 0.0f, 0.0f};
        for (int s = 0; s < nsteps; ++s) {
            world.step(1.0f / 200.0f, gravity);
            if (s % 50 == 49 || s == nsteps - 1) {
                const Fluid& f = world.fluids()[fh];
                Real xmin = 1e9f, xmax = -1e9f;
                for (const Vec3& p : f.positions) { xmin = p[0] < xmin ? p[0] : xmin; xmax = p[0] > xmax ? p[0] : xmax; }
                uint64_t st[4];
                check(salva_hip_get_device_force_stats(world.handle(), st));
                printf("step %d: %zu particles, x in [%.3f, %.3f], device callbacks %llu, table builds %llu, host waits %llu\n", s + 1,
                       f.num_particles(), xmin, xmax, (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[3]);
            }
        }
    } catch (const Error& e) {
        fprintf(stderr, "salva error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
#endif

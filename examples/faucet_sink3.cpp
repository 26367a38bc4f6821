// faucet_sink3.cpp — faucet3.cpp's scene with both ends of the faucet on the device: the nozzle is a sampled shape
// (LiquidWorld::add_particles_from_shape, salva_hip_add_particles_sampled) and what leaves is taken by two sinks the world applies at the
// start of every step (salva_hip_add_sink) - a half-space below the plate and an inverted cylinder around it,
// "everything that left the tank".  No position is read inside the loop: the per-step read-back of the mirror is switched off, and the
// sink statistics say what went.  XSPHViscosity(0.5, 0.0) + Akinci2013SurfaceTension(1.0, 10.0) as in the original (faucet3.rs:37-38).
#include <cstdio>
#include <cstdlib>

#include "../include/salva_hip.hpp"

using namespace salva;

int main(int argc, char** argv) {
    const int nsteps = argc > 1 ? atoi(argv[1]) : 300;
    const Real r = 0.025f, d = 2.0f * r;
    try {
        LiquidWorld world(DFSPHSolver(), r, 2.0f);
        Fluid fluid(std::vector<Vec3>{}, r, 1000.0f, InteractionGroups{});
        fluid.nonpressure_forces.push_back(std::make_shared<XSPHViscosity>(0.5f, 0.0f));
        fluid.nonpressure_forces.push_back(std::make_shared<Akinci2013SurfaceTension>(1.0f, 10.0f));
        const FluidHandle fh = world.add_fluid(std::move(fluid));
        std::vector<Vec3> floor;  // a 1 m x 1 m plate at y = 0
        for (int i = -10; i <= 10; ++i) for (int k = -10; k <= 10; ++k) floor.push_back(Vec3{i * d, 0.0f, k * d});
        world.add_boundary(Boundary(floor));
        const SalvaHipShape nozzle{SALVA_HIP_SHAPE_CUBOID, {5.0f * r, 0.5f * r, 5.0f * r}};  // one layer of particles: it has fallen a spacing when the next one comes
        const Vec3 nozzle_at{0.0f, 0.6f, 0.0f}, nozzle_vel{0.0f, -1.0f, 0.0f}, gravity{0.0f, -9.81f, 0.0f};
        // what fell below y = -0.3, and what left the cylinder of radius 1 around the y axis
        const SinkHandle below = world.add_sink(Region::half_space(Vec3{0.0f, -0.3f, 0.0f}, Vec3{0.0f, 1.0f, 0.0f}), fh);
        const SalvaHipShape well{SALVA_HIP_SHAPE_CYLINDER, {10.0f, 1.0f, 0.0f}};
        const SinkHandle around = world.add_sink(Region::shape(well, Vec3{0.0f, 0.0f, 0.0f}, {0, 0, 0, 1}, 0.0f, /*invert=*/true), fh);
        world.set_readback(false);
        size_t added = 0;
        for (int s = 0; s < nsteps; ++s) {
            if (s % 10 == 0) added += world.add_particles_from_shape(fh, nozzle, nozzle_at, {0, 0, 0, 1}, SALVA_HIP_SAMPLE_VOLUME, &nozzle_vel);
            world.step(1.0f / 200.0f, gravity);
            if (s % 100 == 99 || s == nsteps - 1)
                printf("step %d: %zu particles (added %zu, sinks took %llu below and %llu around), %d div / %d pressure iterations\n", s + 1,
                       world.fluids()[fh].num_particles(), added, (unsigned long long)world.sink_stats(below)[1],
                       (unsigned long long)world.sink_stats(around)[1], world.counters().n_divergence_iters, world.counters().n_pressure_iters);
        }
        world.refresh(fh);  // once, after the loop
        Real ymin = 1e9f, ymax = -1e9f;
        for (const Vec3& p : world.fluids()[fh].positions) { ymin = p[1] < ymin ? p[1] : ymin; ymax = p[1] > ymax ? p[1] : ymax; }
        printf("y in [%.3f, %.3f]\n", ymin, ymax);
    } catch (const Error& e) {
        fprintf(stderr, "salva_hip error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}

// foam3.cpp — whitewater on a dam break: the basic3 block (examples/basic3.cpp: 15^3 particles, r = 0.05, lattice plates for the ground
// and the walls) with DFSPH + XSPHViscosity, and a set of diffuse particles that lives on the device (LiquidWorld::create_diffuse;
// DESIGN.md §24): after every step one update advects and ages the spray, foam and bubbles there are, removes the dissolved ones and
// emits new ones where the fluid traps air, breaks or moves fast.  The scene is small and slow, so the clamps are lower than Ihmsen's
// defaults.  Prints the counts per kind and the totals.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../include/salva_hip.hpp"

using namespace salva;

static const Real PARTICLE_RADIUS = 0.05f, SMOOTHING_FACTOR = 2.0f;

// examples3d/helper.rs:4-20
static Fluid cube_fluid(size_t ni, size_t nj, size_t nk, Real particle_rad, Real density) {
    std::vector<Vec3> points;
    const Vec3 half_extents{(Real)ni * particle_rad, (Real)nj * particle_rad, (Real)nk * particle_rad};
    for (size_t i = 0; i < ni; ++i)
        for (size_t j = 0; j < nj; ++j)
            for (size_t k = 0; k < nk; ++k) {
                const Real x = (Real)i * particle_rad * 2.0f, y = (Real)j * particle_rad * 2.0f, z = (Real)k * particle_rad * 2.0f;
                points.push_back(Vec3{x + particle_rad - half_extents[0], y + particle_rad - half_extents[1],
                                      z + particle_rad - half_extents[2]});
            }
    return Fluid(points, particle_rad, density, InteractionGroups{});
}

static std::vector<Vec3> plate(Real x0, Real x1, Real y0, Real y1, Real z0, Real z1) {  // lattice points of a box region
    std::vector<Vec3> pts;
    const Real d = 2.0f * PARTICLE_RADIUS;
    for (Real x = x0; x <= x1 + 1e-4f; x += d)
        for (Real y = y0; y <= y1 + 1e-4f; y += d)
            for (Real z = z0; z <= z1 + 1e-4f; z += d) pts.push_back(Vec3{x, y, z});
    return pts;
}

int main(int argc, char** argv) {
    const int nsteps = argc > 1 ? atoi(argv[1]) : 60;
    try {
        LiquidWorld world(DFSPHSolver(), PARTICLE_RADIUS, SMOOTHING_FACTOR);
        const Real ground_thickness = 0.2f, ground_half_width = 2.5f, ground_half_height = 0.7f;
        const size_t nparticles = 15;
        Fluid fluid = cube_fluid(nparticles, nparticles, nparticles, PARTICLE_RADIUS, 1000.0f);
        fluid.transform_by(Vec3{0.0f, ground_thickness + (Real)nparticles * PARTICLE_RADIUS, 0.0f});
        fluid.nonpressure_forces.push_back(std::make_shared<XSPHViscosity>(0.5f, 0.0f));
        world.add_fluid(std::move(fluid));
        const Real w = ground_half_width;
        world.add_boundary(Boundary(plate(-w, w, ground_thickness, ground_thickness, -w, w)));
        world.add_boundary(Boundary(plate(-w, w, ground_thickness, 2 * ground_half_height, w, w)));
        world.add_boundary(Boundary(plate(-w, w, ground_thickness, 2 * ground_half_height, -w, -w)));
        world.add_boundary(Boundary(plate(w, w, ground_thickness, 2 * ground_half_height, -w, w)));
        world.add_boundary(Boundary(plate(-w, -w, ground_thickness, 2 * ground_half_height, -w, w)));
        const Vec3 gravity{0.0f, -9.81f, 0.0f};
        Diffuse params;
        params.ta_lo = 1.0f; params.ta_hi = 10.0f; params.wc_lo = 0.5f; params.wc_hi = 4.0f; params.en_lo = 0.1f; params.en_hi = 2.0f;
        params.k_ta = 200.0f; params.k_wc = 2000.0f; params.max_per_particle = 4; params.seed = 3;
        params.gravity = gravity;
        const DiffuseHandle set = world.create_diffuse(20000);
        const Real dt = 1.0f / 200.0f;
        for (int s = 0; s < nsteps; ++s) {
            world.step(dt, gravity);
            world.update_diffuse(set, params, dt);
        }
        const SalvaHipDiffuseStats st = world.diffuse_stats(set);
        printf("after %d steps: %llu diffuse particles: spray %llu, foam %llu, bubbles %llu, new %llu\n", nsteps, (unsigned long long)st.count,
               (unsigned long long)st.kinds[0], (unsigned long long)st.kinds[1], (unsigned long long)st.kinds[2], (unsigned long long)st.kinds[3]);
        printf("emitted %llu, dissolved %llu, killed %llu, dropped %llu\n", (unsigned long long)st.total_emitted, (unsigned long long)st.total_dissolved,
               (unsigned long long)st.total_killed, (unsigned long long)st.total_dropped);
    } catch (const Error& e) {
        fprintf(stderr, "salva error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}

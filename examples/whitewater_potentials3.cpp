// whitewater_potentials3.cpp — where a dam break would make whitewater: the basic3 block (examples/basic3.cpp: 15^3 particles, r = 0.05,
// lattice plates for the ground and the walls) with DFSPH + XSPHViscosity, and after every step the potentials of diffuse particles
// read out on the device (LiquidWorld::diffuse_potentials).  Prints, for the last step, how many particles have a surface
// normal, how many sit on a breaking crest and how many trap air or move fast enough to pass the lower ends of Ihmsen's clamp ranges
// (5 for both) — what an emitter of spray, foam and bubbles starts from.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../include/salva_hip.hpp"

using namespace salva;

static const Real PARTICLE_RADIUS = 0.05f, SMOOTHING_FACTOR = 2.0f;
static const Real TRAPPED_AIR_MIN = 5.0f, ENERGY_MIN = 5.0f;  // Ihmsen et al. 2012: below these a particle emits nothing

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
    const int nsteps = argc > 1 ? atoi(argv[1]) : 50;
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
        const Diffuse params;  // salva_hip_default_diffuse
        DiffusePotentials p;
        for (int s = 0; s < nsteps; ++s) {
            world.step(1.0f / 200.0f, gravity);
            p = world.diffuse_potentials(params);
        }
        size_t normals = 0, crests = 0, trapping = 0, fast = 0;
        uint32_t most = 0;
        for (size_t i = 0; i < p.count.size(); ++i) {
            normals += (p.normal[3 * i] != 0.0f || p.normal[3 * i + 1] != 0.0f || p.normal[3 * i + 2] != 0.0f) ? 1 : 0;
            crests += p.wave_crest[i] > 0.0f ? 1 : 0;
            trapping += p.trapped_air[i] > TRAPPED_AIR_MIN ? 1 : 0;
            fast += p.energy[i] > ENERGY_MIN ? 1 : 0;
            most = p.count[i] > most ? p.count[i] : most;
        }
        printf("%zu particles after %d steps; at most %u neighbours\n", p.count.size(), nsteps, most);
        printf("with a normal: %zu; on a crest: %zu; trapped air above %.1f: %zu; energy above %.1f: %zu\n", normals, crests, TRAPPED_AIR_MIN, trapping,
               ENERGY_MIN, fast);
    } catch (const Error& e) {
        fprintf(stderr, "salva error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}

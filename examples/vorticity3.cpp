// vorticity3.cpp — vorticity confinement on a vortex column: a block of 12^3 particles (r = 0.025) is given the
// velocities of a Lamb-Oseen vortex along y, v_theta = Gamma / (2 pi r) (1 - exp(-r^2 / r_c^2)), and stepped without gravity and
// without boundaries, once with VorticityConfinement(strength) and once with VorticityConfinement(0): that entry adds no force and
// exists to read the vorticity out (LiquidWorld::vorticity).  Prints the enstrophy sum_i m_i |omega_i|^2 of the last step for both
// runs: what XSPH, the pressure solve and the kernel's support take from the column, and how much of it the force keeps.
//   vorticity3 [steps = 50] [strength = 0.1]
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../include/salva_hip.hpp"

using namespace salva;

static const Real PARTICLE_RADIUS = 0.025f, SMOOTHING_FACTOR = 2.0f, DENSITY = 1000.0f;
static const double GAMMA = 0.5, CORE = 0.1;
static const size_t N = 12;

// examples3d/helper.rs:4-20
static std::vector<Vec3> cube_points(size_t ni, size_t nj, size_t nk, Real particle_rad) {
    std::vector<Vec3> points;
    const Vec3 half_extents{(Real)ni * particle_rad, (Real)nj * particle_rad, (Real)nk * particle_rad};
    for (size_t i = 0; i < ni; ++i)
        for (size_t j = 0; j < nj; ++j)
            for (size_t k = 0; k < nk; ++k) {
                const Real x = (Real)i * particle_rad * 2.0f, y = (Real)j * particle_rad * 2.0f, z = (Real)k * particle_rad * 2.0f;
                points.push_back(Vec3{x + particle_rad - half_extents[0], y + particle_rad - half_extents[1],
                                      z + particle_rad - half_extents[2]});
            }
    return points;
}

static double enstrophy_after(int nsteps, Real strength) {
    LiquidWorld world(DFSPHSolver(), PARTICLE_RADIUS, SMOOTHING_FACTOR);
    Fluid fluid(cube_points(N, N, N, PARTICLE_RADIUS), PARTICLE_RADIUS, DENSITY, InteractionGroups{});
    for (size_t i = 0; i < fluid.positions.size(); ++i) {  // the column's axis is the y axis (the block is centred on the origin)
        const double dx = fluid.positions[i][0], dz = fluid.positions[i][2], r2 = dx * dx + dz * dz;
        const double swirl = r2 > 0.0 ? GAMMA / (2.0 * M_PI * r2) * -std::expm1(-r2 / (CORE * CORE)) : 0.0;  // v_theta / r
        fluid.velocities[i] = Vec3{(Real)(swirl * dz), 0.0f, (Real)(-swirl * dx)};
    }
    fluid.nonpressure_forces.push_back(std::make_shared<XSPHViscosity>(0.5f, 0.0f));
    fluid.nonpressure_forces.push_back(std::make_shared<VorticityConfinement>(strength));
    const double mass = (double)fluid.volumes[0] * (double)DENSITY;
    const FluidHandle h = world.add_fluid(std::move(fluid));
    const Vec3 gravity{0.0f, 0.0f, 0.0f};
    for (int s = 0; s < nsteps; ++s) world.step(1.0f / 200.0f, gravity);
    double e = 0.0;
    for (const Vec3& w : world.vorticity(h)) e += mass * ((double)w[0] * w[0] + (double)w[1] * w[1] + (double)w[2] * w[2]);
    return e;
}

int main(int argc, char** argv) {
    const int nsteps = argc > 1 ? atoi(argv[1]) : 50;
    const Real strength = argc > 2 ? (Real)atof(argv[2]) : 0.1f;
    try {
        const double with = enstrophy_after(nsteps, strength), without = enstrophy_after(nsteps, 0.0f);
        printf("%zu particles, %d steps, strength %g\n", N * N * N, nsteps, (double)strength);
        printf("enstrophy with the force: %.9g; without: %.9g\n", with, without);
    } catch (const Error& e) {
        fprintf(stderr, "salva error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}

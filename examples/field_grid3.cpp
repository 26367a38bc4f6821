// field_grid3.cpp — the fluid as a continuum: the basic3 block (examples/basic3.cpp: 15^3 particles, r = 0.05, lattice plates for the
// ground and the walls) with DFSPH + XSPHViscosity, 50 steps, then the volume fraction sum_j V_j W on a voxel lattice at spacing r over
// the fluid's box grown by 4 r, summed on the device (LiquidWorld::evaluate_lattice).  Prints how many nodes hold more
// than half fluid and how high they reach — what an iso-surface extractor or a fill-level sensor starts from.
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
    const int nsteps = argc > 1 ? atoi(argv[1]) : 50;
    try {
        LiquidWorld world(DFSPHSolver(), PARTICLE_RADIUS, SMOOTHING_FACTOR);
        const Real ground_thickness = 0.2f, ground_half_width = 2.5f, ground_half_height = 0.7f;
        const size_t nparticles = 15;
        Fluid fluid = cube_fluid(nparticles, nparticles, nparticles, PARTICLE_RADIUS, 1000.0f);
        fluid.transform_by(Vec3{0.0f, ground_thickness + (Real)nparticles * PARTICLE_RADIUS, 0.0f});
        fluid.nonpressure_forces.push_back(std::make_shared<XSPHViscosity>(0.5f, 0.0f));
        const FluidHandle fh = world.add_fluid(std::move(fluid));
        const Real w = ground_half_width;
        world.add_boundary(Boundary(plate(-w, w, ground_thickness, ground_thickness, -w, w)));
        world.add_boundary(Boundary(plate(-w, w, ground_thickness, 2 * ground_half_height, w, w)));
        world.add_boundary(Boundary(plate(-w, w, ground_thickness, 2 * ground_half_height, -w, -w)));
        world.add_boundary(Boundary(plate(w, w, ground_thickness, 2 * ground_half_height, -w, w)));
        world.add_boundary(Boundary(plate(-w, -w, ground_thickness, 2 * ground_half_height, -w, w)));
        const Vec3 gravity{0.0f, -9.81f, 0.0f};
        for (int s = 0; s < nsteps; ++s) world.step(1.0f / 200.0f, gravity);
        // the lattice: the fluid's box grown by 4 r, spacing r
        const Fluid& f = world.fluids()[fh];
        Vec3 lo{1e9f, 1e9f, 1e9f}, hi{-1e9f, -1e9f, -1e9f};
        for (const Vec3& p : f.positions)
            for (int a = 0; a < 3; ++a) { lo[a] = p[a] < lo[a] ? p[a] : lo[a]; hi[a] = p[a] > hi[a] ? p[a] : hi[a]; }
        const Real r = PARTICLE_RADIUS, margin = 4.0f * r;
        std::array<uint32_t, 3> dims;
        for (int a = 0; a < 3; ++a) {
            lo[a] = lo[a] - margin;
            const Real top = hi[a] + margin;
            dims[a] = (uint32_t)std::floor((top - lo[a]) / r) + 1u;
        }
        const LiquidWorld::Fields fields = world.evaluate_lattice(lo, r, dims, LiquidWorld::FieldSet::FRACTION);
        size_t above = 0;
        long top_row = -1;
        for (uint32_t ix = 0; ix < dims[0]; ++ix)
            for (uint32_t iy = 0; iy < dims[1]; ++iy)
                for (uint32_t iz = 0; iz < dims[2]; ++iz)
                    if (fields.fraction[((size_t)ix * dims[1] + iy) * dims[2] + iz] > 0.5f) {
                        ++above;
                        if ((long)iy > top_row) top_row = (long)iy;
                    }
        const Real height = top_row < 0 ? NAN : lo[1] + (Real)top_row * r;
        printf("lattice %u x %u x %u at spacing %.3f after %d steps\n", dims[0], dims[1], dims[2], r, nsteps);
        printf("nodes above 0.5: %zu of %zu; fill height %.6f\n", above, fields.fraction.size(), height);
    } catch (const Error& e) {
        fprintf(stderr, "salva error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}

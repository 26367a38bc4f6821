// heightfield3.cpp — a block of fluid thrown onto a height field: the one 3D scene of salva's examples whose collider is not a
// primitive.  The height field lives on the device as a triangle mesh (salva::Mesh::heightfield); its surface is
// ray-sampled there (sampling::shape_surface_ray_sample) and registered as a StaticSampling boundary.  Scene: 15^3 particles of
// radius 0.15 falling at 10 m/s, ArtificialViscosity(1, 0), a 41 x 41 height field of size 12 x 1 x 12 with a rim of height 3,
// sampled at r / 1.5, dt = 1 / 200.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../include/salva_hip.hpp"

using namespace salva;

int main(int argc, char** argv) {
    const int nsteps = argc > 1 ? atoi(argv[1]) : 200;
    const Real r = 0.15f, dt = 1.0f / 200.0f;
    try {
        LiquidWorld world(DFSPHSolver(), r, 2.0f);
        // the fluid
        const int n = 15;
        std::vector<Vec3> block;
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) for (int k = 0; k < n; ++k)
            block.push_back(Vec3{(i - n / 2) * 2.0f * r, 5.0f + j * 2.0f * r, (k - n / 2) * 2.0f * r});
        Fluid fluid(block, r, 1000.0f, InteractionGroups{});
        fluid.velocities.assign(block.size(), Vec3{0.0f, -10.0f, 0.0f});
        fluid.nonpressure_forces.push_back(std::make_shared<ArtificialViscosity>(1.0f, 0.0f));
        const FluidHandle fh = world.add_fluid(std::move(fluid));
        // the ground: gentle waves inside, a rim that keeps the fluid in
        const uint32_t rows = 41, cols = 41;
        std::vector<Real> heights(rows * cols);
        for (uint32_t i = 0; i < rows; ++i) for (uint32_t j = 0; j < cols; ++j) {
            const bool rim = i == 0 || j == 0 || i == rows - 1 || j == cols - 1;
            heights[i * cols + j] = rim ? 3.0f : 0.5f * (std::sin(0.6f * (float)i) + std::cos(0.45f * (float)j)) + 1.0f;
        }
        Mesh ground = Mesh::heightfield(world, heights, rows, cols, Vec3{12.0f, 1.0f, 12.0f});
        Boundary b(std::vector<Vec3>{});
        b.sampling = sampling::shape_surface_ray_sample(world, ground, r / 1.5f);
        const size_t nsamples = b.sampling.size();
        const BoundaryHandle bh = world.add_boundary(std::move(b));
        ColliderCouplingSet coupling;
        coupling.register_coupling(bh, [] { SalvaHipRigidPose p{}; p.rotation[3] = 1.0f; return p; });
        printf("%zu fluid particles, %zu boundary samples\n", block.size(), nsamples);
        const Vec3 gravity{0.0f, -9.81f, 0.0f};
        for (int s = 0; s < nsteps; ++s) world.step_with_coupling(dt, gravity, coupling);
        Vec3 lo{1e30f, 1e30f, 1e30f}, hi{-1e30f, -1e30f, -1e30f};
        for (const Vec3& p : world.fluids()[fh].positions)
            for (int a = 0; a < 3; ++a) { lo[a] = p[a] < lo[a] ? p[a] : lo[a]; hi[a] = p[a] > hi[a] ? p[a] : hi[a]; }
        printf("fluid bounding box after %d steps: [%.4f, %.4f, %.4f] - [%.4f, %.4f, %.4f]\n", nsteps, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
    } catch (const Error& e) {
        fprintf(stderr, "salva_hip error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}

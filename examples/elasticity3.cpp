// elasticity3.cpp — /root/reference/examples3d/elasticity3.rs without the viewer: two elastic blocks (12 x 6 x 12 particles,
// Becker2009Elasticity with E = 5e5 and 1e5, nu = 0.3, nonlinear strain, plus XSPHViscosity(0.5, 1.0)) fall onto a fixed cuboid
// ground (half extents 1.5, 0.2, 1.5) whose boundary particles come from DynamicContactSampling.  Prints each block's bounding
// box every 50 steps: the blocks land, bounce and keep their shape.
#include <cstdio>
#include <cstdlib>

#include "../include/salva_hip.hpp"

using namespace salva;

static Fluid cube_fluid(int ni, int nj, int nk, Real r, Real density, Real ty) {  // examples3d/helper.rs cube_fluid + transform_by
    std::vector<Vec3> pts;
    for (int i = 0; i < ni; ++i) for (int j = 0; j < nj; ++j) for (int k = 0; k < nk; ++k)
        pts.push_back(Vec3{i * r * 2.0f + r - ni * r, j * r * 2.0f + r - nj * r + ty, k * r * 2.0f + r - nk * r});
    return Fluid(pts, r, density, InteractionGroups{});
}

int main(int argc, char** argv) {
    const int nsteps = argc > 1 ? atoi(argv[1]) : 300;
    const Real r = 0.025f, dt = 1.0f / 200.0f;
    const Real ground_thickness = 0.2f, ground_half_width = 1.5f, height = 0.4f;
    const int np = 6;
    try {
        LiquidWorld world(DFSPHSolver(), r, 2.0f);
        FluidHandle blocks[2];
        const Real young[2] = {500000.0f, 100000.0f};
        const Real lift[2] = {1.0f, 4.0f};
        for (int b = 0; b < 2; ++b) {
            Fluid fluid = cube_fluid(np * 2, np, np * 2, r, 1000.0f, ground_thickness + r * np * lift[b] + height);
            fluid.nonpressure_forces.push_back(std::make_shared<Becker2009Elasticity>(young[b], 0.3f, true));
            fluid.nonpressure_forces.push_back(std::make_shared<XSPHViscosity>(0.5f, 1.0f));
            blocks[b] = world.add_fluid(std::move(fluid));
        }
        const BoundaryHandle ground = world.add_boundary(Boundary::dynamic_cuboid(Vec3{ground_half_width, ground_thickness, ground_half_width}));
        ColliderCouplingSet coupling;  // RigidBodyBuilder::fixed(): the ground never moves, the reaction impulses go nowhere
        coupling.register_coupling(ground, [] { SalvaHipRigidPose p{}; p.rotation[3] = 1.0f; p.has_body = 1; return p; },
                                   [](const Vec3&, const Vec3&) {});
        const Vec3 gravity{0.0f, -9.81f, 0.0f};
        for (int s = 0; s < nsteps; ++s) {
            world.step_with_coupling(dt, gravity, coupling);
            if (s % 50 == 49 || s == nsteps - 1) {
                printf("step %d:", s + 1);
                for (int b = 0; b < 2; ++b) {
                    const Fluid& f = world.fluids()[blocks[b]];
                    Vec3 lo{1e9f, 1e9f, 1e9f}, hi{-1e9f, -1e9f, -1e9f};
                    for (const Vec3& p : f.positions)
                        for (int k = 0; k < 3; ++k) { lo[k] = p[k] < lo[k] ? p[k] : lo[k]; hi[k] = p[k] > hi[k] ? p[k] : hi[k]; }
                    printf("  block %d [%.3f %.3f %.3f]..[%.3f %.3f %.3f]", b, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
                }
                printf("\n");
            }
        }
    } catch (const Error& e) {
        fprintf(stderr, "salva_hip error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}

// compound_sampling3.cpp — the open box of compound3.cpp as a static container: its five slabs are ray-sampled on the device
// (Boundary::sampled_from_shape(compound): ColliderSampling::StaticSampling(shape_surface_ray_sample(&compound, r)) without the points
// visiting the host) and the fluid poured into it is the volume sample of a second compound, a ball resting on a rotated cuboid
// (LiquidWorld::add_particles_from_shape(compound): fluid.add_particles(&shape_volume_ray_sample(..))).  DESIGN.md §17 "Ray sampling".
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../include/salva_hip.hpp"

using namespace salva;

int main(int argc, char** argv) {
    const int nsteps = argc > 1 ? atoi(argv[1]) : 200;
    const Real r = 0.025f, d = 2.0f * r, dt = 1.0f / 200.0f;
    try {
        LiquidWorld world(DFSPHSolver(), r, 2.0f);
        Fluid fluid(std::vector<Vec3>{}, r, 1000.0f, InteractionGroups{});
        fluid.nonpressure_forces.push_back(std::make_shared<ArtificialViscosity>(1.0f, 0.5f));
        const FluidHandle fh = world.add_fluid(std::move(fluid));
        // the open box: outer half width `half`, slabs of half thickness `wall`, walls of half height `hh` standing on the floor slab
        const Real half = 8.0f * d, wall = 0.4f * d, hh = 5.0f * d;
        const SalvaHipShape floor_slab{SALVA_HIP_SHAPE_CUBOID, {half, wall, half}}, wall_x{SALVA_HIP_SHAPE_CUBOID, {wall, hh, half}},
            wall_z{SALVA_HIP_SHAPE_CUBOID, {half, hh, wall}};
        Compound box(world, {Compound::Part(floor_slab, Vec3{0, -hh, 0}), Compound::Part(wall_x, Vec3{-(half - wall), wall, 0}),
                             Compound::Part(wall_x, Vec3{half - wall, wall, 0}), Compound::Part(wall_z, Vec3{0, wall, -(half - wall)}),
                             Compound::Part(wall_z, Vec3{0, wall, half - wall})});
        const BoundaryHandle bh = world.add_boundary(Boundary::sampled_from_shape(box));
        ColliderCouplingSet coupling;
        coupling.register_coupling(bh, [] { SalvaHipRigidPose p{}; p.rotation[3] = 1.0f; return p; });
        // what is poured in: a ball on a cuboid turned by 0.5 rad about z
        const SalvaHipShape ball{SALVA_HIP_SHAPE_BALL, {4.0f * d, 0, 0}}, brick{SALVA_HIP_SHAPE_CUBOID, {5.0f * d, 2.0f * d, 4.0f * d}};
        Compound drop(world, {Compound::Part(brick, Vec3{0, 0, 0}, {0.0f, 0.0f, std::sin(0.25f), std::cos(0.25f)}), Compound::Part(ball, Vec3{0, 5.0f * d, 0})});
        const Vec3 down{0.0f, -1.0f, 0.0f};
        const size_t poured = world.add_particles_from_shape(fh, drop, Vec3{0.0f, 2.0f * d, 0.0f}, {0, 0, 0, 1}, SALVA_HIP_SAMPLE_VOLUME, &down);
        const size_t surface = sampling::shape_surface_ray_sample(world, box, r).size();
        const Vec3 gravity{0.0f, -9.81f, 0.0f};
        for (int s = 0; s < nsteps; ++s) {
            world.step_with_coupling(dt, gravity, coupling);
            if (s % 50 == 49 || s == nsteps - 1) {
                int inside = 0;
                Real lowest = 1e30f;
                for (const Vec3& p : world.fluids()[fh].positions) {
                    if (std::fabs(p[0]) < half && std::fabs(p[2]) < half && p[1] > -hh - wall) ++inside;  // within the walls, above the floor's underside
                    lowest = std::fmin(lowest, p[1]);
                }
                printf("step %d: %zu fluid particles poured, %d in the box, lowest y %.4f (floor top %.4f); %zu boundary samples (%zu sampled to the host)\n",
                       s + 1, poured, inside, lowest, -hh + wall, world.boundaries()[bh].num_particles(), surface);
            }
        }
    } catch (const Error& e) {
        fprintf(stderr, "salva_hip error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}

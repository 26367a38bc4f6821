// compound3.cpp — dynamic_coupling3.cpp with a compound collider: the dynamic body is an open box made of five cuboid slabs (a floor
// and four walls), which is what a non-primitive dynamic body usually is in rapier — a `Compound` of simple parts.  The box is
// dropped into a pool from just above its surface, as the ball of dynamic_coupling3.cpp is; its slabs are lighter than the fluid they
// displace, so it ends up floating, with whatever fluid came over its rim inside it.  All five parts are projected onto on the device (salva_hip_create_compound,
// salva_hip_set_boundary_dynamic_sampling_compound): per step the coupling sends one pose and receives one wrench.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../include/salva_hip.hpp"

using namespace salva;

struct Body {  // the slice of rapier's RigidBody the coupling touches
    Vec3 translation{0, 0, 0}, linvel{0, 0, 0}, angvel{0, 0, 0};
    Real mass = 1.0f, inertia = 1.0f;  // isotropic inertia: no frame change needed for the torque impulse
    SalvaHipRigidPose pose() const {
        SalvaHipRigidPose p{};
        for (int k = 0; k < 3; ++k) { p.translation[k] = translation[k]; p.linvel[k] = linvel[k]; p.angvel[k] = angvel[k]; p.world_com[k] = translation[k]; }
        p.rotation[3] = 1.0f;  // the example keeps the box axis aligned (small angular velocities are only reported)
        p.has_body = 1; p.is_dynamic = 1;
        return p;
    }
};

int main(int argc, char** argv) {
    const int nsteps = argc > 1 ? atoi(argv[1]) : 200;
    const Real r = 0.025f, d = 2.0f * r, dt = 1.0f / 200.0f;
    try {
        LiquidWorld world(DFSPHSolver(), r, 2.0f);
        std::vector<Vec3> pool, shell;
        const int nx = 16, ny = 8, nz = 16;
        for (int i = 0; i < nx; ++i) for (int j = 0; j < ny; ++j) for (int k = 0; k < nz; ++k)
            pool.push_back(Vec3{(i - nx / 2) * d + r, j * d + r + d, (k - nz / 2) * d + r});
        for (int i = -1; i <= nx; ++i) for (int j = 0; j <= ny + 6; ++j) for (int k = -1; k <= nz; ++k)
            if (i == -1 || i == nx || j == 0 || k == -1 || k == nz) shell.push_back(Vec3{(i - nx / 2) * d + r, j * d + r, (k - nz / 2) * d + r});
        Fluid fluid(pool, r, 1000.0f, InteractionGroups{});
        fluid.nonpressure_forces.push_back(std::make_shared<ArtificialViscosity>(1.0f, 0.5f));
        const FluidHandle fh = world.add_fluid(std::move(fluid));
        world.add_boundary(Boundary(shell));
        // the open box: outer half width `half`, slabs of half thickness `wall`, walls of half height `hh` standing on the floor slab
        const Real half = 3.0f * d, wall = 0.4f * d, hh = 1.6f * d;
        const SalvaHipShape floor_slab{SALVA_HIP_SHAPE_CUBOID, {half, wall, half}}, wall_x{SALVA_HIP_SHAPE_CUBOID, {wall, hh, half}},
            wall_z{SALVA_HIP_SHAPE_CUBOID, {half, hh, wall}};
        Compound box(world, {Compound::Part(floor_slab, Vec3{0, -hh, 0}), Compound::Part(wall_x, Vec3{-(half - wall), wall, 0}),
                             Compound::Part(wall_x, Vec3{half - wall, wall, 0}), Compound::Part(wall_z, Vec3{0, wall, -(half - wall)}),
                             Compound::Part(wall_z, Vec3{0, wall, half - wall})});
        const BoundaryHandle bh = world.add_boundary(Boundary::dynamic_compound(box));
        Body body;
        const Real pool_top = (ny + 1) * d;
        body.translation = Vec3{0.0f, pool_top + hh + 2.0f * wall + d, 0.0f};  // the underside of the floor slab one particle diameter above the pool
        const Real slab_volume = 8.0f * (half * wall * half + 2.0f * wall * hh * half + 2.0f * half * hh * wall);
        body.mass = 0.6f * 1000.0f * slab_volume;  // 0.6 of the density of the fluid
        body.inertia = 0.5f * body.mass * half * half;
        Vec3 force{0, 0, 0}, torque{0, 0, 0};
        ColliderCouplingSet coupling;
        coupling.register_coupling(bh, [&] { return body.pose(); }, [&](const Vec3& j, const Vec3& tj) {
            for (int k = 0; k < 3; ++k) {
                body.linvel[k] += j[k] / body.mass; body.angvel[k] += tj[k] / body.inertia;
                force[k] = j[k] / dt; torque[k] = tj[k] / dt;
            }
        });
        const Vec3 gravity{0.0f, -9.81f, 0.0f};
        for (int s = 0; s < nsteps; ++s) {
            world.step_with_coupling(dt, gravity, coupling);
            for (int k = 0; k < 3; ++k) { body.linvel[k] += gravity[k] * dt; body.translation[k] += body.linvel[k] * dt; }
            if (s % 50 == 49 || s == nsteps - 1) {
                world.sync_boundary(bh);
                int inside = 0;  // fluid particles in the box's cavity
                for (const Vec3& p : world.fluids()[fh].positions) {
                    const Real x = p[0] - body.translation[0], y = p[1] - body.translation[1], z = p[2] - body.translation[2];
                    if (std::fabs(x) < half - 2.0f * wall && std::fabs(z) < half - 2.0f * wall && y > -hh + wall && y < hh + wall) ++inside;
                }
                uint64_t dcs[4] = {0, 0, 0, 0};
                check(salva_hip_get_dcs_stats(world.handle(), dcs));
                printf("step %d: box y %.4f vy %.4f, force (%.3f, %.3f, %.3f) torque (%.4f, %.4f, %.4f), weight %.3f, %zu samples, %d fluid particles inside, "
                       "dcs passes %llu waits %llu batched %llu records %llu\n",
                       s + 1, body.translation[1], body.linvel[1], force[0], force[1], force[2], torque[0], torque[1], torque[2], body.mass * 9.81f,
                       world.boundaries()[bh].num_particles(), inside, (unsigned long long)dcs[0], (unsigned long long)dcs[1],
                       (unsigned long long)dcs[2], (unsigned long long)dcs[3]);
            }
        }
    } catch (const Error& e) {
        fprintf(stderr, "salva_hip error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}

// many_bodies3.cpp — dynamic_coupling3.cpp with many bodies: a 3 x 3 raft of half-density balls dropped on a pool, every one of them
// coupled by ColliderSampling::DynamicContactSampling.  Their boundaries sit in consecutive slots, so every step samples all nine in
// ONE pass over the fluid (salva_hip_get_dcs_stats), and the coupling set sends all poses with one call and receives all wrenches
// with one (salva_hip_update_boundary_poses / salva_hip_get_boundary_wrenches).
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
        p.rotation[3] = 1.0f;
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
        const int nx = 20, ny = 8, nz = 20;
        for (int i = 0; i < nx; ++i) for (int j = 0; j < ny; ++j) for (int k = 0; k < nz; ++k)
            pool.push_back(Vec3{(i - nx / 2) * d + r, j * d + r + d, (k - nz / 2) * d + r});
        for (int i = -1; i <= nx; ++i) for (int j = 0; j <= ny + 6; ++j) for (int k = -1; k <= nz; ++k)
            if (i == -1 || i == nx || j == 0 || k == -1 || k == nz) shell.push_back(Vec3{(i - nx / 2) * d + r, j * d + r, (k - nz / 2) * d + r});
        Fluid fluid(pool, r, 1000.0f, InteractionGroups{});
        fluid.nonpressure_forces.push_back(std::make_shared<ArtificialViscosity>(1.0f, 0.5f));
        const FluidHandle fh = world.add_fluid(std::move(fluid));
        world.add_boundary(Boundary(shell));
        const Real ball_radius = 1.5f * d;
        constexpr int NB = 9;
        std::vector<Body> bodies(NB);
        std::vector<BoundaryHandle> handles;
        ColliderCouplingSet coupling;
        for (int b = 0; b < NB; ++b) {
            handles.push_back(world.add_boundary(Boundary::dynamic_ball(ball_radius)));
            Body& body = bodies[b];
            body.translation = Vec3{(b % 3 - 1) * 5.0f * d, (ny + 4 + b % 2) * d, (b / 3 - 1) * 5.0f * d};
            body.mass = 0.5f * 1000.0f * 4.18879f * ball_radius * ball_radius * ball_radius;  // half the density of the fluid
            body.inertia = 0.4f * body.mass * ball_radius * ball_radius;
            coupling.register_coupling(handles[b], [&body] { return body.pose(); }, [&body](const Vec3& j, const Vec3& tj) {
                for (int k = 0; k < 3; ++k) { body.linvel[k] += j[k] / body.mass; body.angvel[k] += tj[k] / body.inertia; }
            });
        }
        const Vec3 gravity{0.0f, -9.81f, 0.0f};
        for (int s = 0; s < nsteps; ++s) {
            world.step_with_coupling(dt, gravity, coupling);
            for (Body& body : bodies)
                for (int k = 0; k < 3; ++k) { body.linvel[k] += gravity[k] * dt; body.translation[k] += body.linvel[k] * dt; }
            if (s % 50 == 49 || s == nsteps - 1) {
                Real ysum = 0.0f, vysum = 0.0f, ylow = 1e9f;
                size_t samples = 0;
                for (int b = 0; b < NB; ++b) {
                    world.sync_boundary(handles[b]);
                    samples += world.boundaries()[handles[b]].num_particles();
                    ysum += bodies[b].translation[1]; vysum += bodies[b].linvel[1];
                    ylow = bodies[b].translation[1] < ylow ? bodies[b].translation[1] : ylow;
                }
                uint64_t dcs[4] = {0, 0, 0, 0};
                world.dcs_stats(dcs);
                printf("step %d: mean ball y %.4f vy %.4f, lowest ball y %.4f, %zu samples, dcs passes %llu waits %llu batched %llu, fluid %zu particles\n",
                       s + 1, ysum / NB, vysum / NB, ylow, samples, (unsigned long long)dcs[0], (unsigned long long)dcs[1],
                       (unsigned long long)dcs[2], world.fluids()[fh].num_particles());
            }
        }
    } catch (const Error& e) {
        fprintf(stderr, "salva_hip error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}

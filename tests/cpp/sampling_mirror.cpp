// The C++ mirror's ray sampler calls (include/salva_hip.hpp): salva::sampling::shape_surface_ray_sample / shape_volume_ray_sample,
// LiquidWorld::add_particles_from_shape and Boundary::sampled_from_shape.  Writes, as raw f32 triples each preceded by a uint64
// count: the ball's surface samples, the capsule's volume samples, the fluid after add_particles_from_shape, the sampled boundary
// after a pose, and the fluid after two steps.  tests/test_sampling_gpu.py compares the file with the Python mirror's results.
#include <cstdio>
#include <cstdlib>

#include "../../include/salva_hip.hpp"

static void put(FILE* f, const std::vector<salva::Vec3>& v) {
    const uint64_t n = v.size();
    fwrite(&n, sizeof n, 1, f);
    if (n) fwrite(v[0].data(), sizeof(float), 3 * n, f);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    try {
        const float r = 0.0125f;
        salva::LiquidWorld world(salva::DFSPHSolver(), r, 2.0f);
        const SalvaHipShape ball{SALVA_HIP_SHAPE_BALL, {0.15f, 0, 0}}, capsule{SALVA_HIP_SHAPE_CAPSULE, {0.2f, 0.1f, 0}};
        const SalvaHipShape block{SALVA_HIP_SHAPE_CUBOID, {0.06f, 0.05f, 0.07f}}, floor_shape{SALVA_HIP_SHAPE_CUBOID, {0.2f, 0.03f, 0.2f}};
        FILE* f = fopen(argv[1], "wb");
        if (!f) return 3;
        put(f, salva::sampling::shape_surface_ray_sample(world, ball, r));
        put(f, salva::sampling::shape_volume_ray_sample(world, capsule, r));
        const salva::FluidHandle h = world.add_fluid(salva::Fluid({}, r, 1000.0f));
        const salva::BoundaryHandle b = world.add_boundary(salva::Boundary::sampled_from_shape(floor_shape));
        const salva::Vec3 v{0.0f, -0.5f, 0.0f};
        const size_t k = world.add_particles_from_shape(h, block, salva::Vec3{0.01f, 0.12f, -0.02f}, {0, 0, 0, 1}, SALVA_HIP_SAMPLE_VOLUME, &v);
        if (k == 0 || world.fluids()[h].num_particles() != k) return 4;
        put(f, world.fluids()[h].positions);
        SalvaHipRigidPose pose{};
        pose.rotation[3] = 1.0f;
        world.update_boundary_pose(b, pose);
        world.sync_boundary(b);
        put(f, world.boundaries()[b].positions);
        for (int s = 0; s < 2; ++s) world.step(1.0f / 200.0f, salva::Vec3{0.0f, -9.81f, 0.0f});
        put(f, world.fluids()[h].positions);
        fclose(f);
    } catch (const std::exception& e) {
        fprintf(stderr, "sampling_mirror: %s\n", e.what());
        return 1;
    }
    return 0;
}

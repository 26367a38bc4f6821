// depth_image3.cpp — what a depth sensor above the fluid sees: a block of 10^3 particles (r = 0.05, the basic3 lattice) dropped for a
// few steps, then a 64 x 48 camera three units above it looking down, cast at the particles' spheres on the device
// (LiquidWorld::cast_camera): a depth image (t along the unit `forward`) and a thickness image, the two inputs of
// screen-space fluid rendering.  Prints the hit count and the sums and minima of both images.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../include/salva_hip.hpp"

using namespace salva;

static const Real PARTICLE_RADIUS = 0.05f, SMOOTHING_FACTOR = 2.0f;

int main(int argc, char** argv) {
    const int nsteps = argc > 1 ? atoi(argv[1]) : 5;
    try {
        LiquidWorld world(DFSPHSolver(), PARTICLE_RADIUS, SMOOTHING_FACTOR);
        const size_t n = 10;
        std::vector<Vec3> points;
        for (size_t i = 0; i < n; ++i)
            for (size_t j = 0; j < n; ++j)
                for (size_t k = 0; k < n; ++k) {  // examples3d/helper.rs:4-20, lifted by one unit
                    const Real r = PARTICLE_RADIUS, half = (Real)n * r;
                    points.push_back(Vec3{(Real)i * r * 2.0f + r - half, ((Real)j * r * 2.0f + r - half) + 1.0f, (Real)k * r * 2.0f + r - half});
                }
        world.add_fluid(Fluid(points, PARTICLE_RADIUS, 1000.0f, InteractionGroups{}));
        const Vec3 gravity{0.0f, -9.81f, 0.0f};
        for (int s = 0; s < nsteps; ++s) world.step(1.0f / 200.0f, gravity);
        const RayCamera camera{Vec3{0.0f, 3.0f, 0.0f}, Vec3{0.0f, -1.0f, 0.0f}, Vec3{0.8f, 0.0f, 0.0f}, Vec3{0.0f, 0.0f, 0.6f}, 64, 48};
        const RayHits img = world.cast_camera(camera, RaySet::HIT | RaySet::THICKNESS);
        size_t hits = 0;
        double depth_sum = 0.0, thick_sum = 0.0;
        Real depth_min = INFINITY, thick_min = INFINITY;
        for (size_t i = 0; i < img.t.size(); ++i) {
            thick_sum += (double)img.thickness[i];
            if (!img.hit(i)) continue;
            ++hits;
            depth_sum += (double)img.t[i];
            depth_min = img.t[i] < depth_min ? img.t[i] : depth_min;
            thick_min = img.thickness[i] < thick_min ? img.thickness[i] : thick_min;
        }
        printf("camera %u x %u after %d steps\n", camera.width, camera.height, nsteps);
        printf("hits %zu of %zu; depth sum %.17g min %.9g; thickness sum %.17g min %.9g\n", hits, img.t.size(), depth_sum, depth_min, thick_sum,
               thick_min);
    } catch (const std::exception& e) {
        fprintf(stderr, "depth_image3: %s\n", e.what());
        return 1;
    }
    return 0;
}

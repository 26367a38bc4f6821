// anisotropic_surface3.cpp — the fluid's surface with and without anisotropic kernels: the scene of surface3.cpp (the basic3 block,
// 15^3 particles, r = 0.05, DFSPH + XSPHViscosity, 50 steps), a lattice at spacing r around the fluid's box grown by 2h (what an
// anisotropic kernel can reach), and the surface fraction = 0.5 extracted twice on the device with normals: with the isotropic kernels
// of DESIGN.md §21 and with the anisotropic kernels of §23 at their default parameters (LiquidWorld::extract_surface with an
// Anisotropy).  Prints the counts, the enclosed volume and the area of both, and writes two Wavefront OBJ files, PREFIX_isotropic.obj
// and PREFIX_anisotropic.obj, when a prefix is given as the first argument.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

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

// prints the counts, the enclosed volume and the area (in double) and writes the OBJ
static int report(const char* name, const SurfaceMesh& mesh, const char* prefix) {
    double volume = 0.0, area = 0.0;
    for (size_t t = 0; t < mesh.num_triangles(); ++t) {
        double p[3][3];
        for (int c = 0; c < 3; ++c)
            for (int a = 0; a < 3; ++a) p[c][a] = mesh.vertices[3 * (size_t)mesh.triangles[3 * t + c] + a];
        const double u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]}, v[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
        const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
        area += 0.5 * std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        const double bc[3] = {p[1][1] * p[2][2] - p[1][2] * p[2][1], p[1][2] * p[2][0] - p[1][0] * p[2][2], p[1][0] * p[2][1] - p[1][1] * p[2][0]};
        volume += (p[0][0] * bc[0] + p[0][1] * bc[1] + p[0][2] * bc[2]) / 6.0;
    }
    printf("%s: vertices: %zu; triangles: %zu; volume %.6f; area %.6f\n", name, mesh.num_vertices(), mesh.num_triangles(), volume, area);
    if (!prefix) return 0;
    const std::string path = std::string(prefix) + "_" + name + ".obj";
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
    // (nine significant digits: a float survives the round trip)
    for (size_t v = 0; v < mesh.num_vertices(); ++v) fprintf(f, "v %.9g %.9g %.9g\n", mesh.vertices[3 * v], mesh.vertices[3 * v + 1], mesh.vertices[3 * v + 2]);
    for (size_t v = 0; v < mesh.num_vertices(); ++v) fprintf(f, "vn %.9g %.9g %.9g\n", mesh.normals[3 * v], mesh.normals[3 * v + 1], mesh.normals[3 * v + 2]);
    for (size_t t = 0; t < mesh.num_triangles(); ++t) {
        const uint32_t a = mesh.triangles[3 * t] + 1u, b = mesh.triangles[3 * t + 1] + 1u, c = mesh.triangles[3 * t + 2] + 1u;
        fprintf(f, "f %u//%u %u//%u %u//%u\n", a, a, b, b, c, c);
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    const char* prefix = argc > 1 ? argv[1] : nullptr;
    const int nsteps = argc > 2 ? atoi(argv[2]) : 50;
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
        for (int s = 0; s < nsteps; ++s) world.step(1.0f / 200.0f, gravity);
        // one lattice for both: an anisotropic kernel reaches up to 2h from its centre
        const Real r = PARTICLE_RADIUS;
        const LiquidWorld::Lattice lattice = world.surface_lattice(r, 2.0f * world.h());
        printf("lattice %u x %u x %u at spacing %.3f after %d steps\n", lattice.dims[0], lattice.dims[1], lattice.dims[2], r, nsteps);
        const SurfaceMesh iso = world.extract_surface(lattice.origin, r, lattice.dims, 0.5f, SALVA_HIP_SURFACE_FRACTION, true);
        const SurfaceMesh aniso = world.extract_surface(lattice.origin, r, lattice.dims, Anisotropy(), 0.5f, SALVA_HIP_SURFACE_FRACTION, true);
        if (report("isotropic", iso, prefix) || report("anisotropic", aniso, prefix)) return 1;
    } catch (const Error& e) {
        fprintf(stderr, "salva error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}

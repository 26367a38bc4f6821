// anisotropy.hip — anisotropic kernels for the fluid's surface (include/salva_hip.h "Anisotropic kernels").
// k_aniso_moments: one lane per particle over the 27 cells of width 2h around it — nine runs of three contiguous cells in the sorted
// records of the field evaluator's table (field.hip) —, the ten sums S0, S1, S2 in registers, then the symmetric 3 x 3
// eigen-decomposition by cyclic Jacobi and the metric.  k_aniso_points: one lane per place over the same walk on a table built on the
// centres, two more float4 records per candidate.  Every matrix is a handful of named scalars: indexed as an array it would live in
// scratch (tests/test_anisotropy_resources.py).  Both kernels visit cells in ascending order and rows in ascending host index within
// a cell: the order of every sum is fixed.
//
// Compiled once, like field.hip, with the reference's other kernels switched in as wave-uniform branches of kernel_eval.
#define SALVA_OTHER_KERNELS 1
#include "anisotropy.h"
#include "tile.h"

namespace salva {

// the cell of a position in g (field.hip field_cell); false: outside or not finite
__device__ __forceinline__ bool aniso_cell(const FieldGrid& g, float x, float y, float z, uint32_t& ux, uint32_t& uy, uint32_t& uz) {
    bool bad = false;
    const int cx = cell_coord(x, g.h, bad), cy = cell_coord(y, g.h, bad), cz = cell_coord(z, g.h, bad);
    ux = (uint32_t)cx - (uint32_t)g.o[0]; uy = (uint32_t)cy - (uint32_t)g.o[1]; uz = (uint32_t)cz - (uint32_t)g.o[2];
    return !bad && isfinite(x) && isfinite(y) && isfinite(z) && ux < g.d[0] && uy < g.d[1] && uz < g.d[2];
}

// One Jacobi rotation of the symmetric matrix in the plane (p, q), r the third index: app, aqq, apq and the two entries arp, arq
// beside them; (vkp, vkq), k = 0..2: the two columns of the accumulated rotation.  apq = 0 (C = 0, a diagonal C) rotates by nothing.
__device__ __forceinline__ void jacobi_rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float& v0p, float& v0q, float& v1p,
                                              float& v1q, float& v2p, float& v2q) {
    float t = 0.0f;
    if (apq != 0.0f) {
        const float theta = (aqq - app) / (2.0f * apq);  // (may be +-inf: t = 0)
        t = copysignf(1.0f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
    }
    const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0f;
    const float rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    const float a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
    const float a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
    const float a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
    v0p = a0; v0q = b0; v1p = a1; v1q = b1; v2p = a2; v2q = b2;
}

constexpr int ANISO_SWEEPS = 5;  // cyclic Jacobi on a 3 x 3 converges quadratically: f32 is reached in three or four

__global__ __launch_bounds__(BLOCK) void k_aniso_moments(uint32_t n, FieldGrid g, FieldCandidates cand, const uint32_t* __restrict__ rows,
                                                         const float4* __restrict__ st_pos, uint32_t ring, AnisoParams prm, float h, AnisoRows out) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n || p >= cand.cells[g.ncells]) return;  // (cells[ncells]: the kept rows)
    const uint32_t v = rows[p];
    if (v >= n) return;
    const float4 xi = cand.rec0[p];
    uint32_t ux, uy, uz;
    if (!aniso_cell(g, xi.x, xi.y, xi.z, ux, uy, uz)) return;  // (cannot happen: the row was sorted into g by this test)
    if (ux < ring || uy < ring || uz < ring || ux + ring >= g.d[0] || uy + ring >= g.d[1] || uz + ring >= g.d[2]) return;
    const float R = h + h, R2 = R * R, inv_R = 1.0f / R;
    float s0 = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sxx = 0.0f, sxy = 0.0f, sxz = 0.0f, syy = 0.0f, syz = 0.0f, szz = 0.0f;
    uint32_t cnt = 0;
    const uint32_t x0 = ux ? ux - 1u : 0u, x1 = min(ux + 1u, g.d[0] - 1u), y0 = uy ? uy - 1u : 0u, y1 = min(uy + 1u, g.d[1] - 1u),
                   z0 = uz ? uz - 1u : 0u, z1 = min(uz + 1u, g.d[2] - 1u);
    for (uint32_t cx = x0; cx <= x1; ++cx)
        for (uint32_t cy = y0; cy <= y1; ++cy) {
            const uint32_t row = (cx * g.d[1] + cy) * g.d[2];
            const uint32_t b = cand.cells[row + z0], e = min(cand.cells[row + z1 + 1u], n);
            for (uint32_t j = b; j < e; ++j) {
                const float4 xj = cand.rec0[j];
                const float dx = xj.x - xi.x, dy = xj.y - xi.y, dz = xj.z - xi.z;
                const float r2 = dist2_exact(dx, dy, dz);
                if (!(r2 <= R2)) continue;
                const float t = sqrtf(r2) * inv_R;
                const float w = 1.0f - t * t * t;
                const float wx = w * dx, wy = w * dy, wz = w * dz;
                s0 += w;
                sx += wx; sy += wy; sz += wz;
                sxx += wx * dx; sxy += wx * dy; sxz += wx * dz; syy += wy * dy; syz += wy * dz; szz += wz * dz;
                cnt += 1u;
            }
        }
    // (the particle is its own neighbour with w = 1: s0 >= 1)
    const float inv_s0 = 1.0f / s0;
    const float mx = sx * inv_s0, my = sy * inv_s0, mz = sz * inv_s0;
    float a00 = sxx * inv_s0 - mx * mx, a01 = sxy * inv_s0 - mx * my, a02 = sxz * inv_s0 - mx * mz, a11 = syy * inv_s0 - my * my,
          a12 = syz * inv_s0 - my * mz, a22 = szz * inv_s0 - mz * mz;
    const uint32_t neighbours = cnt ? cnt - 1u : 0u;
    const float inv_h = 1.0f / h;
    float gxx, gxy, gxz, gyy, gyz, gzz, det;
    if (neighbours > prm.n_eps) {
        float v00 = 1.0f, v01 = 0.0f, v02 = 0.0f, v10 = 0.0f, v11 = 1.0f, v12 = 0.0f, v20 = 0.0f, v21 = 0.0f, v22 = 1.0f;
#pragma unroll
        for (int sweep = 0; sweep < ANISO_SWEEPS; ++sweep) {
            jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
            jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
            jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
        }
        // one function of every eigenvalue: no order is needed beyond the largest
        const float lowest = fmaxf(fmaxf(a00, a11), a22) / prm.k_r, scale = prm.k_s * (inv_h * inv_h);
        const float s1 = fminf(fmaxf(scale * fmaxf(a00, lowest), SALVA_HIP_ANISOTROPY_S_LO), SALVA_HIP_ANISOTROPY_S_HI);
        const float s2 = fminf(fmaxf(scale * fmaxf(a11, lowest), SALVA_HIP_ANISOTROPY_S_LO), SALVA_HIP_ANISOTROPY_S_HI);
        const float s3 = fminf(fmaxf(scale * fmaxf(a22, lowest), SALVA_HIP_ANISOTROPY_S_LO), SALVA_HIP_ANISOTROPY_S_HI);
        const float i1 = inv_h / s1, i2 = inv_h / s2, i3 = inv_h / s3;
        gxx = i1 * v00 * v00 + i2 * v01 * v01 + i3 * v02 * v02;
        gxy = i1 * v00 * v10 + i2 * v01 * v11 + i3 * v02 * v12;
        gxz = i1 * v00 * v20 + i2 * v01 * v21 + i3 * v02 * v22;
        gyy = i1 * v10 * v10 + i2 * v11 * v11 + i3 * v12 * v12;
        gyz = i1 * v10 * v20 + i2 * v11 * v21 + i3 * v12 * v22;
        gzz = i1 * v20 * v20 + i2 * v21 * v21 + i3 * v22 * v22;
        det = i1 * i2 * i3;
    } else {
        const float i = inv_h / prm.k_n;
        gxx = gyy = gzz = i;
        gxy = gxz = gyz = 0.0f;
        det = i * i * i;
    }
    const float vol = st_pos[v].w;
    out.centre[v] = make_float4(xi.x + prm.lambda * mx, xi.y + prm.lambda * my, xi.z + prm.lambda * mz, vol);
    out.m0[v] = make_float4(gxx, gxy, gxz, gyy);
    out.m1[v] = make_float4(gyz, gzz, det * xi.w, det * vol);
    out.count[v] = neighbours;
}
void launch_aniso_moments(uint32_t n, const FieldGrid& g, const FieldCandidates& cand, const uint32_t* rows, const float4* st_pos, uint32_t ring,
                          const AnisoParams& prm, float h, const AnisoRows& out, hipStream_t st) {
    if (!n) return;
    k_aniso_moments<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, g, cand, rows, st_pos, ring, prm, h, out);
    SALVA_HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(BLOCK) void k_aniso_gather(uint32_t n, const uint32_t* __restrict__ cells, uint32_t ncells, const uint32_t* __restrict__ rows,
                                                        AnisoRows in, float4* __restrict__ g0, float4* __restrict__ g1) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n || p >= cells[ncells]) return;
    const uint32_t v = rows[p];
    if (v >= n) return;
    g0[p] = in.m0[v];
    g1[p] = in.m1[v];
}
void launch_aniso_gather(uint32_t n, const uint32_t* cells, uint32_t ncells, const uint32_t* rows, const AnisoRows& in, float4* g0, float4* g1,
                         hipStream_t st) {
    if (!n) return;
    k_aniso_gather<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, cells, ncells, rows, in, g0, g1);
    SALVA_HIP_CHECK(hipGetLastError());
}

__device__ __forceinline__ float aniso_node(float origin, float spacing, uint32_t i) { return origin + opaque((float)i * spacing); }  // (field.hip field_node)

__global__ __launch_bounds__(BLOCK) void k_aniso_points(FieldQuery q, FieldGrid g, FieldCandidates cand, const float4* __restrict__ g0,
                                                        const float4* __restrict__ g1, SphConsts c, AnisoOutDev out) {
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= q.npoints) return;
    float x, y, z;
    if (q.pts) {
        x = q.pts[3 * i]; y = q.pts[3 * i + 1]; z = q.pts[3 * i + 2];
    } else {
        const uint64_t nz = q.dims[2], ny = q.dims[1];
        const uint32_t iz = (uint32_t)(i % nz), iy = (uint32_t)((i / nz) % ny), ix = (uint32_t)(i / (nz * ny));
        x = aniso_node(q.origin[0], q.spacing, ix); y = aniso_node(q.origin[1], q.spacing, iy); z = aniso_node(q.origin[2], q.spacing, iz);
    }
    const bool want_grad = out.gradient != nullptr;  // (uniform)
    float rho = 0.0f, frac = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
    uint32_t ux, uy, uz;
    if (aniso_cell(g, x, y, z, ux, uy, uz)) {
        const uint32_t x0 = ux ? ux - 1u : 0u, x1 = min(ux + 1u, g.d[0] - 1u), y0 = uy ? uy - 1u : 0u, y1 = min(uy + 1u, g.d[1] - 1u),
                       z0 = uz ? uz - 1u : 0u, z1 = min(uz + 1u, g.d[2] - 1u);
        for (uint32_t cx = x0; cx <= x1; ++cx)
            for (uint32_t cy = y0; cy <= y1; ++cy) {
                const uint32_t row = (cx * g.d[1] + cy) * g.d[2];
                const uint32_t b = cand.cells[row + z0], e = cand.cells[row + z1 + 1u];
                for (uint32_t p = b; p < e; ++p) {
                    const float4 r0 = cand.rec0[p], a0 = g0[p], a1 = g1[p];
                    const float dx = x - r0.x, dy = y - r0.y, dz = z - r0.z;
                    const float yx = a0.x * dx + a0.y * dy + a0.z * dz, yy = a0.y * dx + a0.w * dy + a1.x * dz, yz = a0.z * dx + a1.x * dy + a1.y * dz;
                    const float q2 = dist2_exact(yx, yy, yz);
                    if (!(q2 <= 1.0f)) continue;
                    const KernelEval k = kernel_eval(q2, c);
                    rho += a1.z * k.w;
                    frac += a1.w * k.w;
                    if (want_grad) {
                        const float mg = a1.z * k.g;
                        gx += mg * (a0.x * yx + a0.y * yy + a0.z * yz);
                        gy += mg * (a0.y * yx + a0.w * yy + a1.x * yz);
                        gz += mg * (a0.z * yx + a1.x * yy + a1.y * yz);
                    }
                }
            }
    }
    if (out.density) out.density[i] = rho;
    if (out.fraction) out.fraction[i] = frac;
    if (out.gradient) { out.gradient[3 * i] = gx; out.gradient[3 * i + 1] = gy; out.gradient[3 * i + 2] = gz; }
}
void launch_aniso_points(const FieldQuery& q, const FieldGrid& g, const FieldCandidates& cand, const float4* g0, const float4* g1, const SphConsts& c,
                         const AnisoOutDev& out, hipStream_t st) {
    if (!q.npoints) return;
    k_aniso_points<<<div_up(q.npoints, BLOCK), BLOCK, 0, st>>>(q, g, cand, g0, g1, c, out);
    SALVA_HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(BLOCK) void k_aniso_pack(uint32_t n, const float4* __restrict__ st_pos, const uint32_t* __restrict__ st_model, RowPack pk,
                                                      AnisoRows in, float* __restrict__ centres, float* __restrict__ metric,
                                                      uint32_t* __restrict__ count) {
    const uint32_t v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= n) return;
    const uint32_t s = st_model[v];
    if (s >= FIELD_MAX_SLOTS || !((pk.mask >> s) & 1u) || v < pk.first[s] || v - pk.first[s] >= pk.len[s]) return;
    const uint64_t r = (uint64_t)pk.base[s] + (v - pk.first[s]);
    const float4 x = st_pos[v];
    const bool finite = isfinite(x.x) && isfinite(x.y) && isfinite(x.z);
    const float4 c = finite ? in.centre[v] : x;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 m0 = finite ? in.m0[v] : zero, m1 = finite ? in.m1[v] : zero;
    if (centres) { centres[3 * r] = c.x; centres[3 * r + 1] = c.y; centres[3 * r + 2] = c.z; }
    if (metric) {
        metric[6 * r] = m0.x; metric[6 * r + 1] = m0.y; metric[6 * r + 2] = m0.z; metric[6 * r + 3] = m0.w; metric[6 * r + 4] = m1.x;
        metric[6 * r + 5] = m1.y;
    }
    if (count) count[r] = finite ? in.count[v] : 0u;
}
void launch_aniso_pack(uint32_t n, const float4* st_pos, const uint32_t* st_model, const RowPack& pk, const AnisoRows& in, float* centres,
                       float* metric, uint32_t* count, hipStream_t st) {
    if (!n) return;
    k_aniso_pack<<<div_up(n, BLOCK), BLOCK, 0, st>>>(n, st_pos, st_model, pk, in, centres, metric, count);
    SALVA_HIP_CHECK(hipGetLastError());
}

}  // namespace salva

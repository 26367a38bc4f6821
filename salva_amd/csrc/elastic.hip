// elastic.hip — Becker et al. 2009 corotated SPH elasticity (solver/elasticity/becker2009_elasticity.rs) on the device.
//
// State (elastic.h ElasticState) is per fluid and per force entry, in the fluid's host order: positions0, volumes0, rotations,
// stresses, deformation gradients and the rest lists as CSR (rows ascending in j, so every sum has one fixed order).  The weight
// and gradient of a rest contact are not stored: they are recomputed from p0_i - p0_j, the same f32 arithmetic every time.
// Passes of a step (World::run_elasticity): gather this step's positions into host order, the fused rotation + stress pass, the
// force pass over the sorted slots.  The rest build runs only when the state is stale (a count change, a restored state).
// Compiled with the library's -ffp-contract=off, like the reference (Rust never contracts).
#include <hipcub/hipcub.hpp>

#include "elastic.h"
#include "kernels.h"
#include "sph_math.h"
#include "tile.h"

namespace salva {

// elasticity_coefficients (:15-24), in f32 and in the reference's operation order; no validation (nu = 0.5 gives inf, as there)
ElasticParams elastic_params(const float p[7]) {
    const float E = p[0], nu = p[1];
    ElasticParams ep;
    ep.d0 = (E * (1.0f - nu)) / ((1.0f + nu) * (1.0f - 2.0f * nu));
    ep.d1 = (E * nu) / ((1.0f + nu) * (1.0f - 2.0f * nu));
    ep.d2 = (E * (1.0f - 2.0f * nu)) / (2.0f * (1.0f + nu) * (1.0f - 2.0f * nu));
    ep.nonlinear = p[2] != 0.0f;
    ep.kd = (int)p[3];
    ep.kg = (int)p[4];
    return ep;
}

namespace {

// KernelDensity::points_apply(p0_i, p0_j) from |p0_i - p0_j|^2 (kernel.rs:27-34)
template <bool OK>
__device__ __forceinline__ float el_w(float r2, const SphConsts& c, int kd) {
    const float r = sqrtf(r2);
    if (OK && kd) return other_kernel_w(kd, r, c);
    return c.wnorm * cubic_w_unit(r * c.inv_h);
}
// KernelGradient::points_apply_diff1(p0_i, p0_j) = g (p0_i - p0_j); zero when |v| <= eps (kernel.rs:18-24)
template <bool OK>
__device__ __forceinline__ float el_g(float r2, const SphConsts& c, int kg) {
    if (!(r2 > c.eps2)) return 0.0f;
    const float r = sqrtf(r2);
    if (OK && kg) return other_kernel_dw(kg, r, c) / r;
    return c.gnorm * cubic_dw_unit(r * c.inv_h) / r;
}

__global__ __launch_bounds__(BLOCK) void k_el_gather(StepCtx c, uint32_t off, uint32_t nn, float4* __restrict__ hp) {
    const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
    if (s >= c.n || gate_closed(c)) return;
    const uint32_t i = c.perm[s] - off;  // (wraps for the particles of other fluids)
    if (i < nn) hp[i] = c.posm[s];
}

__global__ __launch_bounds__(BLOCK) void k_el_take_rest(uint32_t n, const float4* __restrict__ hp, float4* __restrict__ p0) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) { const float4 p = hp[i]; p0[i] = make_float4(p.x, p.y, p.z, 0.0f); }
}

__global__ __launch_bounds__(BLOCK) void k_el_identity(uint32_t from, uint32_t to, float* __restrict__ rot) {
    const uint32_t i = from + blockIdx.x * BLOCK + threadIdx.x;
    if (i >= to) return;
    float* r = rot + 9 * (size_t)i;
    for (int k = 0; k < 9; ++k) r[k] = (k % 4 == 0) ? 1.0f : 0.0f;
}

// ---------------------------------------------------------------------------------------------------------- rest build
// The cell search of compute_self_contacts over the 27 cells around the particle's own, cells of width h (HGrid::new(h)) keyed
// into a power-of-two table.  Cells that land in the same bucket are walked once, and a candidate must sit in one of the 27
// cells: the pair set is the reference's, the d^2 <= h^2 test is dist2_exact's.
__device__ __forceinline__ uint32_t el_bucket(int x, int y, int z, uint32_t mask) {
    return (((uint32_t)x * 73856093u) ^ ((uint32_t)y * 19349663u) ^ ((uint32_t)z * 83492791u)) & mask;
}
__device__ __forceinline__ int3 el_cell(float4 p, float h) {
    bool bad = false;
    return make_int3(cell_coord(p.x, h, bad), cell_coord(p.y, h, bad), cell_coord(p.z, h, bad));
}

__global__ __launch_bounds__(BLOCK) void k_el_keys(uint32_t n, const float4* __restrict__ p0, float h, uint32_t mask,
                                                   uint32_t* __restrict__ keys, uint32_t* __restrict__ idx) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int3 q = el_cell(p0[i], h);
    keys[i] = el_bucket(q.x, q.y, q.z, mask);
    idx[i] = i;
}

// FILL = false: count[i] = rest contacts of i; true: write them at off[i], then sort the row by j
template <bool FILL>
__global__ __launch_bounds__(BLOCK) void k_el_search(uint32_t n, const float4* __restrict__ p0, float h, float h2, uint32_t mask,
                                                     const uint32_t* __restrict__ start, const uint32_t* __restrict__ sidx,
                                                     uint32_t* __restrict__ count, const uint32_t* __restrict__ off, uint32_t* __restrict__ nbr) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 pi = p0[i];
    const int3 q = el_cell(pi, h);
    uint32_t seen[27];
    uint32_t nseen = 0, cnt = 0;
    const uint32_t base = FILL ? off[i] : 0u;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const uint32_t b = el_bucket(q.x + dx, q.y + dy, q.z + dz, mask);
                bool dup = false;
                for (uint32_t k = 0; k < nseen; ++k) dup |= seen[k] == b;
                if (dup) continue;
                seen[nseen++] = b;
                for (uint32_t k = start[b]; k < start[b + 1]; ++k) {
                    const uint32_t j = sidx[k];
                    const float4 pj = p0[j];
                    const int3 qj = el_cell(pj, h);
                    if (abs(qj.x - q.x) > 1 || abs(qj.y - q.y) > 1 || abs(qj.z - q.z) > 1) continue;
                    if (dist2_exact(pi.x - pj.x, pi.y - pj.y, pi.z - pj.z) <= h2) {
                        if (FILL) nbr[base + cnt] = j;
                        ++cnt;
                    }
                }
            }
    if (!FILL) { count[i] = cnt; return; }
    // rows are short (a few dozen): insertion sort in place
    for (uint32_t a = 1; a < cnt; ++a) {
        const uint32_t v = nbr[base + a];
        uint32_t b = a;
        while (b > 0 && nbr[base + b - 1] > v) { nbr[base + b] = nbr[base + b - 1]; --b; }
        nbr[base + b] = v;
    }
}

// init (:96-111): volumes0[i] (the value it kept through the resize: quirk 1) + both endpoints of every directed contact (quirk 2),
// i.e. 2 m_j W_ij per rest neighbour j, self pair included; then volumes0[i] = m_i / that
template <bool OK>
__global__ __launch_bounds__(BLOCK) void k_el_volumes0(uint32_t n, const float4* __restrict__ p0, const float4* __restrict__ hp,
                                                       const uint32_t* __restrict__ off, const uint32_t* __restrict__ nbr,
                                                       SphConsts sc, int kd, float* __restrict__ vol0) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 pi = p0[i];
    float acc = vol0[i];
    for (uint32_t k = off[i]; k < off[i + 1]; ++k) {
        const uint32_t j = nbr[k];
        const float4 pj = p0[j];
        const float dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
        const float t = hp[j].w * el_w<OK>(dx * dx + dy * dy + dz * dz, sc, kd);
        acc += t;
        acc += t;
    }
    vol0[i] = hp[i].w / acc;
}

// ---------------------------------------------------------------------------------------------------------- rotation + stress
// Rotation3::from_matrix_eps(A, eps, 20, R_prev) (nalgebra; Mueller et al. 2016): w = sum_c R_c x A_c / (|sum_c R_c . A_c| + eps),
// stop when |w| <= eps, else R <- Rot(w / |w|, |w|) R (Rodrigues)
__device__ __forceinline__ void el_extract_rotation(const float A[9], float R[9]) {
    const float eps = 1.1920929e-7f;
    for (int it = 0; it < 20; ++it) {
        float ax = 0.0f, ay = 0.0f, az = 0.0f, den = 0.0f;
#pragma unroll
        for (int col = 0; col < 3; ++col) {
            const float rx = R[col], ry = R[3 + col], rz = R[6 + col];
            const float mx = A[col], my = A[3 + col], mz = A[6 + col];
            ax += ry * mz - rz * my;
            ay += rz * mx - rx * mz;
            az += rx * my - ry * mx;
            den += rx * mx + ry * my + rz * mz;
        }
        const float dd = fabsf(den) + eps;
        ax = ax / dd; ay = ay / dd; az = az / dd;
        const float ang = sqrtf(ax * ax + ay * ay + az * az);
        if (!(ang > eps)) break;
        const float ux = ax / ang, uy = ay / ang, uz = az / ang;
        float sn, cs;
        sincosf(ang, &sn, &cs);
        const float omc = 1.0f - cs;
        const float Q[9] = {ux * ux + (1.0f - ux * ux) * cs, ux * uy * omc - uz * sn,          ux * uz * omc + uy * sn,
                            ux * uy * omc + uz * sn,          uy * uy + (1.0f - uy * uy) * cs, uy * uz * omc - ux * sn,
                            ux * uz * omc - uy * sn,          uy * uz * omc + ux * sn,          uz * uz + (1.0f - uz * uz) * cs};
        float T[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) T[3 * r + cc] = Q[3 * r] * R[cc] + Q[3 * r + 1] * R[3 + cc] + Q[3 * r + 2] * R[6 + cc];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = T[k];
    }
}

template <bool OK>
__global__ __launch_bounds__(BLOCK) void k_el_rot_stress(StepCtx c, uint32_t n, const float4* __restrict__ hp, const float4* __restrict__ p0,
                                                         const float* __restrict__ vol0, const uint32_t* __restrict__ off,
                                                         const uint32_t* __restrict__ nbr, ElasticParams ep, const float* __restrict__ rot,
                                                         float* __restrict__ rot_out,
                                                         float* __restrict__ sig, float* __restrict__ Fo) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || gate_closed(c)) return;
    const SphConsts& sc = c.sc;
    const float4 pi = hp[i], p0i = p0[i];
    const uint32_t k0 = off[i], k1 = off[i + 1];
    // compute_rotations (:115-137): A_pq = sum_j m_j W_ij (p_j - p_i) (p0_j - p0_i)^T
    float A[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t j = nbr[k];
        const float4 pj = hp[j], p0j = p0[j];
        const float ex = p0i.x - p0j.x, ey = p0i.y - p0j.y, ez = p0i.z - p0j.z;
        const float coeff = el_w<OK>(ex * ex + ey * ey + ez * ez, sc, ep.kd) * pj.w;
        const float px = pj.x - pi.x, py = pj.y - pi.y, pz = pj.z - pi.z;
        const float qx = (p0j.x - p0i.x) * coeff, qy = (p0j.y - p0i.y) * coeff, qz = (p0j.z - p0i.z) * coeff;
        A[0] += px * qx; A[1] += px * qy; A[2] += px * qz;
        A[3] += py * qx; A[4] += py * qy; A[5] += py * qz;
        A[6] += pz * qx; A[7] += pz * qy; A[8] += pz * qz;
    }
    float R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = rot[9 * (size_t)i + k];
    el_extract_rotation(A, R);
    // compute_stresses (:139-262): F = sum_j (grad W_ij V0_j) u_ji^T, u_ji = R^T (p_j - p_i) - (p0_j - p0_i)
    float F[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t j = nbr[k];
        const float4 pj = hp[j], p0j = p0[j];
        const float ex = p0i.x - p0j.x, ey = p0i.y - p0j.y, ez = p0i.z - p0j.z;
        const float g = el_g<OK>(ex * ex + ey * ey + ez * ez, sc, ep.kg);
        const float v = vol0[j];
        const float gx = (ex * g) * v, gy = (ey * g) * v, gz = (ez * g) * v;
        const float px = pj.x - pi.x, py = pj.y - pi.y, pz = pj.z - pi.z;
        const float ux = (R[0] * px + R[3] * py + R[6] * pz) - (p0j.x - p0i.x);
        const float uy = (R[1] * px + R[4] * py + R[7] * pz) - (p0j.y - p0i.y);
        const float uz = (R[2] * px + R[5] * py + R[8] * pz) - (p0j.z - p0i.z);
        F[0] += gx * ux; F[1] += gx * uy; F[2] += gx * uz;
        F[3] += gy * ux; F[4] += gy * uy; F[5] += gy * uz;
        F[6] += gz * ux; F[7] += gz * uy; F[8] += gz * uz;
    }
    const float k05 = 0.564f;  // `_0_5` of compute_stresses (:141) is 0.564, not 0.5 (quirk 3)
    float e0, e1, e2, sxy, sxz, syz;
    if (ep.nonlinear) {
        // J = F + I, S = J J^T
        const float J[9] = {F[0] + 1.0f, F[1], F[2], F[3], F[4] + 1.0f, F[5], F[6], F[7], F[8] + 1.0f};
        auto S = [&](int r, int cc) { return J[3 * r] * J[3 * cc] + J[3 * r + 1] * J[3 * cc + 1] + J[3 * r + 2] * J[3 * cc + 2]; };
        e0 = S(0, 0) - 1.0f; e1 = S(1, 1) - 1.0f; e2 = S(2, 2) - 1.0f;
        const float s0 = (ep.d0 * e0 + ep.d1 * e1 + ep.d1 * e2) * k05;
        const float s1 = (ep.d1 * e0 + ep.d0 * e1 + ep.d1 * e2) * k05;
        const float s2 = (ep.d1 * e0 + ep.d1 * e1 + ep.d0 * e2) * k05;
        e0 = s0; e1 = s1; e2 = s2;
        sxy = S(1, 0) * k05 * ep.d2; sxz = S(2, 0) * k05 * ep.d2; syz = S(2, 1) * k05 * ep.d2;
    } else {
        const float s0 = ep.d0 * F[0] + ep.d1 * F[4] + ep.d1 * F[8];
        const float s1 = ep.d1 * F[0] + ep.d0 * F[4] + ep.d1 * F[8];
        const float s2 = ep.d1 * F[0] + ep.d1 * F[4] + ep.d0 * F[8];
        e0 = s0; e1 = s1; e2 = s2;
        sxy = (F[3] + F[1]) * k05 * ep.d2; sxz = (F[6] + F[2]) * k05 * ep.d2; syz = (F[5] + F[7]) * k05 * ep.d2;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) { rot_out[9 * (size_t)i + k] = R[k]; Fo[9 * (size_t)i + k] = F[k]; }
    float* so = sig + 6 * (size_t)i;
    so[0] = e0; so[1] = e1; so[2] = e2; so[3] = sxy; so[4] = sxz; so[5] = syz;
}

// ---------------------------------------------------------------------------------------------------------- forces
// sym_mat_mul_vec (:27-37), stress (x, y, z, w, a, b) = (xx, yy, zz, xy, xz, yz)
__device__ __forceinline__ float3 el_sym(const float s[6], float x, float y, float z) {
    return make_float3(s[0] * x + s[3] * y + s[4] * z, s[3] * x + s[1] * y + s[5] * z, s[4] * x + s[5] * y + s[2] * z);
}

// solve (:268-334), per rest contact (i, j) with g = grad W(p0_i - p0_j):
//   f_ji = -V0_i (sigma_i d_ij [+ F_i sigma_i d_ij]),  d_ij = g V0_j
//   f_ij = -V0_j (sigma_j d_ji [+ F_j sigma_j d_ji]),  d_ji = -g V0_i
//   a_i += 0.5 (R_j f_ij - R_i f_ji) / (V_i rho0) — V_i rho0 is the particle's mass, posm.w of its sorted slot
template <bool OK, bool NL>
__global__ __launch_bounds__(BLOCK) void k_el_forces(StepCtx c, uint32_t off, uint32_t nn, const float4* __restrict__ p0,
                                                     const float* __restrict__ vol0, const uint32_t* __restrict__ roff,
                                                     const uint32_t* __restrict__ nbr, const float* __restrict__ rot,
                                                     const float* __restrict__ sig, const float* __restrict__ Fg, int kg,
                                                     float4* __restrict__ acc) {
    const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
    if (s >= c.n || gate_closed(c)) return;
    const uint32_t i = c.perm[s] - off;
    if (i >= nn) return;
    const SphConsts& sc = c.sc;
    const float4 p0i = p0[i];
    const float v0i = vol0[i];
    float si[6], Fi[9];
#pragma unroll
    for (int k = 0; k < 6; ++k) si[k] = sig[6 * (size_t)i + k];
#pragma unroll
    for (int k = 0; k < 9; ++k) Fi[k] = NL ? Fg[9 * (size_t)i + k] : 0.0f;
    float ax = 0.f, ay = 0.f, az = 0.f;  // sum_j R_j f_ij
    float bx = 0.f, by = 0.f, bz = 0.f;  // sum_j f_ji (R_i applied once, below)
    for (uint32_t k = roff[i]; k < roff[i + 1]; ++k) {
        const uint32_t j = nbr[k];
        const float4 p0j = p0[j];
        const float ex = p0i.x - p0j.x, ey = p0i.y - p0j.y, ez = p0i.z - p0j.z;
        const float g = el_g<OK>(ex * ex + ey * ey + ez * ez, sc, kg);
        const float gx = ex * g, gy = ey * g, gz = ez * g;
        const float v0j = vol0[j];
        {
            float3 t = el_sym(si, gx * v0j, gy * v0j, gz * v0j);
            if (NL) {
                const float3 u = t;
                t.x += Fi[0] * u.x + Fi[1] * u.y + Fi[2] * u.z;
                t.y += Fi[3] * u.x + Fi[4] * u.y + Fi[5] * u.z;
                t.z += Fi[6] * u.x + Fi[7] * u.y + Fi[8] * u.z;
            }
            bx += t.x * -v0i; by += t.y * -v0i; bz += t.z * -v0i;
        }
        {
            float sj[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) sj[q] = sig[6 * (size_t)j + q];
            float3 t = el_sym(sj, gx * -v0i, gy * -v0i, gz * -v0i);
            if (NL) {
                const float* Fj = Fg + 9 * (size_t)j;
                const float3 u = t;
                t.x += Fj[0] * u.x + Fj[1] * u.y + Fj[2] * u.z;
                t.y += Fj[3] * u.x + Fj[4] * u.y + Fj[5] * u.z;
                t.z += Fj[6] * u.x + Fj[7] * u.y + Fj[8] * u.z;
            }
            const float fx = t.x * -v0j, fy = t.y * -v0j, fz = t.z * -v0j;
            const float* Rj = rot + 9 * (size_t)j;
            ax += Rj[0] * fx + Rj[1] * fy + Rj[2] * fz;
            ay += Rj[3] * fx + Rj[4] * fy + Rj[5] * fz;
            az += Rj[6] * fx + Rj[7] * fy + Rj[8] * fz;
        }
    }
    const float* Ri = rot + 9 * (size_t)i;
    const float rx = Ri[0] * bx + Ri[1] * by + Ri[2] * bz;
    const float ry = Ri[3] * bx + Ri[4] * by + Ri[5] * bz;
    const float rz = Ri[6] * bx + Ri[7] * by + Ri[8] * bz;
    const float f = 0.5f / c.posm[s].w;
    float4 a = acc[s];
    a.x += (ax - rx) * f; a.y += (ay - ry) * f; a.z += (az - rz) * f;
    acc[s] = a;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------- launchers
void elastic_build_rest(ElasticState& e, const SphConsts& sc, const ElasticParams& ep, bool lists_only, hipStream_t s) {
    const uint32_t n = (uint32_t)e.n0;
    e.off.ensure((size_t)n + 1);
    if (n == 0) { e.nnz = 0; return; }
    uint32_t nb = 64;
    int bits = 6;
    while (nb < n) { nb <<= 1; ++bits; }
    const uint32_t mask = nb - 1u;
    DevBuf<uint32_t> keys, skeys, idx, sidx, start, cnt;
    keys.ensure(n); skeys.ensure(n); idx.ensure(n); sidx.ensure(n); start.ensure((size_t)nb + 1); cnt.ensure((size_t)n + 1);
    k_el_keys<<<div_up(n, BLOCK), BLOCK, 0, s>>>(n, e.p0.p, sc.h, mask, keys.p, idx.p);
    DevBuf<unsigned char> temp;
    size_t tb = std::max(sort_pairs_temp_bytes(n, bits), scan_temp_bytes(n + 1));
    temp.ensure(tb ? tb : 1);
    sort_pairs(temp.p, tb, keys.p, skeys.p, idx.p, sidx.p, n, bits, s);
    launch_cell_start(skeys.p, n, nb, start.p, s);
    k_el_search<false><<<div_up(n, BLOCK), BLOCK, 0, s>>>(n, e.p0.p, sc.h, sc.h2, mask, start.p, sidx.p, cnt.p, nullptr, nullptr);
    SALVA_HIP_CHECK(hipMemsetAsync(cnt.p + n, 0, sizeof(uint32_t), s));
    SALVA_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(temp.p, tb, cnt.p, e.off.p, (int)(n + 1), s));
    uint32_t total = 0;
    SALVA_HIP_CHECK(hipMemcpyAsync(&total, e.off.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    SALVA_HIP_CHECK(hipStreamSynchronize(s));
    e.nnz = total;
    e.nbr.ensure(total ? total : 1);
    k_el_search<true><<<div_up(n, BLOCK), BLOCK, 0, s>>>(n, e.p0.p, sc.h, sc.h2, mask, start.p, sidx.p, nullptr, e.off.p, e.nbr.p);
    if (!lists_only) {
        if (ep.kd) k_el_volumes0<true><<<div_up(n, BLOCK), BLOCK, 0, s>>>(n, e.p0.p, e.hp.p, e.off.p, e.nbr.p, sc, ep.kd, e.vol0.p);
        else k_el_volumes0<false><<<div_up(n, BLOCK), BLOCK, 0, s>>>(n, e.p0.p, e.hp.p, e.off.p, e.nbr.p, sc, 0, e.vol0.p);
    }
    SALVA_HIP_CHECK(hipStreamSynchronize(s));
    e.list_valid = true;
}

void launch_elastic_gather(const StepCtx& c, uint32_t off, ElasticState& e, hipStream_t s) {
    if (c.n) k_el_gather<<<div_up(c.n, BLOCK), BLOCK, 0, s>>>(c, off, (uint32_t)e.n0, e.hp.p);
}

void launch_elastic_take_rest(ElasticState& e, hipStream_t s) {
    if (e.n0) k_el_take_rest<<<div_up(e.n0, BLOCK), BLOCK, 0, s>>>((uint32_t)e.n0, e.hp.p, e.p0.p);
}

void launch_elastic_identity(ElasticState& e, uint64_t from, uint64_t to, hipStream_t s) {
    if (to > from) k_el_identity<<<div_up(to - from, BLOCK), BLOCK, 0, s>>>((uint32_t)from, (uint32_t)to, e.rot.p);
}

void launch_elastic_rot_stress(const StepCtx& c, ElasticState& e, const ElasticParams& ep, hipStream_t s) {
    const uint32_t n = (uint32_t)e.n0;
    if (!n) return;
    if (ep.kd | ep.kg)
        k_el_rot_stress<true><<<div_up(n, BLOCK), BLOCK, 0, s>>>(c, n, e.hp.p, e.p0.p, e.vol0.p, e.off.p, e.nbr.p, ep, e.rot.p, e.rot_new.p, e.sig.p, e.F.p);
    else
        k_el_rot_stress<false><<<div_up(n, BLOCK), BLOCK, 0, s>>>(c, n, e.hp.p, e.p0.p, e.vol0.p, e.off.p, e.nbr.p, ep, e.rot.p, e.rot_new.p, e.sig.p, e.F.p);
}

void launch_elastic_forces(const StepCtx& c, uint32_t off, ElasticState& e, const ElasticParams& ep, float4* acc, hipStream_t s) {
    if (!c.n || !e.n0) return;
    const uint32_t nn = (uint32_t)e.n0, nblk = div_up(c.n, BLOCK);
    const bool ok = (ep.kd | ep.kg) != 0;
#define SALVA_EL_FORCES(OKV, NLV) \
    k_el_forces<OKV, NLV><<<nblk, BLOCK, 0, s>>>(c, off, nn, e.p0.p, e.vol0.p, e.off.p, e.nbr.p, e.rot_new.p, e.sig.p, e.F.p, ep.kg, acc)
    if (ok) { if (ep.nonlinear) SALVA_EL_FORCES(true, true); else SALVA_EL_FORCES(true, false); }
    else { if (ep.nonlinear) SALVA_EL_FORCES(false, true); else SALVA_EL_FORCES(false, false); }
#undef SALVA_EL_FORCES
}

}  // namespace salva

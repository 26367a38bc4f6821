// vorticity.hip — vorticity confinement (Fedkiw et al. 2001 in the particle form of Macklin & Mueller 2013, section 5) as two
// dependent neighbour passes on the tile skeleton (tile.h).  Not in the reference: the contract is include/salva_hip.h,
// SALVA_HIP_FORCE_VORTICITY_CONFINEMENT, and tests/vorticity_reading.py is its numpy reading.
//
// The force belongs to one fluid and acts between particles of that fluid only; it has no boundary arm.  Velocities are w = v + dv
// (the head of forces.hip), whose .w component carries the model id.
//   pass 1: omega_i = (sum_j m_j (v_i - v_j) x grad W_ij) / rho_i,  n_i = |omega_i|              -> omega[i] = (omega_i, n_i)
//   pass 2: eta_i = sum_j (m_j / rho_j) (n_j - n_i) grad W_ij,  D_i = |eta_i| + (kappa / h) n_i,
//           a_i += eps (eta_i / D_i) x omega_i   unless D_i == 0
// Both stage two 16-byte records per halo slot (32 bytes: two tiles share a CU, the figure k_akinci_normals' comment measured);
// pass 2 adds the 4-byte model id in a world with more than one fluid, where omega's rows of another fluid are that fluid's or
// nothing at all.  The quotient by rho_i, the root and the quotient by D_i are taken once per particle, correctly rounded.
#include "kernels.h"
#include "tile.h"

namespace SALVA_KNS {
using namespace salva;

__global__ __launch_bounds__(TILE_MAX_THREADS) void k_vorticity_curl(StepCtx c, uint32_t model, float4* __restrict__ omega) {
    Tile t;
    t.setup(c);
    if (t.empty()) return;
    uint32_t i0_, gs0_;
    t.first_own(i0_, gs0_);
    const ListOwn lo0_ = list_own(c, i0_, gs0_);  // list head and count: in registers before the staging barrier
    const float4* Lp = nullptr;
    const float4* Lw = nullptr;
    t.stage(c, static_cast<const float4*>(c.posm), static_cast<const float4*>(c.w), Lp, Lw);
    Tile::staged_barrier();
    t.for_own_pre(lo0_, [&](uint32_t i_, uint32_t gs_) { return list_own(c, i_, gs_); }, [&](const ListOwn& lo, uint32_t i, uint32_t gs, bool active) {
        if (!active || c.model[i] != model) return;
        const float4 pi = c.posm[i];
        const float4 vi = c.w[i];
        float cx = 0.f, cy = 0.f, cz = 0.f;
        for_each_ff_regs(c, gs, lo, [&](uint32_t s) { SALVA_PAIR_MATH
            const float4 pj = Lp[s];
            const float4 vj = lds_f4(Lw + s);
            const float dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
            const float g = kernel_grad(dx * dx + dy * dy + dz * dz, c.sc);
            const float sc = (__float_as_uint(vj.w) == model) ? g * pj.w : 0.0f;
            // (the self contact and a coincident twin with the same velocity: u = 0 and d = 0 exactly)
            const float ux = vi.x - vj.x, uy = vi.y - vj.y, uz = vi.z - vj.z;
            cx += (uy * dz - uz * dy) * sc;
            cy += (uz * dx - ux * dz) * sc;
            cz += (ux * dy - uy * dx) * sc;
        });
        const float ri = c.rho[i];
        const float wx = cx / ri, wy = cy / ri, wz = cz / ri;
        omega[i] = make_float4(wx, wy, wz, sqrtf(wx * wx + wy * wy + wz * wz));
    });
}

__global__ __launch_bounds__(TILE_MAX_THREADS) void k_vorticity_confine(StepCtx c, uint32_t model, float eps, float kappa_over_h,
                                                                   const float4* __restrict__ omega) {
    Tile t;
    t.setup(c);
    if (t.empty()) return;
    uint32_t i0_, gs0_;
    t.first_own(i0_, gs0_);
    const ListOwn lo0_ = list_own(c, i0_, gs0_);  // list head and count: in registers before the staging barrier
    const float4* Lp = nullptr;  // (x_j, m_j / rho_j)
    const float4* Lo = nullptr;  // (omega_j, n_j) — only meaningful for particles of `model`, the only ones used
    t.stage(c, static_cast<const float4*>(c.posmr), omega, Lp, Lo);
    const uint32_t* Lm = nullptr;
    if (c.nmodels > 1) t.stage(c, static_cast<const uint32_t*>(c.model), Lm);
    Tile::staged_barrier();
    t.for_own_pre(lo0_, [&](uint32_t i_, uint32_t gs_) { return list_own(c, i_, gs_); }, [&](const ListOwn& lo, uint32_t i, uint32_t gs, bool active) {
        if (!active || c.model[i] != model) return;
        const float4 pi = c.posmr[i];
        const float4 oi = omega[i];
        float ex = 0.f, ey = 0.f, ez = 0.f;
        for_each_ff_regs(c, gs, lo, [&](uint32_t s) { SALVA_PAIR_MATH
            const float4 pj = Lp[s];
            const float4 oj = lds_f4(Lo + s);
            const bool same = Lm ? (Lm[s] == model) : true;
            const float dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
            const float g = kernel_grad(dx * dx + dy * dy + dz * dz, c.sc);
            const float sc = same ? g * pj.w * (oj.w - oi.w) : 0.0f;  // (a select: another fluid's row may hold anything)
            ex += dx * sc; ey += dy * sc; ez += dz * sc;
        });
        const float D = sqrtf(ex * ex + ey * ey + ez * ez) + kappa_over_h * oi.w;
        if (!(D > 0.0f)) return;  // eta = 0 and (kappa = 0 or omega = 0): the numerator is zero too
        const float nx = ex / D, ny = ey / D, nz = ez / D;
        float4 a = c.acc[i];
        a.x += eps * (ny * oi.z - nz * oi.y);
        a.y += eps * (nz * oi.x - nx * oi.z);
        a.z += eps * (nx * oi.y - ny * oi.x);
        c.acc[i] = a;
    });
}

void launch_vorticity_curl(const StepCtx& c, const TileLds& L, uint32_t model, float4* omega, hipStream_t s) {
    SALVA_OK_DISPATCH(launch_vorticity_curl, c, L, model, omega, s);
    SALVA_LAUNCH_TILE(k_vorticity_curl, c, L, L.bytes(32, 0, 2), s, c, model, omega);
}
void launch_vorticity_confine(const StepCtx& c, const TileLds& L, uint32_t model, float eps, float kappa_over_h, const float4* omega,
                              hipStream_t s) {
    SALVA_OK_DISPATCH(launch_vorticity_confine, c, L, model, eps, kappa_over_h, omega, s);
    SALVA_LAUNCH_TILE(k_vorticity_confine, c, L, L.bytes(c.nmodels > 1 ? 36 : 32, 0, 3), s, c, model, eps, kappa_over_h, omega);
}

}  // namespace SALVA_KNS

// Affine finite-horizon LQR: the Riccati sweep of lqr_riccati_kernel.h on the deviation of a nominal that does NOT obey the dynamics
// (include/scpp_hip_lqr.h, scpp_hip_lqr_compute_gains_affine).
//
//   de/dt = A e + B du + c(t),   c = f(x_ref, u_ref) - dx_ref/dt,   V = e'P e + 2 p'e + s
//   -dP/dt = A'P + P A - P B R^-1 B'P + Q            P(T) = Qf
//   -dp/dt = (A - B R^-1 B'P)'p + P c                p(T) = 0
//   -ds/dt = 2 p'c - p'B R^-1 B'p                    s(T) = 0
//   du = -K e - k,   K_k = R^-1 B_k'P(t_k),   k_k = R^-1 B_k'p(t_k)
//
// It is the Riccati equation of the augmented state z = [e; 1]:  A_aug = [[A, c], [0, 0]],  B_aug = [B; 0],  Q_aug = diag(Q, 0),
// P_aug = [[P, p], [p', s]].  nx + 1 <= 15, so P_aug is the ONE 16 x 16 tile of the Riccati kernel, and riccatiRhs is used unchanged: column NX
// of the LDS Jacobian tile carries c, row NX stays zero.  The P block sees the same products as in the Riccati kernel plus p 0 and 0 p, so P and K
// are those of the Riccati sweep; P_aug is symmetric to the bit by the Riccati kernel's argument.
// Mapping: lane r < nx evaluates Jacobian row r as in the Riccati kernel; lane nx, idle there, evaluates the flow map at the same point and writes
// column nx.  The two branches run one after the other in the wave (DESIGN.md 5.2 has what that costs).
#pragma once
#include "lqr_riccati_kernel.h"
#include <utility>

namespace scpp
{
namespace lqr
{

// riccatiJacobian with the defect column: lane NX writes c = f(x, u) - xdot into column NX of the A tile (rows < NX) before the tiles are read back;
// xdot [NX] is the slope of the reference over the segment (read by lane NX only)
template <class P>
__device__ __forceinline__ void affineJacobian(RiccatiLds &lds, int lane, const double *x, const double *u, const double *p, const double *aux,
                                               const double *xdot, double (&At)[4], double (&Bt)[4])
{
    constexpr int NX = P::Model::NX;
    if (lane == NX)
    {
        double f[NX];
        P::Model::template systemFlowMap<double>(x, u, p, f);
#pragma unroll
        for (int j = 0; j < NX; j++)
            lds.A[j * RT + NX] = f[j] - xdot[j];
    }
    riccatiJacobian<P>(lds, lane, x, u, p, aux, At, Bt);
}

// rkf78TileStep (lqr_tile_sweep.h) with the stage loop unrolled by the template instead of by the optimiser: the same expressions in the same
// order, so a tile advanced by either is the same to the bit.  With the flow map next to the Jacobian row, thirteen copies of Rocket2D's stage
// (sin and cos of two angles, twice) pass the size up to which the optimiser honours `#pragma unroll`; the loop then stays a loop, the stage
// slopes are indexed at run time and land in scratch memory (448 bytes per lane).  Here the stage index is a constant by construction.
template <int S, class Rhs>
__device__ __forceinline__ void affineStage(d4_t (&kk)[RK_S], const d4_t &T, double h, Rhs &rhs)
{
    d4_t Ts;
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        double acc = 0.;
#pragma unroll
        for (int qq = 0; qq < S; qq++)
            if (RK_A[S][qq] != 0.)
                acc += RK_A[S][qq] * kk[qq][r];
        Ts[r] = T[r] + h * acc;
    }
    kk[S] = rhs(S, Ts);
}
template <class Rhs, int... S>
__device__ __forceinline__ void affineTileStep(d4_t &T, double h, Rhs &&rhs, std::integer_sequence<int, S...>)
{
    d4_t kk[RK_S];
    (affineStage<S>(kk, T, h, rhs), ...);
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        double acc = 0.;
#pragma unroll
        for (int s = 0; s < RK_S; s++)
            if (RK_B[s] != 0.)
                acc += RK_B[s] * kk[s][r];
        T[r] += h * acc;
    }
}

// One sweep per trajectory; arguments as lqr_riccati_kernel, and  ->  FF [B][K][nu] = k_k, Pout [B][K][nx][nx], pout [B][K][nx], sout [B][K]
// (the three nullptr: not kept).  The reference inside segment i, the stage positions, the node's linearisation point, status, iters and the
// zeroing of failed nodes are the Riccati kernel's; p and s are in the tile, so its finiteness check covers them (a non-finite flow map of a
// finite node fails the node it reaches and every earlier one).
template <class P>
__global__ void __launch_bounds__(WAVE) lqr_affine_kernel(int K, int nU, int uRows, int steps, const double *__restrict__ X, const double *__restrict__ U,
                                                           const double *__restrict__ T, const double *__restrict__ par, int par_stride,
                                                           const double *__restrict__ qw, const double *__restrict__ rw, const double *__restrict__ qfw,
                                                           double *__restrict__ G, int *__restrict__ status, int *__restrict__ iters,
                                                           double *__restrict__ FF, double *__restrict__ Pout, double *__restrict__ pout,
                                                           double *__restrict__ sout)
{
    using Model = typename P::Model;
    using JR = typename Model::JacobianRows;
    constexpr int NX = Model::NX, NU = Model::NU, NP = Model::NP;
    static_assert(NX + 1 <= RT && NU <= 4, "[[P, p], [p', s]] is one 16 x 16 tile, B'P one 4-row chunk");
    __shared__ RiccatiLds lds;
    const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
    const long b = blockIdx.x;
    const bool foh = (nU == K);
    const double *Xb = X + b * K * NX, *Ub = U + b * uRows * NU;
    double *Gb = G + b * K * NU * NX, *Fb = FF + b * K * NU;
    double *Pb = Pout ? Pout + b * K * NX * NX : nullptr;
    double *pb = pout ? pout + b * K * NX : nullptr;
    double *sb = sout ? sout + b * K : nullptr;

    for (int e = lane; e < RT * RT; e += WAVE)
        lds.A[e] = 0.;
    lds.Bm[lane] = 0.;
    double p[NP], aux[JR::NAUX > 0 ? JR::NAUX : 1];
    for (int j = 0; j < NP; j++)
        p[j] = par[b * par_stride + j];
    JR::prepare(p, aux);
    const double rinv = g < NU ? 1. / rw[g < NU ? g : 0] : 0., sr = sqrt(rinv);
    const d4_t qd = diagonalTile<NX>(lane, qw);
    d4_t Pc = diagonalTile<NX>(lane, qfw);
    const double t_max = T[b];
    const int bad = waveOr(referenceNonFinite<NX, NU>(lane, t_max, Xb, Ub, K, nU));
    WAVE_SYNC();

    const double dt = t_max / double(K - 1);
    const double h = dt / double(steps);
    int kfail = bad ? K - 1 : -1; // nodes 0..kfail carry ST_NONFINITE and zeros
    for (int k = K - 1; k >= 0 && kfail < 0; k--)
    {
        if (k < K - 1)
        {
            // ---- segment k: P_aug(t_{k+1}) -> P_aug(t_k), `steps` RKF78 steps ----
            loadSegment<NX, NU>(lds.seg, lane, Xb, Ub, k, foh ? k + 1 : k);
            WAVE_SYNC();
            double xdot[NX];
            if (lane == NX)
            {
#pragma unroll
                for (int j = 0; j < NX; j++)
                    xdot[j] = (lds.seg.x1[j] - lds.seg.x0[j]) / dt;
            }
            for (int n = 0; n < steps; n++)
                affineTileStep(Pc, h, [&](int s, const d4_t Ps) __attribute__((always_inline)) {
                    const double a = 1. - (double(n) + RK_C[s]) / double(steps);
                    double x[NX], u[NU], At[4], Bt[4];
                    if (lane <= NX)
                        interpolateSegment(lds.seg, a, x, u);
                    affineJacobian<P>(lds, lane, x, u, p, aux, xdot, At, Bt);
                    return riccatiRhs(Ps, At, Bt, sr, qd);
                }, std::make_integer_sequence<int, RK_S>{});
        }
        // ---- node k: [K_k | k_k] = R^-1 B_k'[P | p](t_k), B_k at (X[k], U[min(k, nU-1)]) ----
        double x[NX], u[NU], At[4], Bt[4];
        const int ku = k < nU ? k : nU - 1;
        if (lane < NX)
        {
#pragma unroll
            for (int j = 0; j < NX; j++)
                x[j] = Xb[k * NX + j];
#pragma unroll
            for (int j = 0; j < NU; j++)
                u[j] = Ub[ku * NU + j];
        }
        riccatiJacobian<P>(lds, lane, x, u, p, aux, At, Bt);
        d4_t Wt = {0., 0., 0., 0.};
#pragma unroll
        for (int c = 0; c < 4; c++)
            Wt = __builtin_amdgcn_mfma_f64_16x16x4f64(Bt[c], Pc[c], Wt, 0, 0, 0);
        const double gain = rinv * Wt[0]; // lane (g, col): K[g][col], col == NX: k[g]
        int nf = isFinite(gain) ? 0 : 1;
#pragma unroll
        for (int r = 0; r < 4; r++)
            nf |= isFinite(Pc[r]) ? 0 : 1;
        if (waveOr(nf))
        {
            kfail = k;
            break;
        }
        if (g < NU && col < NX)
            Gb[(k * NU + g) * NX + col] = gain;
        if (g < NU && col == NX)
            Fb[k * NU + g] = gain;
        if (Pb)
            storeTile<NX>(lane, Pb + k * NX * NX, Pc);
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (4 * r + g == NX) // row NX of the tile: [p' | s]
            {
                if (pb && col < NX)
                    pb[k * NX + col] = Pc[r];
                if (sb && col == NX)
                    sb[k] = Pc[r];
            }
        if (lane == 0)
        {
            status[b * K + k] = ST_OK;
            iters[b * K + k] = (K - 1 - k) * steps;
        }
    }
    // a failed node never writes a non-finite value: zeros and its status, for the node the tile went non-finite at and every earlier one
    for (int e = lane; e < (kfail + 1) * NU * NX; e += WAVE)
        Gb[e] = 0.;
    for (int e = lane; e < (kfail + 1) * NU; e += WAVE)
        Fb[e] = 0.;
    if (Pb)
        for (int e = lane; e < (kfail + 1) * NX * NX; e += WAVE)
            Pb[e] = 0.;
    if (pb)
        for (int e = lane; e < (kfail + 1) * NX; e += WAVE)
            pb[e] = 0.;
    if (sb)
        for (int e = lane; e <= kfail; e += WAVE)
            sb[e] = 0.;
    for (int e = lane; e <= kfail; e += WAVE)
    {
        status[b * K + e] = ST_NONFINITE;
        iters[b * K + e] = 0;
    }
}

} // namespace lqr
} // namespace scpp

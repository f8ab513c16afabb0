// Closed-loop mean next to the covariance: the covariance sweep of lqr_covariance_kernel.h on the state z = [e; 1] (include/scpp_hip_lqr.h,
// scpp_hip_lqr_propagate_moments).
//
//   dS/dt = A_cl S + S A_cl' + W      S(0) = S0        A_cl = A - B K_t
//   dm/dt = A_cl m + d(t)             m(0) = mean0     d = c - [B k_t],   c = f(x_ref, u_ref) - dx_ref/dt
//   mean correction of node k: du_mean[k] = -G[k] m(t_k) - [ff[k]]
//
// The tile is T = [[S, m], [m', 0]] (nx + 1 <= 15) in the accumulator layout.  closedLoopJacobian and covarianceRhs are the covariance kernel's,
// unchanged: row and column NX of the LDS A_cl tile stay zero, so A_cl T + T A_cl' is [[A_cl S + S A_cl', A_cl m], [(A_cl m)', 0]] and the S block
// sees the covariance kernel's products plus 0 m' and m 0: S, and everything recorded from it, is that of the covariance sweep.  d enters OUTSIDE
// the products: the lanes that hold column NX (rows < NX) and row NX (columns < NX) add it to their slope, both from the same LDS value, so the
// tile stays symmetric to the bit by the covariance kernel's argument; m is downloaded from column NX.  S + m m' is never formed.
// Mapping: lane r < nx evaluates Jacobian row r inside closedLoopJacobian as in the covariance kernel and, with feedforward terms, once more for
// -B_r k_t (closedLoopJacobian does not hand its row out); lane nx, idle there, evaluates the flow map at the same point and writes c.
#pragma once
#include "lqr_covariance_kernel.h"
#include <utility>

namespace scpp
{
namespace lqr
{

struct MomentsLds
{
    CovarianceLds cov;
    double dc[RT], db[RT]; // c and -B k_t of the stage, rows >= nx zero
    double f0[4], f1[4];   // feedforward terms of the segment's two nodes (the gain's indices)
};

// rkf78TileStep with the stage loop unrolled by the template (lqr_affine_kernel.h, affineTileStep, says why): the same expressions in the same order
template <int S, class Rhs>
__device__ __forceinline__ void momentsStage(d4_t (&kk)[RK_S], const d4_t &T, double h, Rhs &rhs)
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
__device__ __forceinline__ void momentsTileStep(d4_t &T, double h, Rhs &&rhs, std::integer_sequence<int, S...>)
{
    d4_t kk[RK_S];
    (momentsStage<S>(kk, T, h, rhs), ...);
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

// the drive of the mean at the reference's point a of the segment -> LDS: lane NX writes c = f(x, u) - xdot (xdot [NX]: the slope of the reference
// over the segment, read by lane NX only), lanes r < NX write -B_r k_t = ((0 - B_r0 k_0) - B_r1 k_1) - ..., k_t = f0 + a (f1 - f0) (ff only; zero
// otherwise).  The caller synchronises before it reads.
template <class P>
__device__ __forceinline__ void momentsDrive(MomentsLds &lds, int lane, double a, const double *p, const double *aux, const double *xdot, bool ff)
{
    constexpr int NX = P::Model::NX, NU = P::Model::NU;
    if (lane == NX)
    {
        double x[NX], u[NU], f[NX];
        interpolateSegment(lds.cov.seg, a, x, u);
        P::Model::template systemFlowMap<double>(x, u, p, f);
#pragma unroll
        for (int j = 0; j < NX; j++)
            lds.dc[j] = f[j] - xdot[j];
    }
    else if (lane < NX && ff)
    {
        double x[NX], u[NU], jr[NX + NU];
        interpolateSegment(lds.cov.seg, a, x, u);
        jacobianRow<P>(lane, x, u, p, aux, jr);
        double acc = 0.;
#pragma unroll
        for (int q = 0; q < NU; q++)
            acc -= jr[NX + q] * (lds.f0[q] + a * (lds.f1[q] - lds.f0[q]));
        lds.db[lane] = acc;
    }
}

// One sweep per trajectory; arguments as lqr_covariance_kernel, and FF [B][K][nu] (nullptr: no feedforward term, d = c), M0 [B][nx] (nullptr:
// mean0 = 0; m0_stride 0: one row for every trajectory)  ->  mean [B][K][nx] = m(t_k), dumean [B][K][nu] = -G[k] m(t_k) - [FF[k]].
// The reference inside segment i, the stage positions, the status and the zeroing of failed nodes are the covariance kernel's; m is in the
// tile, so its finiteness check covers it (a non-finite flow map at a finite point fails the node it reaches and every later one).
template <class P>
__global__ void __launch_bounds__(WAVE) lqr_moments_kernel(int K, int nU, int uRows, int steps, const double *__restrict__ X, const double *__restrict__ U,
                                                            const double *__restrict__ T, const double *__restrict__ par, int par_stride,
                                                            const double *__restrict__ G, const int *__restrict__ gstatus,
                                                            const double *__restrict__ S0, int s0_stride, const double *__restrict__ w,
                                                            const double *__restrict__ FF, const double *__restrict__ M0, int m0_stride,
                                                            double *__restrict__ sd, double *__restrict__ icov, double *__restrict__ fcov,
                                                            int *__restrict__ status, double *__restrict__ cov, double *__restrict__ mean,
                                                            double *__restrict__ dumean)
{
    using Model = typename P::Model;
    using JR = typename Model::JacobianRows;
    constexpr int NX = Model::NX, NU = Model::NU, NP = Model::NP;
    static_assert(NX + 1 <= RT && NU <= 4, "[[S, m], [m', 0]] is one 16 x 16 tile, the gain one 4-row chunk");
    __shared__ MomentsLds lds;
    const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
    const long b = blockIdx.x;
    const bool foh = (nU == K), ff = FF != nullptr;
    const double *Xb = X + b * K * NX, *Ub = U + b * uRows * NU, *Gb = G + b * K * NU * NX;
    const double *Fb = ff ? FF + b * K * NU : nullptr;
    double *sdb = sd + b * K * NX, *icb = icov + b * K * NU * NU, *fcb = fcov + b * NX * NX;
    double *cvb = cov ? cov + b * K * NX * NX : nullptr;
    double *mb = mean + b * K * NX, *dub = dumean + b * K * NU;

    for (int e = lane; e < RT * RT; e += WAVE)
        lds.cov.At[e] = 0.;
    if (lane < RT)
        lds.dc[lane] = lds.db[lane] = 0.;
    double p[NP], aux[JR::NAUX > 0 ? JR::NAUX : 1];
    for (int j = 0; j < NP; j++)
        p[j] = par[b * par_stride + j];
    JR::prepare(p, aux);
    const d4_t wd = diagonalTile<NX>(lane, w);
    d4_t Tc;
    int bad = 0;
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        const int row = 4 * r + g;
        const bool in = row < NX && col < NX;
        const int mi = (col == NX && row < NX) ? row : ((row == NX && col < NX) ? col : -1); // the entry of m this register holds
        double v = in ? S0[b * s0_stride + (in ? row * NX + col : 0)] : 0.;
        if (mi >= 0 && M0)
        {
            v = M0[b * m0_stride + mi];
            bad |= isFinite(v) ? 0 : 1;
        }
        Tc[r] = v;
    }
    const double t_max = T[b];
    int incomplete = 0;
    bad |= referenceNonFinite<NX, NU>(lane, t_max, Xb, Ub, K, nU);
    for (int e = lane; e < K * NU * NX; e += WAVE)
        bad |= isFinite(Gb[e]) ? 0 : 1;
    if (ff)
        for (int e = lane; e < K * NU; e += WAVE)
            bad |= isFinite(Fb[e]) ? 0 : 1;
    if (gstatus)
        for (int e = lane; e < K; e += WAVE)
            incomplete |= gstatus[b * K + e] != ST_OK ? 1 : 0;
    bad = waveOr(bad);
    incomplete = waveOr(incomplete);
    WAVE_SYNC();

    const double dt = t_max / double(K - 1);
    const double h = dt / double(steps);
    int kfail = bad ? 0 : K; // nodes kfail..K-1 carry zeros
    for (int k = 0; k < K && kfail == K; k++)
    {
        if (k > 0)
        {
            // ---- segment i = k-1: T(t_i) -> T(t_k), `steps` RKF78 steps ----
            const int i = k - 1, ju = foh ? k : i;
            loadSegment<NX, NU>(lds.cov.seg, lane, Xb, Ub, i, ju);
            if (g < NU && col < NX)
            {
                lds.cov.G0[g * RT + col] = Gb[(i * NU + g) * NX + col];
                lds.cov.G1[g * RT + col] = Gb[(ju * NU + g) * NX + col];
            }
            if (ff && lane < NU)
            {
                lds.f0[lane] = Fb[i * NU + lane];
                lds.f1[lane] = Fb[ju * NU + lane];
            }
            WAVE_SYNC();
            double xdot[NX];
            if (lane == NX)
            {
#pragma unroll
                for (int j = 0; j < NX; j++)
                    xdot[j] = (lds.cov.seg.x1[j] - lds.cov.seg.x0[j]) / dt;
            }
            for (int n = 0; n < steps; n++)
                momentsTileStep(Tc, h, [&](int s, const d4_t Ts) __attribute__((always_inline)) {
                    const double a = (double(n) + RK_C[s]) / double(steps);
                    double Ac[4];
                    momentsDrive<P>(lds, lane, a, p, aux, xdot, ff);
                    closedLoopJacobian<P>(lds.cov, lane, a, p, aux, Ac); // synchronises after its writes and after its reads
                    d4_t F = covarianceRhs(Ts, Ac, wd);
#pragma unroll
                    for (int r = 0; r < 4; r++)
                    {
                        const int row = 4 * r + g;
                        const int mi = (col == NX && row < NX) ? row : ((row == NX && col < NX) ? col : -1);
                        if (mi >= 0)
                            F[r] += lds.dc[mi] + lds.db[mi]; // d = c + (-B k_t)
                    }
                    WAVE_SYNC(); // the next stage writes dc and db
                    return F;
                }, std::make_integer_sequence<int, RK_S>{});
        }
        // ---- node k: T(t_k); S G' carries (G m)' in row NX, G (S G') is the input covariance (8 matrix-core instructions) ----
        double Gt[4]; // the lane's share of the gain tile (rows >= nu and column NX zero): G[col][4c + g]
#pragma unroll
        for (int c = 0; c < 4; c++)
        {
            const bool in = col < NU && 4 * c + g < NX;
            Gt[c] = in ? Gb[(k * NU + (in ? col : 0)) * NX + (in ? 4 * c + g : 0)] : 0.;
        }
        d4_t Wp = {0., 0., 0., 0.}, Sk = {0., 0., 0., 0.};
#pragma unroll
        for (int c = 0; c < 4; c++)
            Wp = __builtin_amdgcn_mfma_f64_16x16x4f64(Tc[c], Gt[c], Wp, 0, 0, 0); // T G': register r of lane l is (T G')[4r + g][col]
#pragma unroll
        for (int c = 0; c < 4; c++)
            Sk = __builtin_amdgcn_mfma_f64_16x16x4f64(Gt[c], Wp[c], Sk, 0, 0, 0); // register 0 of lane l is (G S G')[g][col]
        double du = 0.; // the lane of row NX, column q < nu: du_mean[k][q]
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (4 * r + g == NX && col < NU)
                du = ff ? -Wp[r] - Fb[k * NU + col] : -Wp[r];
        int nf = (isFinite(Sk[0]) && isFinite(du)) ? 0 : 1;
#pragma unroll
        for (int r = 0; r < 4; r++)
            nf |= isFinite(Tc[r]) ? 0 : 1;
        if (waveOr(nf))
        {
            kfail = k;
            break;
        }
        if (cvb)
            storeTile<NX>(lane, cvb + k * NX * NX, Tc);
#pragma unroll
        for (int r = 0; r < 4; r++)
        {
            if (4 * r + g == col && col < NX)
                sdb[k * NX + col] = sqrt(Tc[r] > 0. ? Tc[r] : 0.); // a diagonal entry negative from rounding: 0
            if (col == NX && 4 * r + g < NX)
                mb[k * NX + 4 * r + g] = Tc[r];
            if (4 * r + g == NX && col < NU)
                dub[k * NU + col] = du;
        }
        if (g < NU && col < NU)
            icb[(k * NU + g) * NU + col] = Sk[0];
    }
    // nothing non-finite is ever written: zeros for the node the tile went non-finite at and every later one (every node of a non-finite trajectory)
    for (int e = kfail * NX + lane; e < K * NX; e += WAVE)
        sdb[e] = mb[e] = 0.;
    for (int e = kfail * NU * NU + lane; e < K * NU * NU; e += WAVE)
        icb[e] = 0.;
    for (int e = kfail * NU + lane; e < K * NU; e += WAVE)
        dub[e] = 0.;
    if (cvb)
        for (int e = kfail * NX * NX + lane; e < K * NX * NX; e += WAVE)
            cvb[e] = 0.;
    const d4_t zero = {0., 0., 0., 0.};
    storeTile<NX>(lane, fcb, kfail == K ? Tc : zero);
    if (lane == 0)
        status[b] = kfail < K ? ST_NONFINITE : (incomplete ? ST_GAINS_INCOMPLETE : ST_OK);
}

} // namespace lqr
} // namespace scpp

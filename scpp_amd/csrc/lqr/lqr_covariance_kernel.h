// Linear covariance analysis: the closed-loop state covariance swept forwards along every trajectory (include/scpp_hip_lqr.h,
// scpp_hip_lqr_propagate_covariance).
//
//   dS/dt = A_cl(t) S + S A_cl(t)' + W,   S(0) = S0,   A_cl(t) = A(t) - B(t) K(t),   input covariance of node k: G[k] S(t_k) G[k]'
//
// Mapping: that of lqr_riccati_kernel.h.  ONE WAVEFRONT PER TRAJECTORY; S, padded with zeros, is one 16 x 16 FP64 tile in the accumulator layout of
// v_mfma_f64_16x16x4_f64 (lane l, register r: row (l >> 4) + 4 r, column l & 15), and so is each of the 13 RKF78 stage slopes.  S being symmetric,
// register c of lane l is the lane's share of chunk c of the B operand (S[4c + g][col]) and of the A operand (S[col][4c + g]) alike.  Lane r < nx
// evaluates row r of [A | B] at the stage's reference, forms row r of A_cl = A - B K_t (nu nx FMAs, K_t interpolated from an LDS copy of the
// segment's two node gains) and writes it to a zero-padded LDS tile, which is kept TRANSPOSED (the row goes down a column: consecutive lanes,
// consecutive addresses), so that the read-back in the accumulator pattern, At[(4c + g)][col] = A_cl[col][4c + g], is the lane's share of the A
// operand of A_cl S and of the B operand of S A_cl' alike.  A right-hand side is eight matrix-core instructions and no lane exchange:
//     M1 = A_cl S     4   (A operand: A_cl, B operand: S)
//     M2 = S A_cl'    4   (A operand: S, B operand: A_cl)     M2[i][j] is bitwise M1[j][i]: the same products, summed in the same order
//     F  = (M1 + M2) + W
// S STAYS SYMMETRIC BY CONSTRUCTION (bitwise); nothing is symmetrised.
#pragma once
#include "lqr_riccati_kernel.h"

namespace scpp
{
namespace lqr
{

constexpr int ST_GAINS_INCOMPLETE = 2;

struct CovarianceLds
{
    double At[RT * RT];         // At[c][r] = A_cl[r][c]; rows and columns >= nx stay zero
    double G0[4 * RT], G1[4 * RT]; // gains of the segment's two nodes, [a][c]
    double x0[RT], x1[RT], u0[4], u1[4];
};

// F = (A_cl S + S A_cl') + W in the accumulator layout; Ac = the lane's share of the transposed A_cl tile, wd = its share of W
__device__ __forceinline__ d4_t covarianceRhs(const d4_t Sn, const double (&Ac)[4], const d4_t wd)
{
    d4_t M1 = {0., 0., 0., 0.}, M2 = {0., 0., 0., 0.};
#pragma unroll
    for (int c = 0; c < 4; c++)
        M1 = __builtin_amdgcn_mfma_f64_16x16x4f64(Ac[c], Sn[c], M1, 0, 0, 0);
#pragma unroll
    for (int c = 0; c < 4; c++)
        M2 = __builtin_amdgcn_mfma_f64_16x16x4f64(Sn[c], Ac[c], M2, 0, 0, 0);
    d4_t F;
#pragma unroll
    for (int r = 0; r < 4; r++)
        F[r] = (M1[r] + M2[r]) + wd[r];
    return F;
}

// One sweep per trajectory.  X [B][K][nx], U [B][uRows][nu] (nU rows used), T [B], par [B][np], G [B][K][nu][nx], gstatus [B][K] (nullptr: gains
// without a status), S0 [B][nx][nx] (s0_stride 0: one matrix for every trajectory), w [nx]  ->  sd [B][K][nx] = sqrt(diag S(t_k)),
// icov [B][K][nu][nu] = G[k] S(t_k) G[k]', fcov [B][nx][nx] = S(T), status [B], cov [B][K][nx][nx] (nullptr: not kept).
// Segment i (nodes i, i+1) is integrated from a = 0 up to a = 1 with x = X[i] + a (X[i+1] - X[i]), u = U[i] + a (U[j] - U[i]),
// K_t = G[i] + a (G[j] - G[i]), j = i+1 (first-order) or i (zero-order); the segment index is the loop's, never derived from a time.
template <class P>
__global__ void __launch_bounds__(WAVE) lqr_covariance_kernel(int K, int nU, int uRows, int steps, const double *__restrict__ X, const double *__restrict__ U,
                                                               const double *__restrict__ T, const double *__restrict__ par, int par_stride,
                                                               const double *__restrict__ G, const int *__restrict__ gstatus,
                                                               const double *__restrict__ S0, int s0_stride, const double *__restrict__ w,
                                                               double *__restrict__ sd, double *__restrict__ icov, double *__restrict__ fcov,
                                                               int *__restrict__ status, double *__restrict__ cov)
{
    using Model = typename P::Model;
    using JR = typename Model::JacobianRows;
    constexpr int NX = Model::NX, NU = Model::NU, NP = Model::NP;
    static_assert(NX <= RT && NU <= 4, "S is one 16 x 16 tile, the gain one 4-row chunk");
    __shared__ CovarianceLds lds;
    const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
    const long b = blockIdx.x;
    const bool foh = (nU == K);
    const double *Xb = X + b * K * NX, *Ub = U + b * uRows * NU, *Gb = G + b * K * NU * NX;
    double *sdb = sd + b * K * NX, *icb = icov + b * K * NU * NU, *fcb = fcov + b * NX * NX;
    double *cvb = cov ? cov + b * K * NX * NX : nullptr;

    for (int e = lane; e < RT * RT; e += WAVE)
        lds.At[e] = 0.;
    double p[NP], aux[JR::NAUX > 0 ? JR::NAUX : 1];
    for (int j = 0; j < NP; j++)
        p[j] = par[b * par_stride + j];
    JR::prepare(p, aux);
    d4_t wd, Sc;
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        const int row = 4 * r + g;
        const bool in = row < NX && col < NX;
        wd[r] = (in && row == col) ? w[in ? col : 0] : 0.;
        Sc[r] = in ? S0[b * s0_stride + (in ? row * NX + col : 0)] : 0.;
    }
    const double t_max = T[b];
    int bad = isFinite(t_max) ? 0 : 1, incomplete = 0;
    for (int e = lane; e < K * NX; e += WAVE)
        bad |= isFinite(Xb[e]) ? 0 : 1;
    for (int e = lane; e < nU * NU; e += WAVE)
        bad |= isFinite(Ub[e]) ? 0 : 1;
    for (int e = lane; e < K * NU * NX; e += WAVE)
        bad |= isFinite(Gb[e]) ? 0 : 1;
    if (gstatus)
        for (int e = lane; e < K; e += WAVE)
            incomplete |= gstatus[b * K + e] != ST_OK ? 1 : 0;
    bad = waveOr(bad);
    incomplete = waveOr(incomplete);
    WAVE_SYNC();

    const double h = t_max / double(K - 1) / double(steps);
    int kfail = bad ? 0 : K; // nodes kfail..K-1 carry zeros
    for (int k = 0; k < K && kfail == K; k++)
    {
        if (k > 0)
        {
            // ---- segment i = k-1: S(t_i) -> S(t_k), `steps` RKF78 steps ----
            const int i = k - 1, ju = foh ? k : i;
            if (lane < NX)
            {
                lds.x0[lane] = Xb[i * NX + lane];
                lds.x1[lane] = Xb[k * NX + lane];
            }
            if (lane < NU)
            {
                lds.u0[lane] = Ub[i * NU + lane];
                lds.u1[lane] = Ub[ju * NU + lane];
            }
            if (g < NU && col < NX)
            {
                lds.G0[g * RT + col] = Gb[(i * NU + g) * NX + col];
                lds.G1[g * RT + col] = Gb[(ju * NU + g) * NX + col];
            }
            WAVE_SYNC();
            for (int n = 0; n < steps; n++)
            {
                d4_t kk[RK_S];
#pragma unroll
                for (int s = 0; s < RK_S; s++)
                {
                    const double a = (double(n) + RK_C[s]) / double(steps);
                    if (lane < NX)
                    {
                        double x[NX], u[NU], uaux[JR::NUAUX > 0 ? JR::NUAUX : 1], jr[NX + NU];
#pragma unroll
                        for (int j = 0; j < NX; j++)
                            x[j] = lds.x0[j] + a * (lds.x1[j] - lds.x0[j]);
#pragma unroll
                        for (int j = 0; j < NU; j++)
                            u[j] = lds.u0[j] + a * (lds.u1[j] - lds.u0[j]);
                        JR::prepareInput(u, p, uaux);
                        (void)JR::row(lane, x, u, p, aux, uaux, jr);
#pragma unroll
                        for (int c = 0; c < NX; c++)
                        {
                            double acl = jr[c];
#pragma unroll
                            for (int q = 0; q < NU; q++)
                                acl -= jr[NX + q] * (lds.G0[q * RT + c] + a * (lds.G1[q * RT + c] - lds.G0[q * RT + c]));
                            lds.At[c * RT + lane] = acl;
                        }
                    }
                    WAVE_SYNC();
                    double Ac[4];
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        Ac[c] = lds.At[(4 * c + g) * RT + col];
                    WAVE_SYNC();
                    d4_t Ss;
#pragma unroll
                    for (int r = 0; r < 4; r++)
                    {
                        double acc = 0.;
#pragma unroll
                        for (int qq = 0; qq < s; qq++)
                            if (RK_A[s][qq] != 0.)
                                acc += RK_A[s][qq] * kk[qq][r];
                        Ss[r] = Sc[r] + h * acc;
                    }
                    kk[s] = covarianceRhs(Ss, Ac, wd);
                }
#pragma unroll
                for (int r = 0; r < 4; r++)
                {
                    double acc = 0.;
#pragma unroll
                    for (int s = 0; s < RK_S; s++)
                        if (RK_B[s] != 0.)
                            acc += RK_B[s] * kk[s][r];
                    Sc[r] += h * acc;
                }
            }
        }
        // ---- node k: S(t_k), its standard deviations and the input covariance G[k] S G[k]' = G (S G')  (8 matrix-core instructions) ----
        double Gt[4]; // the lane's share of the gain tile (rows >= nu zero): G[col][4c + g]
#pragma unroll
        for (int c = 0; c < 4; c++)
        {
            const bool in = col < NU && 4 * c + g < NX;
            Gt[c] = in ? Gb[(k * NU + (in ? col : 0)) * NX + (in ? 4 * c + g : 0)] : 0.;
        }
        d4_t Wp = {0., 0., 0., 0.}, Sk = {0., 0., 0., 0.};
#pragma unroll
        for (int c = 0; c < 4; c++)
            Wp = __builtin_amdgcn_mfma_f64_16x16x4f64(Sc[c], Gt[c], Wp, 0, 0, 0); // S G': register r of lane l is (S G')[4r + g][col]
#pragma unroll
        for (int c = 0; c < 4; c++)
            Sk = __builtin_amdgcn_mfma_f64_16x16x4f64(Gt[c], Wp[c], Sk, 0, 0, 0); // register 0 of lane l is (G S G')[g][col]
        int nf = isFinite(Sk[0]) ? 0 : 1;
#pragma unroll
        for (int r = 0; r < 4; r++)
            nf |= isFinite(Sc[r]) ? 0 : 1;
        if (waveOr(nf))
        {
            kfail = k;
            break;
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
        {
            const int row = 4 * r + g;
            if (row < NX && col < NX)
            {
                if (cvb)
                    cvb[(k * NX + row) * NX + col] = Sc[r];
                if (row == col)
                    sdb[k * NX + col] = sqrt(Sc[r] > 0. ? Sc[r] : 0.); // a diagonal entry negative from rounding: 0
            }
        }
        if (g < NU && col < NU)
            icb[(k * NU + g) * NU + col] = Sk[0];
    }
    // nothing non-finite is ever written: zeros for the node S went non-finite at and every later one (every node of a non-finite trajectory)
    for (int e = kfail * NX + lane; e < K * NX; e += WAVE)
        sdb[e] = 0.;
    for (int e = kfail * NU * NU + lane; e < K * NU * NU; e += WAVE)
        icb[e] = 0.;
    if (cvb)
        for (int e = kfail * NX * NX + lane; e < K * NX * NX; e += WAVE)
            cvb[e] = 0.;
#pragma unroll
    for (int r = 0; r < 4; r++)
        if (4 * r + g < NX && col < NX)
            fcb[(4 * r + g) * NX + col] = kfail == K ? Sc[r] : 0.;
    if (lane == 0)
        status[b] = kfail < K ? ST_NONFINITE : (incomplete ? ST_GAINS_INCOMPLETE : ST_OK);
}

} // namespace lqr
} // namespace scpp

// Linear covariance analysis: the closed-loop state covariance swept forwards along every trajectory (include/scpp_hip_lqr.h,
// scpp_hip_lqr_propagate_covariance).
//
//   dS/dt = A_cl(t) S + S A_cl(t)' + W,   S(0) = S0,   A_cl(t) = A(t) - B(t) K(t),   input covariance of node k: G[k] S(t_k) G[k]'
//
// Mapping: ONE WAVEFRONT PER TRAJECTORY, S one 16 x 16 FP64 tile in the accumulator layout (lqr_tile_sweep.h).  Lane r < nx
// evaluates row r of [A | B] at the stage's reference, forms row r of A_cl = A - B K_t (nu nx FMAs, K_t interpolated from an LDS copy of the
// segment's two node gains) and writes it to a zero-padded LDS tile, which is kept TRANSPOSED (the row goes down a column: consecutive lanes,
// consecutive addresses), so that the read-back in the accumulator pattern, At[(4c + g)][col] = A_cl[col][4c + g], is the lane's share of the A
// operand of A_cl S and of the B operand of S A_cl' alike.  A right-hand side is eight matrix-core instructions and no lane exchange:
//     M1 = A_cl S     4   (A operand: A_cl, B operand: S)
//     M2 = S A_cl'    4   (A operand: S, B operand: A_cl)     M2[i][j] is bitwise M1[j][i]: the same products, summed in the same order
//     F  = (M1 + M2) + W
// S STAYS SYMMETRIC BY CONSTRUCTION (bitwise); nothing is symmetrised.
#pragma once
#include "lqr_tile_sweep.h"

namespace scpp
{
namespace lqr
{

constexpr int ST_GAINS_INCOMPLETE = 2;

struct CovarianceLds
{
    double At[RT * RT];         // At[c][r] = A_cl[r][c]; rows and columns >= nx stay zero
    double G0[4 * RT], G1[4 * RT]; // gains of the segment's two nodes, [a][c]
    SegmentLds seg;
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

// lane r < NX: row r of A_cl = A - B K_t at the reference's point a of the segment -> LDS, transposed; afterwards every lane holds its share of the tile
template <class P>
__device__ __forceinline__ void closedLoopJacobian(CovarianceLds &lds, int lane, double a, const double *p, const double *aux, double (&Ac)[4])
{
    constexpr int NX = P::Model::NX, NU = P::Model::NU;
    const int g = lane >> 4, col = lane & 15;
    if (lane < NX)
    {
        double x[NX], u[NU], jr[NX + NU];
        interpolateSegment(lds.seg, a, x, u);
        jacobianRow<P>(lane, x, u, p, aux, jr);
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
#pragma unroll
    for (int c = 0; c < 4; c++)
        Ac[c] = lds.At[(4 * c + g) * RT + col];
    WAVE_SYNC();
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
    const d4_t wd = diagonalTile<NX>(lane, w);
    d4_t Sc;
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        const int row = 4 * r + g;
        const bool in = row < NX && col < NX;
        Sc[r] = in ? S0[b * s0_stride + (in ? row * NX + col : 0)] : 0.;
    }
    const double t_max = T[b];
    int bad = referenceNonFinite<NX, NU>(lane, t_max, Xb, Ub, K, nU), incomplete = 0;
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
            loadSegment<NX, NU>(lds.seg, lane, Xb, Ub, i, ju);
            if (g < NU && col < NX)
            {
                lds.G0[g * RT + col] = Gb[(i * NU + g) * NX + col];
                lds.G1[g * RT + col] = Gb[(ju * NU + g) * NX + col];
            }
            WAVE_SYNC();
            for (int n = 0; n < steps; n++)
                rkf78TileStep(Sc, h, [&](int s, const d4_t Ss) __attribute__((always_inline)) {
                    const double a = (double(n) + RK_C[s]) / double(steps);
                    double Ac[4];
                    closedLoopJacobian<P>(lds, lane, a, p, aux, Ac);
                    return covarianceRhs(Ss, Ac, wd);
                });
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
        if (cvb)
            storeTile<NX>(lane, cvb + k * NX * NX, Sc);
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (4 * r + g == col && col < NX)
                sdb[k * NX + col] = sqrt(Sc[r] > 0. ? Sc[r] : 0.); // a diagonal entry negative from rounding: 0
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
    const d4_t zero = {0., 0., 0., 0.};
    storeTile<NX>(lane, fcb, kfail == K ? Sc : zero);
    if (lane == 0)
        status[b] = kfail < K ? ST_NONFINITE : (incomplete ? ST_GAINS_INCOMPLETE : ST_OK);
}

} // namespace lqr
} // namespace scpp

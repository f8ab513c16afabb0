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
//
// The moments sweep (lqr_moments_kernel.h has its equations) is THE SAME BODY, covarianceSweep<P, MEAN = true>: the tile is [[S, m], [m', 0]],
// and what the mean adds stands under `if constexpr (MEAN)`.  Its entry point is compiled in a translation unit of its own (lqr_sweep_launch.h).
#pragma once
#include "lqr_sweep_frame.h"

namespace scpp
{
namespace lqr
{

struct CovarianceLds
{
    double At[RT * RT];         // At[c][r] = A_cl[r][c]; rows and columns >= nx stay zero
    double G0[4 * RT], G1[4 * RT]; // gains of the segment's two nodes, [a][c]
    SegmentLds seg;
};

struct MomentsLds
{
    CovarianceLds cov;
    double dc[RT], db[RT]; // c and -B k_t of the stage, rows >= nx zero
    double f0[4], f1[4];   // feedforward terms of the segment's two nodes (the gain's indices)
};

__device__ __forceinline__ CovarianceLds &covarianceLds(CovarianceLds &lds) { return lds; }
__device__ __forceinline__ CovarianceLds &covarianceLds(MomentsLds &lds) { return lds.cov; }

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

// One sweep per trajectory.  X [B][K][nx], U [B][uRows][nu] (nU rows used), T [B], par [B][np], G [B][K][nu][nx], gstatus [B][K] (nullptr: gains
// without a status), S0 [B][nx][nx] (s0_stride 0: one matrix for every trajectory), w [nx]  ->  sd [B][K][nx] = sqrt(diag S(t_k)),
// icov [B][K][nu][nu] = G[k] S(t_k) G[k]', fcov [B][nx][nx] = S(T), status [B], cov [B][K][nx][nx] (nullptr: not kept).
// MEAN: and FF [B][K][nu] (nullptr: no feedforward term, d = c), M0 [B][nx] (nullptr: mean0 = 0; m0_stride 0: one row for every trajectory)
// ->  mean [B][K][nx] = m(t_k), dumean [B][K][nu] = -G[k] m(t_k) - [FF[k]]; m is in the tile, so the frame's finiteness check covers it (a
// non-finite flow map at a finite point fails the node it reaches and every later one).  Lds: CovarianceLds, or MomentsLds with MEAN.
// Segment i (nodes i, i+1) is integrated from a = 0 up to a = 1 with x = X[i] + a (X[i+1] - X[i]), u = U[i] + a (U[j] - U[i]),
// K_t = G[i] + a (G[j] - G[i]), j = i+1 (first-order) or i (zero-order); the segment index is the loop's, never derived from a time.
template <class P, bool MEAN, class Lds>
__device__ __forceinline__ void covarianceSweep(Lds &mlds, int K, int nU, int uRows, int steps, const double *__restrict__ X, const double *__restrict__ U,
                                                const double *__restrict__ T, const double *__restrict__ par, int par_stride,
                                                const double *__restrict__ G, const int *__restrict__ gstatus, const double *__restrict__ S0,
                                                int s0_stride, const double *__restrict__ w, const double *__restrict__ FF,
                                                const double *__restrict__ M0, int m0_stride, double *__restrict__ sd, double *__restrict__ icov,
                                                double *__restrict__ fcov, int *__restrict__ status, double *__restrict__ cov,
                                                double *__restrict__ mean, double *__restrict__ dumean)
{
    using Model = typename P::Model;
    using JR = typename Model::JacobianRows;
    constexpr int NX = Model::NX, NU = Model::NU, NP = Model::NP;
    static_assert(NX + (MEAN ? 1 : 0) <= RT && NU <= 4, "S, or [[S, m], [m', 0]], is one 16 x 16 tile, the gain one 4-row chunk");
    CovarianceLds &lds = covarianceLds(mlds);
    const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
    const long b = blockIdx.x;
    const bool foh = (nU == K), ff = MEAN && FF != nullptr;
    const double *Xb = X + b * K * NX, *Ub = U + b * uRows * NU;
    const ForwardIo io = forwardIo<NX, NU>(b, K, G, FF, sd, icov, fcov, cov, mean, dumean);

    for (int e = lane; e < RT * RT; e += WAVE)
        lds.At[e] = 0.;
    if constexpr (MEAN)
        if (lane < RT)
            mlds.dc[lane] = mlds.db[lane] = 0.;
    double p[NP], aux[JR::NAUX > 0 ? JR::NAUX : 1];
    loadParameters<P>(par, b, par_stride, p, aux);
    const d4_t wd = diagonalTile<NX>(lane, w);
    int bad = 0, incomplete;
    d4_t Tc = loadInitialTile<NX, MEAN>(lane, S0 + b * s0_stride, (MEAN && M0) ? M0 + b * m0_stride : nullptr, bad);
    const double t_max = T[b];
    scanForwardInputs<NX, NU, MEAN>(lane, t_max, Xb, Ub, K, nU, io, gstatus ? gstatus + b * K : nullptr, bad, incomplete);
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
            loadSegment<NX, NU>(lds.seg, lane, Xb, Ub, i, ju);
            if (g < NU && col < NX)
            {
                lds.G0[g * RT + col] = io.Gb[(i * NU + g) * NX + col];
                lds.G1[g * RT + col] = io.Gb[(ju * NU + g) * NX + col];
            }
            if constexpr (MEAN)
                if (ff && lane < NU)
                {
                    mlds.f0[lane] = io.Fb[i * NU + lane];
                    mlds.f1[lane] = io.Fb[ju * NU + lane];
                }
            WAVE_SYNC();
            [[maybe_unused]] double xdot[NX];
            if constexpr (MEAN)
                if (lane == NX)
                {
#pragma unroll
                    for (int j = 0; j < NX; j++)
                        xdot[j] = (lds.seg.x1[j] - lds.seg.x0[j]) / dt;
                }
            for (int n = 0; n < steps; n++)
                rkf78TileStep(Tc, h, [&](int s, const d4_t Ts) __attribute__((always_inline)) {
                    const double a = (double(n) + RK_C[s]) / double(steps);
                    double Ac[4];
                    if constexpr (MEAN)
                        momentsDrive<P>(mlds, lane, a, p, aux, xdot, ff);
                    closedLoopJacobian<P>(lds, lane, a, p, aux, Ac); // synchronises after its writes and after its reads
                    d4_t F = covarianceRhs(Ts, Ac, wd);
                    if constexpr (MEAN)
                    {
                        // d = c + (-B k_t) enters OUTSIDE the products: column NX and row NX add it from the same LDS value
#pragma unroll
                        for (int r = 0; r < 4; r++)
                        {
                            const int mi = meanIndex<NX>(4 * r + g, col);
                            if (mi >= 0)
                                F[r] += mlds.dc[mi] + mlds.db[mi];
                        }
                        WAVE_SYNC(); // the next stage writes dc and db
                    }
                    return F;
                });
        }
        if (!forwardNode<NX, NU, MEAN>(lane, k, Tc, io))
        {
            kfail = k;
            break;
        }
    }
    forwardEpilogue<NX, NU, MEAN>(lane, K, kfail, incomplete, Tc, io, status + b);
}

template <class P>
__global__ void __launch_bounds__(WAVE) lqr_covariance_kernel(int K, int nU, int uRows, int steps, const double *__restrict__ X, const double *__restrict__ U,
                                                               const double *__restrict__ T, const double *__restrict__ par, int par_stride,
                                                               const double *__restrict__ G, const int *__restrict__ gstatus,
                                                               const double *__restrict__ S0, int s0_stride, const double *__restrict__ w,
                                                               double *__restrict__ sd, double *__restrict__ icov, double *__restrict__ fcov,
                                                               int *__restrict__ status, double *__restrict__ cov)
{
    __shared__ CovarianceLds lds;
    covarianceSweep<P, false>(lds, K, nU, uRows, steps, X, U, T, par, par_stride, G, gstatus, S0, s0_stride, w, nullptr, nullptr, 0, sd, icov, fcov,
                              status, cov, nullptr, nullptr);
}

} // namespace lqr
} // namespace scpp

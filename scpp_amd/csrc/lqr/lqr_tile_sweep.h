// What the matrix sweeps along a trajectory share (lqr_riccati_kernel.h and lqr_discrete_kernel.h backwards, lqr_covariance_kernel.h and
// lqr_covariance_discrete_kernel.h forwards): the tile layout, the reference segment in LDS, the Jacobian row of a lane, one RKF78
// step of a tile, the scan of the reference and two tile helpers.  The frame around a sweep (start, node, failure tail) is lqr_sweep_frame.h.
//
// THE TILE LAYOUT (stated here, referred to by both kernels).  ONE WAVEFRONT PER TRAJECTORY.  nx <= 14, so a symmetric nx x nx matrix M, padded with
// zeros, is one 16 x 16 FP64 tile, kept in the accumulator layout of v_mfma_f64_16x16x4_f64 (lane l, register r: row (l >> 4) + 4 r, column l & 15):
// 4 doubles per lane for M and for each of the 13 RKF78 stage slopes.  With g = l >> 4 and col = l & 15, register c of lane l is at once the lane's
// share of chunk c of the B operand (M[4c + g][col]) and, M being symmetric, of the A operand (M[col][4c + g]); the same holds for a 16 x 16 tile
// read back from LDS as tile[(4c + g) * RT + col].  Products of such tiles are therefore matrix-core instructions with no lane exchange.
#pragma once
#include "lqr_kernels.h"
#include <utility>

namespace scpp
{
namespace lqr
{

constexpr int RT = 16; // tile edge

__device__ __forceinline__ int waveOr(int v)
{
    for (int m = WAVE / 2; m >= 1; m >>= 1)
        v |= __shfl_xor(v, m);
    return v;
}

// ---- the reference over one segment: nodes i and i+1, inputs i and ju ----
struct SegmentLds
{
    double x0[RT], x1[RT], u0[4], u1[4];
};

// ju = i+1 (first-order hold) or i (zero-order hold); the caller synchronises the wave before the first interpolation
template <int NX, int NU>
__device__ __forceinline__ void loadSegment(SegmentLds &seg, int lane, const double *Xb, const double *Ub, int i, int ju)
{
    if (lane < NX)
    {
        seg.x0[lane] = Xb[i * NX + lane];
        seg.x1[lane] = Xb[(i + 1) * NX + lane];
    }
    if (lane < NU)
    {
        seg.u0[lane] = Ub[i * NU + lane];
        seg.u1[lane] = Ub[ju * NU + lane];
    }
}

// x = x0 + a (x1 - x0), u = u0 + a (u1 - u0)
template <int NX, int NU>
__device__ __forceinline__ void interpolateSegment(const SegmentLds &seg, double a, double (&x)[NX], double (&u)[NU])
{
#pragma unroll
    for (int j = 0; j < NX; j++)
        x[j] = seg.x0[j] + a * (seg.x1[j] - seg.x0[j]);
#pragma unroll
    for (int j = 0; j < NU; j++)
        u[j] = seg.u0[j] + a * (seg.u1[j] - seg.u0[j]);
}

// row r of [A | B] at (x, u): the generated rows the gain kernel evaluates; aux from JacobianRows::prepare(p, aux)
template <class P>
__device__ __forceinline__ void jacobianRow(int r, const double *x, const double *u, const double *p, const double *aux,
                                            double (&jr)[P::Model::NX + P::Model::NU])
{
    using JR = typename P::Model::JacobianRows;
    double uaux[JR::NUAUX > 0 ? JR::NUAUX : 1];
    JR::prepareInput(u, p, uaux);
    (void)JR::row(r, x, u, p, aux, uaux, jr);
}

// One fixed RKF78 step of a tile: T <- T + h sum_s b_s k_s, k_s = rhs(s, T + h sum_q a_sq k_q).  rhs is the caller's lambda (forced inline).
// The stage loop is unrolled by the template, not by the optimiser, so the stage index is a constant by construction and the 13 slopes stay in
// registers.  `#pragma unroll` does not promise that: with the flow map next to the Jacobian row (the affine and the moments sweep), thirteen
// copies of Rocket2D's stage (sin and cos of two angles, twice) pass the size up to which the optimiser honours the pragma; the loop then stays a
// loop, the stage slopes are indexed at run time and land in scratch memory (448 bytes per lane).
template <int S, class Rhs>
__device__ __forceinline__ void rkf78TileStage(d4_t (&kk)[RK_S], const d4_t &T, double h, Rhs &rhs)
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
__device__ __forceinline__ void rkf78TileStages(d4_t &T, double h, Rhs &rhs, std::integer_sequence<int, S...>)
{
    d4_t kk[RK_S];
    (rkf78TileStage<S>(kk, T, h, rhs), ...);
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
template <class Rhs>
__device__ __forceinline__ void rkf78TileStep(d4_t &T, double h, Rhs &&rhs)
{
    rkf78TileStages(T, h, rhs, std::make_integer_sequence<int, RK_S>{});
}

// The same step for N tiles that advance together (the filter sweep: the error covariance and the covariance of the estimate): rhs(s, Ts, F) fills
// the N slopes F from the N stage tiles Ts.  Element for element the arithmetic of rkf78TileStep, so a tile whose slope does not depend on its
// neighbours comes out bitwise as rkf78TileStep leaves it; 13 N slope tiles stay in registers by the same unrolling.
template <int S, int N, class Rhs>
__device__ __forceinline__ void rkf78TilesStage(d4_t (&kk)[N][RK_S], const d4_t (&T)[N], double h, Rhs &rhs)
{
    d4_t Ts[N], F[N];
#pragma unroll
    for (int t = 0; t < N; t++)
#pragma unroll
        for (int r = 0; r < 4; r++)
        {
            double acc = 0.;
#pragma unroll
            for (int qq = 0; qq < S; qq++)
                if (RK_A[S][qq] != 0.)
                    acc += RK_A[S][qq] * kk[t][qq][r];
            Ts[t][r] = T[t][r] + h * acc;
        }
    rhs(S, Ts, F);
#pragma unroll
    for (int t = 0; t < N; t++)
        kk[t][S] = F[t];
}
template <int N, class Rhs, int... S>
__device__ __forceinline__ void rkf78TilesStages(d4_t (&T)[N], double h, Rhs &rhs, std::integer_sequence<int, S...>)
{
    d4_t kk[N][RK_S];
    (rkf78TilesStage<S, N>(kk, T, h, rhs), ...);
#pragma unroll
    for (int t = 0; t < N; t++)
#pragma unroll
        for (int r = 0; r < 4; r++)
        {
            double acc = 0.;
#pragma unroll
            for (int s = 0; s < RK_S; s++)
                if (RK_B[s] != 0.)
                    acc += RK_B[s] * kk[t][s][r];
            T[t][r] += h * acc;
        }
}
template <int N, class Rhs>
__device__ __forceinline__ void rkf78TilesStep(d4_t (&T)[N], double h, Rhs &&rhs)
{
    rkf78TilesStages<N>(T, h, rhs, std::make_integer_sequence<int, RK_S>{});
}

// this lane's finding about the trajectory's inputs: 1 when the final time, a state or an input is not finite (the caller reduces with waveOr)
template <int NX, int NU>
__device__ __forceinline__ int referenceNonFinite(int lane, double t_max, const double *Xb, const double *Ub, int K, int nU)
{
    int bad = isFinite(t_max) ? 0 : 1;
    for (int e = lane; e < K * NX; e += WAVE)
        bad |= isFinite(Xb[e]) ? 0 : 1;
    for (int e = lane; e < nU * NU; e += WAVE)
        bad |= isFinite(Ub[e]) ? 0 : 1;
    return bad;
}

// the lane's share of diag(d), d [NX]
template <int NX>
__device__ __forceinline__ d4_t diagonalTile(int lane, const double *d)
{
    const int g = lane >> 4, col = lane & 15;
    d4_t D;
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        const bool diag = (4 * r + g == col) && col < NX;
        D[r] = diag ? d[diag ? col : 0] : 0.;
    }
    return D;
}

// the NX x NX corner of a tile -> dst [NX][NX]
template <int NX>
__device__ __forceinline__ void storeTile(int lane, double *dst, const d4_t M)
{
    const int g = lane >> 4, col = lane & 15;
#pragma unroll
    for (int r = 0; r < 4; r++)
        if (4 * r + g < NX && col < NX)
            dst[(4 * r + g) * NX + col] = M[r];
}

} // namespace lqr
} // namespace scpp

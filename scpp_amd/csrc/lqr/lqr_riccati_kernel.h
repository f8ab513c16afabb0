// Finite-horizon LQR: the differential Riccati equation swept backwards along every trajectory (include/scpp_hip_lqr.h,
// scpp_hip_lqr_compute_gains_riccati).
//
//   -dP/dt = A(t)'P + P A(t) - P B(t) R^-1 B(t)'P + Q,   P(T) = Qf,   K_k = R^-1 B_k' P(t_k)
//
// Mapping: ONE WAVEFRONT PER TRAJECTORY, P one 16 x 16 FP64 tile in the accumulator layout (lqr_tile_sweep.h: register c of a lane is its share of
// the A operand and of the B operand alike, for P and for the Jacobian tile read back from LDS).  A right-hand side is therefore thirteen
// matrix-core instructions and no lane exchange:
//     M1 = P A        4   (A operand: P, B operand: A)
//     M2 = A'P        4   (A operand: A, B operand: P)        M2[i][j] is bitwise M1[j][i]: the same products, summed in the same order
//     W' = B'P        4   (rows 0..nu-1; register 0 of lane l is W[col][g])
//     S  = (W R^-1/2)(W R^-1/2)'   1   (both operands the same register, so S is bitwise symmetric)
//     F  = (M1 + M2) - S + Q
// P STAYS SYMMETRIC BY CONSTRUCTION (bitwise: F[i][j] and F[j][i] are the same operations on the same numbers); nothing is symmetrised.
// The Jacobian rows are the generated rows the gain kernel evaluates: lane r < nx evaluates row r at the interpolated reference and writes it to LDS.
//
// The affine sweep (lqr_affine_kernel.h has its equations) is THE SAME BODY, riccatiSweep<P, AFFINE = true>, on the tile [[P, p], [p', s]]; what
// it adds stands under `if constexpr (AFFINE)`.  Its entry point is compiled in a translation unit of its own (lqr_sweep_launch.h).
#pragma once
#include "lqr_sweep_frame.h"

namespace scpp
{
namespace lqr
{

struct RiccatiLds
{
    double A[RT * RT]; // rows and columns >= nx stay zero
    double Bm[RT * 4]; // rows >= nx, columns >= nu stay zero
    SegmentLds seg;
};

// lane r < NX: row r of [A | B] at (x, u) -> LDS; afterwards every lane holds its share of both tiles
template <class P>
__device__ __forceinline__ void riccatiJacobian(RiccatiLds &lds, int lane, const double *x, const double *u, const double *p, const double *aux,
                                                double (&At)[4], double (&Bt)[4])
{
    constexpr int NX = P::Model::NX, NU = P::Model::NU;
    const int g = lane >> 4, col = lane & 15;
    if (lane < NX)
    {
        double jr[NX + NU];
        jacobianRow<P>(lane, x, u, p, aux, jr);
#pragma unroll
        for (int c = 0; c < NX; c++)
            lds.A[lane * RT + c] = jr[c];
#pragma unroll
        for (int a = 0; a < NU; a++)
            lds.Bm[lane * 4 + a] = jr[NX + a];
    }
    WAVE_SYNC();
#pragma unroll
    for (int c = 0; c < 4; c++)
    {
        At[c] = lds.A[(4 * c + g) * RT + col];
        Bt[c] = lds.Bm[(4 * c + g) * 4 + (col & 3)];
        if (col >= NU)
            Bt[c] = 0.;
    }
    WAVE_SYNC();
}

// F = (P A + A'P) - (P B R^-1/2)(P B R^-1/2)' + Q in the accumulator layout; sr = sqrt(1 / r[g]) (0 for g >= nu), qd = the lane's share of Q
__device__ __forceinline__ d4_t riccatiRhs(const d4_t Pn, const double (&At)[4], const double (&Bt)[4], double sr, const d4_t qd)
{
    d4_t M1 = {0., 0., 0., 0.}, M2 = {0., 0., 0., 0.}, Wt = {0., 0., 0., 0.}, S = {0., 0., 0., 0.};
#pragma unroll
    for (int c = 0; c < 4; c++)
        M1 = __builtin_amdgcn_mfma_f64_16x16x4f64(Pn[c], At[c], M1, 0, 0, 0);
#pragma unroll
    for (int c = 0; c < 4; c++)
        M2 = __builtin_amdgcn_mfma_f64_16x16x4f64(At[c], Pn[c], M2, 0, 0, 0);
#pragma unroll
    for (int c = 0; c < 4; c++)
        Wt = __builtin_amdgcn_mfma_f64_16x16x4f64(Bt[c], Pn[c], Wt, 0, 0, 0);
    const double s = Wt[0] * sr;
    S = __builtin_amdgcn_mfma_f64_16x16x4f64(s, s, S, 0, 0, 0);
    d4_t F;
#pragma unroll
    for (int r = 0; r < 4; r++)
        F[r] = (M1[r] + M2[r]) - S[r] + qd[r];
    return F;
}

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

// One sweep per trajectory.  X [B][K][nx], U [B][uRows][nu] (nU rows used: K first-order hold, K-1 zero-order hold), T [B], par [B][np], q / qf [nx],
// r [nu]  ->  G [B][K][nu][nx], status [B][K], iters [B][K] = RKF78 steps behind the node, Pout [B][K][nx][nx] (nullptr: not kept).
// AFFINE: and  ->  FF [B][K][nu] = k_k, pout [B][K][nx], sout [B][K] (the two nullptr: not kept); p and s are in the tile, so the finiteness
// check covers them (a non-finite flow map of a finite node fails the node it reaches and every earlier one).
// Segment i (nodes i, i+1) is integrated from a = 1 down to a = 0 with the reference x = X[i] + a (X[i+1] - X[i]), u = U[i] + a (U[j] - U[i]),
// j = i+1 (first-order) or i (zero-order); the segment index is the loop's, never derived from a time.
template <class P, bool AFFINE>
__device__ __forceinline__ void riccatiSweep(RiccatiLds &lds, int K, int nU, int uRows, int steps, const double *__restrict__ X,
                                             const double *__restrict__ U, const double *__restrict__ T, const double *__restrict__ par, int par_stride,
                                             const double *__restrict__ qw, const double *__restrict__ rw, const double *__restrict__ qfw,
                                             double *__restrict__ G, int *__restrict__ status, int *__restrict__ iters, double *__restrict__ FF,
                                             double *__restrict__ Pout, double *__restrict__ pout, double *__restrict__ sout)
{
    using Model = typename P::Model;
    using JR = typename Model::JacobianRows;
    constexpr int NX = Model::NX, NU = Model::NU, NP = Model::NP;
    static_assert(NX + (AFFINE ? 1 : 0) <= RT && NU <= 4, "P, or [[P, p], [p', s]], is one 16 x 16 tile, B'P one 4-row chunk");
    const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
    const long b = blockIdx.x;
    const bool foh = (nU == K);
    const double *Xb = X + b * K * NX, *Ub = U + b * uRows * NU;
    double *Gb = G + b * K * NU * NX;
    double *Pb = Pout ? Pout + b * K * NX * NX : nullptr;
    [[maybe_unused]] double *Fb = AFFINE ? FF + b * K * NU : nullptr;
    [[maybe_unused]] double *pb = (AFFINE && pout) ? pout + b * K * NX : nullptr;
    [[maybe_unused]] double *sb = (AFFINE && sout) ? sout + b * K : nullptr;

    for (int e = lane; e < RT * RT; e += WAVE)
        lds.A[e] = 0.;
    lds.Bm[lane] = 0.;
    double p[NP], aux[JR::NAUX > 0 ? JR::NAUX : 1];
    loadParameters<P>(par, b, par_stride, p, aux);
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
            // ---- segment k: the tile from t_{k+1} to t_k, `steps` RKF78 steps ----
            loadSegment<NX, NU>(lds.seg, lane, Xb, Ub, k, foh ? k + 1 : k);
            WAVE_SYNC();
            [[maybe_unused]] double xdot[NX];
            if constexpr (AFFINE)
                if (lane == NX)
                {
#pragma unroll
                    for (int j = 0; j < NX; j++)
                        xdot[j] = (lds.seg.x1[j] - lds.seg.x0[j]) / dt;
                }
            for (int n = 0; n < steps; n++)
                rkf78TileStep(Pc, h, [&](int s, const d4_t Ps) __attribute__((always_inline)) {
                    const double a = 1. - (double(n) + RK_C[s]) / double(steps);
                    double x[NX], u[NU], At[4], Bt[4];
                    if (lane < NX + (AFFINE ? 1 : 0)) // AFFINE: lane NX evaluates the flow map at the same point
                        interpolateSegment(lds.seg, a, x, u);
                    if constexpr (AFFINE)
                        affineJacobian<P>(lds, lane, x, u, p, aux, xdot, At, Bt);
                    else
                        riccatiJacobian<P>(lds, lane, x, u, p, aux, At, Bt);
                    return riccatiRhs(Ps, At, Bt, sr, qd);
                });
        }
        // ---- node k: K_k = R^-1 B_k'P(t_k), B_k at (X[k], U[min(k, nU-1)]): the frozen-time kernel's linearisation point ----
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
        const double gain = rinv * Wt[0]; // lane (g, col): K[g][col]; AFFINE, col == NX: k[g]
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
        if (Pb)
            storeTile<NX>(lane, Pb + k * NX * NX, Pc);
        if constexpr (AFFINE)
        {
            if (g < NU && col == NX)
                Fb[k * NU + g] = gain;
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (4 * r + g == NX) // row NX of the tile: [p' | s]
                {
                    if (pb && col < NX)
                        pb[k * NX + col] = Pc[r];
                    if (sb && col == NX)
                        sb[k] = Pc[r];
                }
        }
        markNodeOk(lane, status + b * K, iters + b * K, k, (K - 1 - k) * steps);
    }
    // a failed node never writes a non-finite value: zeros and its status, for the node the tile went non-finite at and every earlier one
    backwardEpilogue<NX, NU>(lane, kfail, Gb, Pb, status + b * K, iters + b * K);
    if constexpr (AFFINE)
    {
        for (int e = lane; e < (kfail + 1) * NU; e += WAVE)
            Fb[e] = 0.;
        if (pb)
            for (int e = lane; e < (kfail + 1) * NX; e += WAVE)
                pb[e] = 0.;
        if (sb)
            for (int e = lane; e <= kfail; e += WAVE)
                sb[e] = 0.;
    }
}

template <class P>
__global__ void __launch_bounds__(WAVE) lqr_riccati_kernel(int K, int nU, int uRows, int steps, const double *__restrict__ X, const double *__restrict__ U,
                                                            const double *__restrict__ T, const double *__restrict__ par, int par_stride,
                                                            const double *__restrict__ qw, const double *__restrict__ rw, const double *__restrict__ qfw,
                                                            double *__restrict__ G, int *__restrict__ status, int *__restrict__ iters,
                                                            double *__restrict__ Pout)
{
    __shared__ RiccatiLds lds;
    riccatiSweep<P, false>(lds, K, nU, uRows, steps, X, U, T, par, par_stride, qw, rw, qfw, G, status, iters, nullptr, Pout, nullptr, nullptr);
}

} // namespace lqr
} // namespace scpp

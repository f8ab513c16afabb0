// Finite-horizon LQR: the differential Riccati equation swept backwards along every trajectory (include/scpp_hip_lqr.h,
// scpp_hip_lqr_compute_gains_riccati).
//
//   -dP/dt = A(t)'P + P A(t) - P B(t) R^-1 B(t)'P + Q,   P(T) = Qf,   K_k = R^-1 B_k' P(t_k)
//
// Mapping: ONE WAVEFRONT PER TRAJECTORY.  nx <= 14, so P, padded with zeros, is one 16 x 16 FP64 tile, kept in the accumulator layout of
// v_mfma_f64_16x16x4_f64 (lane l, register r: row (l >> 4) + 4 r, column l & 15): 4 doubles per lane for P and for each of the 13 RKF78 stage
// slopes.  In that layout register c of lane l is at once the lane's share of chunk c of the B operand (P[4c + g][col]) and, P being symmetric, of
// the A operand (P[col][4c + g]), and the same holds for the Jacobian tile read back from LDS.  A right-hand side is therefore thirteen
// matrix-core instructions and no lane exchange:
//     M1 = P A        4   (A operand: P, B operand: A)
//     M2 = A'P        4   (A operand: A, B operand: P)        M2[i][j] is bitwise M1[j][i]: the same products, summed in the same order
//     W' = B'P        4   (rows 0..nu-1; register 0 of lane l is W[col][g])
//     S  = (W R^-1/2)(W R^-1/2)'   1   (both operands the same register, so S is bitwise symmetric)
//     F  = (M1 + M2) - S + Q
// P STAYS SYMMETRIC BY CONSTRUCTION (bitwise: F[i][j] and F[j][i] are the same operations on the same numbers); nothing is symmetrised.
// The Jacobian rows are the generated rows the gain kernel evaluates: lane r < nx evaluates row r at the interpolated reference and writes it to LDS.
#pragma once
#include "lqr_kernels.h"

namespace scpp
{
namespace lqr
{

constexpr int RT = 16; // tile edge

struct RiccatiLds
{
    double A[RT * RT]; // rows and columns >= nx stay zero
    double Bm[RT * 4]; // rows >= nx, columns >= nu stay zero
    double x0[RT], x1[RT], u0[4], u1[4];
};

__device__ __forceinline__ int waveOr(int v)
{
    for (int m = WAVE / 2; m >= 1; m >>= 1)
        v |= __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ bool isFinite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// lane r < NX: row r of [A | B] at (x, u) -> LDS; afterwards every lane holds its share of both tiles
template <class P>
__device__ __forceinline__ void riccatiJacobian(RiccatiLds &lds, int lane, const double *x, const double *u, const double *p, const double *aux,
                                                double (&At)[4], double (&Bt)[4])
{
    using Model = typename P::Model;
    using JR = typename Model::JacobianRows;
    constexpr int NX = Model::NX, NU = Model::NU;
    const int g = lane >> 4, col = lane & 15;
    if (lane < NX)
    {
        double uaux[JR::NUAUX > 0 ? JR::NUAUX : 1], jr[NX + NU];
        JR::prepareInput(u, p, uaux);
        (void)JR::row(lane, x, u, p, aux, uaux, jr);
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

// One sweep per trajectory.  X [B][K][nx], U [B][uRows][nu] (nU rows used: K first-order hold, K-1 zero-order hold), T [B], par [B][np], q / qf [nx],
// r [nu]  ->  G [B][K][nu][nx], status [B][K], iters [B][K] = RKF78 steps behind the node, Pout [B][K][nx][nx] (nullptr: not kept).
// Segment i (nodes i, i+1) is integrated from a = 1 down to a = 0 with the reference x = X[i] + a (X[i+1] - X[i]), u = U[i] + a (U[j] - U[i]),
// j = i+1 (first-order) or i (zero-order); the segment index is the loop's, never derived from a time.
template <class P>
__global__ void __launch_bounds__(WAVE) lqr_riccati_kernel(int K, int nU, int uRows, int steps, const double *__restrict__ X, const double *__restrict__ U,
                                                            const double *__restrict__ T, const double *__restrict__ par, int par_stride,
                                                            const double *__restrict__ qw, const double *__restrict__ rw, const double *__restrict__ qfw,
                                                            double *__restrict__ G, int *__restrict__ status, int *__restrict__ iters,
                                                            double *__restrict__ Pout)
{
    using Model = typename P::Model;
    using JR = typename Model::JacobianRows;
    constexpr int NX = Model::NX, NU = Model::NU, NP = Model::NP;
    static_assert(NX <= RT && NU <= 4, "P is one 16 x 16 tile, B'P one 4-row chunk");
    __shared__ RiccatiLds lds;
    const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
    const long b = blockIdx.x;
    const bool foh = (nU == K);
    const double *Xb = X + b * K * NX, *Ub = U + b * uRows * NU;
    double *Gb = G + b * K * NU * NX;
    double *Pb = Pout ? Pout + b * K * NX * NX : nullptr;

    for (int e = lane; e < RT * RT; e += WAVE)
        lds.A[e] = 0.;
    lds.Bm[lane] = 0.;
    double p[NP], aux[JR::NAUX > 0 ? JR::NAUX : 1];
    for (int j = 0; j < NP; j++)
        p[j] = par[b * par_stride + j];
    JR::prepare(p, aux);
    const double rinv = g < NU ? 1. / rw[g < NU ? g : 0] : 0., sr = sqrt(rinv);
    d4_t qd, Pc;
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        const bool diag = (4 * r + g == col) && col < NX;
        qd[r] = diag ? qw[diag ? col : 0] : 0.;
        Pc[r] = diag ? qfw[diag ? col : 0] : 0.;
    }
    const double t_max = T[b];
    int bad = isFinite(t_max) ? 0 : 1;
    for (int e = lane; e < K * NX; e += WAVE)
        bad |= isFinite(Xb[e]) ? 0 : 1;
    for (int e = lane; e < nU * NU; e += WAVE)
        bad |= isFinite(Ub[e]) ? 0 : 1;
    bad = waveOr(bad);
    WAVE_SYNC();

    const double h = t_max / double(K - 1) / double(steps);
    int kfail = bad ? K - 1 : -1; // nodes 0..kfail carry ST_NONFINITE and zeros
    for (int k = K - 1; k >= 0 && kfail < 0; k--)
    {
        if (k < K - 1)
        {
            // ---- segment k: P(t_{k+1}) -> P(t_k), `steps` RKF78 steps ----
            const int ju = foh ? k + 1 : k;
            if (lane < NX)
            {
                lds.x0[lane] = Xb[k * NX + lane];
                lds.x1[lane] = Xb[(k + 1) * NX + lane];
            }
            if (lane < NU)
            {
                lds.u0[lane] = Ub[k * NU + lane];
                lds.u1[lane] = Ub[ju * NU + lane];
            }
            WAVE_SYNC();
            for (int n = 0; n < steps; n++)
            {
                d4_t kk[RK_S];
#pragma unroll
                for (int s = 0; s < RK_S; s++)
                {
                    const double a = 1. - (double(n) + RK_C[s]) / double(steps);
                    double x[NX], u[NU], At[4], Bt[4];
                    if (lane < NX)
                    {
#pragma unroll
                        for (int j = 0; j < NX; j++)
                            x[j] = lds.x0[j] + a * (lds.x1[j] - lds.x0[j]);
#pragma unroll
                        for (int j = 0; j < NU; j++)
                            u[j] = lds.u0[j] + a * (lds.u1[j] - lds.u0[j]);
                    }
                    riccatiJacobian<P>(lds, lane, x, u, p, aux, At, Bt);
                    d4_t Ps;
#pragma unroll
                    for (int r = 0; r < 4; r++)
                    {
                        double acc = 0.;
#pragma unroll
                        for (int qq = 0; qq < s; qq++)
                            if (RK_A[s][qq] != 0.)
                                acc += RK_A[s][qq] * kk[qq][r];
                        Ps[r] = Pc[r] + h * acc;
                    }
                    kk[s] = riccatiRhs(Ps, At, Bt, sr, qd);
                }
#pragma unroll
                for (int r = 0; r < 4; r++)
                {
                    double acc = 0.;
#pragma unroll
                    for (int s = 0; s < RK_S; s++)
                        if (RK_B[s] != 0.)
                            acc += RK_B[s] * kk[s][r];
                    Pc[r] += h * acc;
                }
            }
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
        const double gain = rinv * Wt[0]; // lane (g, col): K[g][col]
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
        {
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (4 * r + g < NX && col < NX)
                    Pb[(k * NX + 4 * r + g) * NX + col] = Pc[r];
        }
        if (lane == 0)
        {
            status[b * K + k] = ST_OK;
            iters[b * K + k] = (K - 1 - k) * steps;
        }
    }
    // a failed node never writes a non-finite gain: zeros and its status, for the node P went non-finite at and every earlier one
    for (int e = lane; e < (kfail + 1) * NU * NX; e += WAVE)
        Gb[e] = 0.;
    if (Pb)
        for (int e = lane; e < (kfail + 1) * NX * NX; e += WAVE)
            Pb[e] = 0.;
    for (int e = lane; e <= kfail; e += WAVE)
    {
        status[b * K + e] = ST_NONFINITE;
        iters[b * K + e] = 0;
    }
}

} // namespace lqr
} // namespace scpp

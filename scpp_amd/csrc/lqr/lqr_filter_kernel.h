// LQG along every trajectory: the Kalman-Bucy error covariance swept forwards and, with LOOP, the covariance of the estimate under the
// output-feedback loop du = -K_t e^ (include/scpp_hip_lqr.h, scpp_hip_lqr_filter).  Measurement y = H e + v, H [ny][nx] constant and
// one for all trajectories, v white with intensity V = diag(v), v_m > 0;  eps = e - e^:
//
//   dSg/dt = A Sg + Sg A' + W - Sg H' V^-1 H Sg     Sg(0) = S0      L(t) = Sg H' V^-1                    (A: the OPEN-loop Jacobian)
//   dXh/dt = A_cl Xh + Xh A_cl' + Sg H' V^-1 H Sg   Xh(0) = 0       A_cl = A - B K_t                     (LOOP)
//   state covariance of the loop: Sg + Xh (E[e^ eps'] = 0),   covariance of the commanded correction at node k: G[k] Xh(t_k) G[k]'
//
// Mapping: ONE WAVEFRONT PER TRAJECTORY, Sg and Xh one 16 x 16 FP64 tile each in the accumulator layout (lqr_tile_sweep.h); both advance in ONE
// RKF78 step (rkf78TilesStep).  Lane r < nx evaluates row r of [A | B] once per stage and writes row r of A and (LOOP) of A_cl, transposed, to
// two zero-padded LDS tiles, as closedLoopJacobian does for one.  A right-hand side is 16 matrix-core instructions (LOOP: 24), no lane exchange:
//     M1 + M2 + W       8   covarianceRhs(Sg, A, W), called, not restated: Sg is symmetric to the bit, and with H = 0 bitwise the covariance
//                           sweep's S under zero gains
//     Y  = H Sg         4   A operand of lane (g, col), chunk c: H[col][4c + g], zero outside ny x nx, loaded once per kernel
//     Ys[r] = Y[r] sqrt(1 / v[4r + g])
//     S  = Ys' Ys       4   both operands the same registers (mfma(X, Y) = X'Y): S is symmetric to the bit
//     F  = (M1 + M2 + W) - S
//     F^ = covarianceRhs(Xh, A_cl, 0) + S     8   (LOOP)
// Node k: one more H Sg (4), L_k[j][m] = Y[m][j] / v[m], error_std = sqrt diag Sg; LOOP: state_std = sqrt diag(Sg + Xh) and G Xh G' (8).
// Failure rules: the forward frame's (lqr_sweep_frame.h).  A gain L_k that overflows fails its node like a non-finite tile.
//
// Registers, from the compiler's kernel-resource-usage report (hipcc -O3 -ffp-contract=on, gfx950).  Twenty-six slope tiles are 208 registers
// per lane, which does not fit the 256 of two wavefronts per SIMD (lqr_covariance_discrete_kernel.h), so the kernel is compiled and launched for
// ONE wavefront per SIMD, __launch_bounds__(64, 1): 512 registers per lane.
// No scratch and no vector-register spill for any variant; scalar values the compiler parks in lanes of a vector register (its "SGPRs Spill")
// never touch memory.  Without LOOP (13 slopes) the compiler stays below 256 registers by itself, so two such wavefronts fit a SIMD.
//                          VGPR   AGPR   scratch bytes/lane   SGPRs Spill   wavefronts per SIMD   LDS bytes
//     Lander3dof               162     32                    0            76                     2        2392
//     Lander3dof, LOOP         256     59                    0           102                     1        5440
//     Rocket2D                 194     32                    0            83                     2        2392
//     Rocket2D, LOOP           256     69                    0           104                     1        5440
//     RocketQuat               186     32                    0            81                     2        2392
//     RocketQuat, LOOP         256    104                    0           105                     1        5440
#pragma once
#include "lqr_covariance_kernel.h"

namespace scpp
{
namespace lqr
{

constexpr int FILTER_WAVES_PER_SIMD = 1;

template <bool LOOP>
struct FilterLds
{
    double At[RT * RT];                               // At[c][r] = A[r][c], open loop; rows and columns >= nx stay zero
    double Acl[LOOP ? RT * RT : 1];                   // the same of A_cl = A - B K_t (LOOP; one unused entry otherwise, as G0 and G1)
    double G0[LOOP ? 4 * RT : 1], G1[LOOP ? 4 * RT : 1]; // gains of the segment's two nodes, [a][c]
    SegmentLds seg;
};

// one trajectory's share of the filter sweep's arrays; ecb, xcb == nullptr: not kept; ssb, icb, fsb, xcb are the loop's (LOOP)
struct FilterIo
{
    const double *Gb;
    double *Lb, *esb, *feb, *ecb, *ssb, *icb, *fsb, *xcb;
};

// lane r < NX: row r of A and (LOOP) of A_cl = A - B K_t at the reference's point a of the segment -> LDS, transposed; afterwards every lane holds
// its share of both tiles.  The A_cl row is formed as closedLoopJacobian forms it.
template <class P, bool LOOP>
__device__ __forceinline__ void filterJacobian(FilterLds<LOOP> &lds, int lane, double a, const double *p, const double *aux, double (&Ao)[4],
                                               double (&Ac)[4])
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
            lds.At[c * RT + lane] = jr[c];
            if constexpr (LOOP)
            {
                double acl = jr[c];
#pragma unroll
                for (int q = 0; q < NU; q++)
                    acl -= jr[NX + q] * (lds.G0[q * RT + c] + a * (lds.G1[q * RT + c] - lds.G0[q * RT + c]));
                lds.Acl[c * RT + lane] = acl;
            }
        }
    }
    WAVE_SYNC();
#pragma unroll
    for (int c = 0; c < 4; c++)
    {
        Ao[c] = lds.At[(4 * c + g) * RT + col];
        Ac[c] = LOOP ? lds.Acl[LOOP ? (4 * c + g) * RT + col : 0] : 0.;
    }
    WAVE_SYNC();
}

// Y = H Sg in the accumulator layout: register r of lane l is (H Sg)[4r + g][col]
__device__ __forceinline__ d4_t measuredTile(const double (&Ht)[4], const d4_t &Sg)
{
    d4_t Y = {0., 0., 0., 0.};
#pragma unroll
    for (int c = 0; c < 4; c++)
        Y = __builtin_amdgcn_mfma_f64_16x16x4f64(Ht[c], Sg[c], Y, 0, 0, 0);
    return Y;
}

// node k: L_k, error_std, the kept tiles; LOOP: state_std and G[k] Xh G[k]'.  false, and nothing written, if anything is not finite.
template <int NX, int NU, bool LOOP>
__device__ __forceinline__ bool filterNode(int lane, int k, int ny, const d4_t &Sg, const d4_t &Xh, const double (&Ht)[4], const double (&vr)[4],
                                           const FilterIo &io)
{
    const int g = lane >> 4, col = lane & 15;
    const d4_t Y = measuredTile(Ht, Sg);
    d4_t Lr, St = Sg;
    int nf = 0;
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        Lr[r] = Y[r] / vr[r];
        nf |= (isFinite(Lr[r]) && isFinite(Sg[r])) ? 0 : 1;
    }
    [[maybe_unused]] d4_t Sk = {0., 0., 0., 0.};
    if constexpr (LOOP)
    {
        double Gt[4];
        d4_t Wp;
        loadGainTile<NX, NU>(lane, k, io.Gb, Gt);
        Sk = gainCongruence(Xh, Gt, Wp); // register 0 of lane l is (G Xh G')[g][col]
        nf |= isFinite(Sk[0]) ? 0 : 1;
#pragma unroll
        for (int r = 0; r < 4; r++)
        {
            St[r] = Sg[r] + Xh[r];
            nf |= (isFinite(Xh[r]) && isFinite(St[r])) ? 0 : 1;
        }
    }
    if (waveOr(nf))
        return false;
    if (io.ecb)
        storeTile<NX>(lane, io.ecb + k * NX * NX, Sg);
    if constexpr (LOOP)
        if (io.xcb)
            storeTile<NX>(lane, io.xcb + k * NX * NX, Xh);
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        if (4 * r + g < ny && col < NX)
            io.Lb[(k * NX + col) * ny + 4 * r + g] = Lr[r];
        if (4 * r + g == col && col < NX)
        {
            io.esb[k * NX + col] = sqrt(Sg[r] > 0. ? Sg[r] : 0.); // a diagonal entry negative from rounding: 0
            if constexpr (LOOP)
                io.ssb[k * NX + col] = sqrt(St[r] > 0. ? St[r] : 0.);
        }
    }
    if constexpr (LOOP)
        if (g < NU && col < NU)
            io.icb[(k * NU + g) * NU + col] = Sk[0];
    return true;
}

// zeros for nodes kfail..K-1 (kfail == K: none), the final tiles (zeros after a failure) and the trajectory's status
template <int NX, int NU, bool LOOP>
__device__ __forceinline__ void filterEpilogue(int lane, int K, int kfail, int ny, int incomplete, const d4_t &Sg, const d4_t &Xh, const FilterIo &io,
                                               int *status_b)
{
    for (int e = kfail * NX * ny + lane; e < K * NX * ny; e += WAVE)
        io.Lb[e] = 0.;
    for (int e = kfail * NX + lane; e < K * NX; e += WAVE)
    {
        io.esb[e] = 0.;
        if constexpr (LOOP)
            io.ssb[e] = 0.;
    }
    if (io.ecb)
        for (int e = kfail * NX * NX + lane; e < K * NX * NX; e += WAVE)
            io.ecb[e] = 0.;
    const d4_t zero = {0., 0., 0., 0.};
    const bool ok = kfail == K;
    storeTile<NX>(lane, io.feb, ok ? Sg : zero);
    if constexpr (LOOP)
    {
        for (int e = kfail * NU * NU + lane; e < K * NU * NU; e += WAVE)
            io.icb[e] = 0.;
        if (io.xcb)
            for (int e = kfail * NX * NX + lane; e < K * NX * NX; e += WAVE)
                io.xcb[e] = 0.;
        d4_t St;
#pragma unroll
        for (int r = 0; r < 4; r++)
            St[r] = Sg[r] + Xh[r];
        storeTile<NX>(lane, io.fsb, ok ? St : zero);
    }
    if (lane == 0)
        *status_b = !ok ? ST_NONFINITE : (incomplete ? ST_GAINS_INCOMPLETE : ST_OK);
}

// One sweep per trajectory.  X [B][K][nx], U [B][uRows][nu] (nU rows used), T [B], par [B][np], S0 [B][nx][nx] (s0_stride 0: one matrix for every
// trajectory), w [nx], H [ny][nx], v [ny], 1 <= ny <= 16  ->  L [B][K][nx][ny], esd [B][K][nx] = sqrt diag Sg(t_k), fecov [B][nx][nx] = Sg(T),
// status [B], ecov [B][K][nx][nx] = Sg(t_k) (nullptr: not kept).  LOOP: and G [B][K][nu][nx], gstatus [B][K] (nullptr: gains without a status)
// ->  ssd [B][K][nx] = sqrt diag (Sg + Xh)(t_k), icov [B][K][nu][nu] = G[k] Xh(t_k) G[k]', fscov [B][nx][nx] = (Sg + Xh)(T), xcov [B][K][nx][nx] =
// Xh(t_k) (nullptr: not kept); without LOOP none of these is read or written.  Segments, holds and the gain interpolation: covarianceSweep.
template <class P, bool LOOP>
__global__ void __launch_bounds__(WAVE, FILTER_WAVES_PER_SIMD)
    lqr_filter_kernel(int K, int nU, int uRows, int steps, const double *__restrict__ X, const double *__restrict__ U, const double *__restrict__ T,
                      const double *__restrict__ par, int par_stride, const double *__restrict__ G, const int *__restrict__ gstatus,
                      const double *__restrict__ S0, int s0_stride, const double *__restrict__ w, const double *__restrict__ H,
                      const double *__restrict__ v, int ny, double *__restrict__ L, double *__restrict__ esd, double *__restrict__ fecov,
                      int *__restrict__ status, double *__restrict__ ecov, double *__restrict__ ssd, double *__restrict__ icov,
                      double *__restrict__ fscov, double *__restrict__ xcov)
{
    using Model = typename P::Model;
    using JR = typename Model::JacobianRows;
    constexpr int NX = Model::NX, NU = Model::NU, NP = Model::NP, NT = LOOP ? 2 : 1;
    static_assert(NX <= RT && NU <= 4, "Sg and Xh are one 16 x 16 tile each, the gain one 4-row chunk");
    __shared__ FilterLds<LOOP> lds;
    const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
    const long b = blockIdx.x;
    const bool foh = (nU == K);
    const double *Xb = X + b * K * NX, *Ub = U + b * uRows * NU;
    FilterIo io = {nullptr, L + b * K * NX * ny, esd + b * K * NX, fecov + b * NX * NX, ecov ? ecov + b * K * NX * NX : nullptr,
                   nullptr, nullptr, nullptr, nullptr};
    if constexpr (LOOP)
    {
        io.Gb = G + b * K * NU * NX;
        io.ssb = ssd + b * K * NX;
        io.icb = icov + b * K * NU * NU;
        io.fsb = fscov + b * NX * NX;
        io.xcb = xcov ? xcov + b * K * NX * NX : nullptr;
    }

    for (int e = lane; e < RT * RT; e += WAVE)
    {
        lds.At[e] = 0.;
        if constexpr (LOOP)
            lds.Acl[e] = 0.;
    }
    double p[NP], aux[JR::NAUX > 0 ? JR::NAUX : 1];
    loadParameters<P>(par, b, par_stride, p, aux);
    const d4_t wd = diagonalTile<NX>(lane, w);
    // the measurement, once per kernel: the lane's share of the H tile, v of its four rows (1 below row ny, where Y is zero) and sqrt(1 / v)
    double Ht[4], vr[4], vs[4];
#pragma unroll
    for (int c = 0; c < 4; c++)
    {
        const bool in = col < ny && 4 * c + g < NX;
        Ht[c] = in ? H[(in ? col : 0) * NX + (in ? 4 * c + g : 0)] : 0.;
        const bool row = 4 * c + g < ny;
        vr[c] = row ? v[row ? 4 * c + g : 0] : 1.;
        vs[c] = row ? sqrt(1. / vr[c]) : 0.;
    }
    int bad = 0, incomplete = 0;
    d4_t Tc[NT];
    Tc[0] = loadInitialTile<NX, false>(lane, S0 + b * s0_stride, nullptr, bad);
    const d4_t zero = {0., 0., 0., 0.};
    if constexpr (LOOP)
        Tc[1] = zero;
    const double t_max = T[b];
    if constexpr (LOOP)
    {
        const ForwardIo fio = {io.Gb, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        scanForwardInputs<NX, NU, false>(lane, t_max, Xb, Ub, K, nU, fio, gstatus ? gstatus + b * K : nullptr, bad, incomplete);
    }
    else
        bad = waveOr(bad | referenceNonFinite<NX, NU>(lane, t_max, Xb, Ub, K, nU));
    WAVE_SYNC();

    const double dt = t_max / double(K - 1);
    const double h = dt / double(steps);
    int kfail = bad ? 0 : K; // nodes kfail..K-1 carry zeros
    for (int k = 0; k < K && kfail == K; k++)
    {
        if (k > 0)
        {
            // ---- segment i = k-1: both tiles from t_i to t_k, `steps` RKF78 steps ----
            const int i = k - 1, ju = foh ? k : i;
            loadSegment<NX, NU>(lds.seg, lane, Xb, Ub, i, ju);
            if constexpr (LOOP)
                if (g < NU && col < NX)
                {
                    lds.G0[g * RT + col] = io.Gb[(i * NU + g) * NX + col];
                    lds.G1[g * RT + col] = io.Gb[(ju * NU + g) * NX + col];
                }
            WAVE_SYNC();
            for (int n = 0; n < steps; n++)
                rkf78TilesStep<NT>(Tc, h, [&](int s, const d4_t (&Ts)[NT], d4_t (&F)[NT]) __attribute__((always_inline)) {
                    const double a = (double(n) + RK_C[s]) / double(steps);
                    double Ao[4], Ac[4];
                    filterJacobian<P, LOOP>(lds, lane, a, p, aux, Ao, Ac); // synchronises after its writes and after its reads
                    const d4_t Y = measuredTile(Ht, Ts[0]);
                    double Ys[4];
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        Ys[r] = Y[r] * vs[r];
                    d4_t S = {0., 0., 0., 0.};
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        S = __builtin_amdgcn_mfma_f64_16x16x4f64(Ys[c], Ys[c], S, 0, 0, 0);
                    const d4_t Fo = covarianceRhs(Ts[0], Ao, wd);
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        F[0][r] = Fo[r] - S[r];
                    if constexpr (LOOP)
                    {
                        const d4_t Fh = covarianceRhs(Ts[1], Ac, zero);
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            F[1][r] = Fh[r] + S[r];
                    }
                });
        }
        if (!filterNode<NX, NU, LOOP>(lane, k, ny, Tc[0], Tc[LOOP ? 1 : 0], Ht, vr, io))
        {
            kfail = k;
            break;
        }
    }
    filterEpilogue<NX, NU, LOOP>(lane, K, kfail, ny, incomplete, Tc[0], Tc[LOOP ? 1 : 0], io, status + b);
}

} // namespace lqr
} // namespace scpp

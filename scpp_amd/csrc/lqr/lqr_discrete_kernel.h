// Sampled-data LQR: the discrete Riccati recursion swept backwards along every trajectory (include/scpp_hip_lqr.h,
// scpp_hip_lqr_compute_gains_discrete).  A correction du_i held over segment i moves the deviation by
//
//   dx_{i+1} = Phi_i dx_i + Gamma_i du_i,    d[Phi | Gamma]/dt = A(t) [Phi | Gamma] + [0 | B(t)],   [Phi | Gamma](t_i) = [I | 0]
//   S_i = R dt + Gamma_i'P_{i+1} Gamma_i,    N_i = Gamma_i'P_{i+1} Phi_i,    L_i L_i' = S_i,    Y_i = L_i^-1 N_i
//   K_i = L_i^-T Y_i,                        P_i = Q dt + Phi_i'P_{i+1} Phi_i - Y_i'Y_i,        P_{K-1} = Qf
//
// Mapping: ONE WAVEFRONT PER TRAJECTORY, every matrix one 16 x 16 FP64 tile in the accumulator layout (lqr_tile_sweep.h).  A tile in that layout,
// handed to the matrix core as the A operand, is read as its own transpose; as the B operand it is read as it is.  So with X and Y in the layout
// mfma(X, Y) = X'Y, and no product below needs a lane exchange:
//     right-hand side   A T + C        4   (A operand: the Jacobian tile kept TRANSPOSED in LDS, as the covariance sweep keeps A_cl; C = [0 | B] in the accumulator)
//     W = P Phi         4   (A operand: P, symmetric)          V = P Gamma       4
//     F = Phi'W         4                                      N = Gamma'W       4        S = Gamma'V   4
//     Y'Y               1   (both operands the same register, so the product is symmetric to the bit)
// [Phi | Gamma] is ONE tile where nx + nu <= 16 (Rocket2D 6 + 2, Lander3dof 7 + 3): Gamma sits in columns nx.. and is moved to columns 0.. through
// LDS once per segment.  RocketQuat (14 + 4): thirteen stage slopes of two tiles do not fit beside the Jacobian rows, so Phi is the tile and Gamma
// (56 entries) is ONE ENTRY PER LANE, integrated in the same pass on the same Jacobian evaluation; its A Gamma entry is nx multiply-adds on LDS.
// F = Phi'(P Phi) is symmetric only to rounding; it is SYMMETRISED ONCE PER NODE through LDS, F <- (F + F') / 2, the sum of the same two numbers on
// both sides of the diagonal.  Q dt and Y'Y are symmetric to the bit, so P is, at every node.
// The nu x nu Cholesky factor and the two triangular solves are scalar work every lane does for its own column.
#pragma once
#include "lqr_sweep_frame.h"

namespace scpp
{
namespace lqr
{

constexpr int DISCRETE_WAVES_PER_SIMD = 2; // the register budget the compiler is held to: 256 per lane (see the kernel)

struct DiscreteLds
{
    double At[RT * RT]; // At[c][r] = A[r][c]; rows and columns >= nx stay zero
    double Bm[RT * 4];  // rows >= nx, columns >= nu stay zero
    double M[RT * RT];  // exchange tile: the split of [Phi | Gamma], then F for its transpose
    double S[4 * 4];    // Gamma'P Gamma
    double N[4 * RT];   // Gamma'P Phi; columns >= nx stay zero
    double Gs[RT * 4];  // Gamma of the stage, one entry per lane (RocketQuat): Gs[row][a]
    SegmentLds seg;
};

// lane r < NX: row r of [A | B] at fraction a of the segment -> LDS (A transposed); afterwards Ac is the lane's share of the A operand that reads
// as A, and Ct its share of the tile [0 | B], B in columns NX .. NX + NU - 1
template <class P>
__device__ __forceinline__ void transitionJacobian(DiscreteLds &lds, int lane, double a, const double *p, const double *aux, double (&Ac)[4], d4_t &Ct)
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
            lds.At[c * RT + lane] = jr[c];
#pragma unroll
        for (int q = 0; q < NU; q++)
            lds.Bm[lane * 4 + q] = jr[NX + q];
    }
    WAVE_SYNC();
    const bool inB = col >= NX && col < NX + NU;
#pragma unroll
    for (int c = 0; c < 4; c++)
    {
        Ac[c] = lds.At[(4 * c + g) * RT + col];
        Ct[c] = inB ? lds.Bm[(4 * c + g) * 4 + (inB ? col - NX : 0)] : 0.;
    }
    WAVE_SYNC();
}

// `steps` RKF78 steps of dT/dt = A T + [0 | B], T = [Phi | Gamma] one tile, forwards over the segment in lds.seg; stage s of step n at a = (n + c_s) / steps
template <class P>
__device__ __forceinline__ void integrateTransition(DiscreteLds &lds, int lane, int steps, double h, const double *p, const double *aux, d4_t &Tt)
{
    for (int n = 0; n < steps; n++)
        rkf78TileStep(Tt, h, [&](int s, const d4_t Ts) __attribute__((always_inline)) {
            const double a = (double(n) + RK_C[s]) / double(steps);
            double Ac[4];
            d4_t F;
            transitionJacobian<P>(lds, lane, a, p, aux, Ac, F);
#pragma unroll
            for (int c = 0; c < 4; c++)
                F = __builtin_amdgcn_mfma_f64_16x16x4f64(Ac[c], Ts[c], F, 0, 0, 0);
            return F;
        });
}

// One fixed RKF78 step of a tile AND one double per lane (rkf78TileStep of lqr_tile_sweep.h with a fifth component): the thirteen slopes of both
// stay in registers, 65 doubles per lane.  rhs(s, Ts, vs, kT, kv) fills the two slopes.
template <class Rhs>
__device__ __forceinline__ void rkf78TileLaneStep(d4_t &T, double &v, double h, Rhs &&rhs)
{
    d4_t kk[RK_S];
    double kv[RK_S];
#pragma unroll
    for (int s = 0; s < RK_S; s++)
    {
        d4_t Ts;
#pragma unroll
        for (int r = 0; r < 4; r++)
        {
            double acc = 0.;
#pragma unroll
            for (int qq = 0; qq < s; qq++)
                if (RK_A[s][qq] != 0.)
                    acc += RK_A[s][qq] * kk[qq][r];
            Ts[r] = T[r] + h * acc;
        }
        double acc = 0.;
#pragma unroll
        for (int qq = 0; qq < s; qq++)
            if (RK_A[s][qq] != 0.)
                acc += RK_A[s][qq] * kv[qq];
        const double vs = v + h * acc;
        rhs(s, Ts, vs, kk[s], kv[s]);
    }
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
    double acc = 0.;
#pragma unroll
    for (int s = 0; s < RK_S; s++)
        if (RK_B[s] != 0.)
            acc += RK_B[s] * kv[s];
    v += h * acc;
}

// `steps` RKF78 steps of dPhi/dt = A Phi (a tile) and dGamma/dt = A Gamma + B with Gamma ONE ENTRY PER LANE (lane l: Gamma[l >> 2][l & 3]; for
// nx + nu > 16): one Jacobian evaluation serves both.  The lane's A Gamma entry is nx multiply-adds on the LDS copies of A and of the stage's Gamma.
template <class P>
__device__ __forceinline__ void integrateTransitionLane(DiscreteLds &lds, int lane, int steps, double h, const double *p, const double *aux, d4_t &Ph,
                                                        double &gam)
{
    constexpr int NX = P::Model::NX, NU = P::Model::NU;
    static_assert(RT * 4 <= WAVE, "one lane per entry of the 16 x 4 input tile");
    const int g = lane >> 4, col = lane & 15, row = lane >> 2, in = lane & 3;
    for (int n = 0; n < steps; n++)
        rkf78TileLaneStep(Ph, gam, h, [&](int s, const d4_t Ts, double vs, d4_t &kT, double &kv) __attribute__((always_inline)) {
            const double a = (double(n) + RK_C[s]) / double(steps);
            lds.Gs[lane] = vs;
            if (lane < NX)
            {
                double x[NX], u[NU], jr[NX + NU];
                interpolateSegment(lds.seg, a, x, u);
                jacobianRow<P>(lane, x, u, p, aux, jr);
#pragma unroll
                for (int c = 0; c < NX; c++)
                    lds.At[c * RT + lane] = jr[c];
#pragma unroll
                for (int q = 0; q < NU; q++)
                    lds.Bm[lane * 4 + q] = jr[NX + q];
            }
            WAVE_SYNC();
            d4_t F = {0., 0., 0., 0.};
#pragma unroll
            for (int c = 0; c < 4; c++)
                F = __builtin_amdgcn_mfma_f64_16x16x4f64(lds.At[(4 * c + g) * RT + col], Ts[c], F, 0, 0, 0);
            double acc = lds.Bm[row * 4 + in]; // rows >= nx of A and B are zero: those lanes stay at 0
#pragma unroll
            for (int j = 0; j < NX; j++)
                acc += lds.At[j * RT + row] * lds.Gs[j * 4 + in];
            WAVE_SYNC();
            kT = F;
            kv = acc;
        });
}

// X'Y of two tiles in the accumulator layout
__device__ __forceinline__ d4_t tileTransposeProduct(const d4_t X, const d4_t Y)
{
    d4_t D = {0., 0., 0., 0.};
#pragma unroll
    for (int c = 0; c < 4; c++)
        D = __builtin_amdgcn_mfma_f64_16x16x4f64(X[c], Y[c], D, 0, 0, 0);
    return D;
}

__device__ __forceinline__ int tileNonFinite(const d4_t M)
{
    int nf = 0;
#pragma unroll
    for (int r = 0; r < 4; r++)
        nf |= isFinite(M[r]) ? 0 : 1;
    return nf;
}

// the NX x NU corner of a tile -> dst [NX][NU]
template <int NX, int NU>
__device__ __forceinline__ void storeInputTile(int lane, double *dst, const d4_t M)
{
    const int g = lane >> 4, col = lane & 15;
#pragma unroll
    for (int r = 0; r < 4; r++)
        if (4 * r + g < NX && col < NU)
            dst[(4 * r + g) * NU + col] = M[r];
}

// One sweep per trajectory.  X [B][K][nx], U [B][uRows][nu] (nU rows used: K first-order hold, K-1 zero-order hold), T [B], par [B][np], q / qf [nx],
// r [nu]  ->  G [B][K][nu][nx], status [B][K], iters [B][K] = RKF78 steps behind the node; Pout [B][K][nx][nx], PhiOut [B][K-1][nx][nx],
// GamOut [B][K-1][nx][nu] (all three nullptr: not kept).  Segment i is integrated from a = 0 up to a = 1 with x = X[i] + a (X[i+1] - X[i]),
// u = U[i] + a (U[j] - U[i]), j = i+1 (first-order) or i (zero-order); the segment index is the loop's, never derived from a time.  Node K-1 has no
// segment behind it: its gain is a copy of node K-2's (and shares its fate), its P is Qf.
// Two wavefronts per SIMD are asked for: left alone the compiler parks 38 values in accumulator registers on top of 171 .. 224 vector registers and
// RocketQuat ends at one wavefront; held to 256 registers in all it needs 228 and no accumulator register, with no scratch and no spill.
template <class P>
__global__ void __launch_bounds__(WAVE, DISCRETE_WAVES_PER_SIMD) lqr_discrete_kernel(int K, int nU, int uRows, int steps, const double *__restrict__ X, const double *__restrict__ U,
                                                             const double *__restrict__ T, const double *__restrict__ par, int par_stride,
                                                             const double *__restrict__ qw, const double *__restrict__ rw, const double *__restrict__ qfw,
                                                             double *__restrict__ G, int *__restrict__ status, int *__restrict__ iters,
                                                             double *__restrict__ Pout, double *__restrict__ PhiOut, double *__restrict__ GamOut)
{
    using Model = typename P::Model;
    using JR = typename Model::JacobianRows;
    constexpr int NX = Model::NX, NU = Model::NU, NP = Model::NP;
    constexpr bool ONE_TILE = NX + NU <= RT;
    static_assert(NX <= RT && NU <= 4, "Phi is one 16 x 16 tile, Gamma'P one 4-row chunk");
    __shared__ DiscreteLds lds;
    const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
    const long b = blockIdx.x;
    const bool foh = (nU == K);
    const double *Xb = X + b * K * NX, *Ub = U + b * uRows * NU;
    double *Gb = G + b * K * NU * NX;
    double *Pb = Pout ? Pout + b * K * NX * NX : nullptr;
    double *Fb = PhiOut ? PhiOut + b * (K - 1) * NX * NX : nullptr;
    double *Cb = GamOut ? GamOut + b * (K - 1) * NX * NU : nullptr;

    for (int e = lane; e < RT * RT; e += WAVE)
        lds.At[e] = 0.;
    lds.Bm[lane] = 0.;
    lds.N[lane] = 0.;
    double p[NP], aux[JR::NAUX > 0 ? JR::NAUX : 1];
    loadParameters<P>(par, b, par_stride, p, aux);
    const double t_max = T[b];
    const double dt = t_max / double(K - 1);
    const double h = t_max / double(K - 1) / double(steps);
    double rdt[NU];
#pragma unroll
    for (int q = 0; q < NU; q++)
        rdt[q] = rw[q] * dt;
    d4_t qd = diagonalTile<NX>(lane, qw);
#pragma unroll
    for (int r = 0; r < 4; r++)
        qd[r] *= dt;
    d4_t Pc = diagonalTile<NX>(lane, qfw);
    const int bad = waveOr(referenceNonFinite<NX, NU>(lane, t_max, Xb, Ub, K, nU));
    WAVE_SYNC();

    int kfail = bad ? K - 1 : -1; // nodes 0..kfail carry ST_NONFINITE and zeros
    for (int k = K - 2; k >= 0 && kfail < 0; k--)
    {
        const int failed = (k == K - 2) ? K - 1 : k; // what a failure in this segment takes with it
        // ---- segment k: [Phi | Gamma] from t_k to t_{k+1}, `steps` RKF78 steps ----
        loadSegment<NX, NU>(lds.seg, lane, Xb, Ub, k, foh ? k + 1 : k);
        WAVE_SYNC();
        d4_t Ph, Gm;
#pragma unroll
        for (int r = 0; r < 4; r++)
            Ph[r] = (4 * r + g == col && col < NX) ? 1. : 0.;
        if constexpr (ONE_TILE)
        {
            integrateTransition<P>(lds, lane, steps, h, p, aux, Ph);
#pragma unroll
            for (int r = 0; r < 4; r++)
                lds.M[(4 * r + g) * RT + col] = Ph[r];
            WAVE_SYNC();
#pragma unroll
            for (int r = 0; r < 4; r++)
            {
                Gm[r] = col < NU ? lds.M[(4 * r + g) * RT + NX + (col < NU ? col : 0)] : 0.;
                Ph[r] = col < NX ? Ph[r] : 0.;
            }
            WAVE_SYNC();
        }
        else
        {
            double gam = 0.;
            integrateTransitionLane<P>(lds, lane, steps, h, p, aux, Ph, gam);
            lds.Gs[lane] = gam;
            WAVE_SYNC();
#pragma unroll
            for (int r = 0; r < 4; r++)
                Gm[r] = col < NU ? lds.Gs[(4 * r + g) * 4 + (col < NU ? col : 0)] : 0.;
            WAVE_SYNC();
        }
        if (waveOr(tileNonFinite(Ph) | tileNonFinite(Gm)))
        {
            kfail = failed;
            break;
        }
        // ---- one step of the recursion: P_{k+1} -> K_k, P_k ----
        const d4_t W = tileTransposeProduct(Pc, Ph), V = tileTransposeProduct(Pc, Gm);
        const d4_t F = tileTransposeProduct(Ph, W), Nn = tileTransposeProduct(Gm, W), Sg = tileTransposeProduct(Gm, V);
        if (g < NU && col < NX)
            lds.N[g * RT + col] = Nn[0];
        if (g < NU && col < NU)
            lds.S[g * 4 + col] = Sg[0];
#pragma unroll
        for (int r = 0; r < 4; r++)
            lds.M[(4 * r + g) * RT + col] = F[r];
        WAVE_SYNC();
        // L L' = R dt + S from the lower triangle; a pivot that is not positive and finite fails the segment
        double L[NU][NU], Y[NU], Kc[NU];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < NU; j++)
        {
            double d = rdt[j] + lds.S[j * 4 + j];
#pragma unroll
            for (int m = 0; m < j; m++)
                d -= L[j][m] * L[j][m];
            ok = ok && d > 0. && isFinite(d);
            L[j][j] = sqrt(d);
#pragma unroll
            for (int i = j + 1; i < NU; i++)
            {
                double s = lds.S[i * 4 + j];
#pragma unroll
                for (int m = 0; m < j; m++)
                    s -= L[i][m] * L[j][m];
                L[i][j] = s / L[j][j];
            }
        }
        // column `col` of Y = L^-1 N and of K = L^-T Y
#pragma unroll
        for (int i = 0; i < NU; i++)
        {
            double s = lds.N[i * RT + col];
#pragma unroll
            for (int m = 0; m < i; m++)
                s -= L[i][m] * Y[m];
            Y[i] = s / L[i][i];
        }
#pragma unroll
        for (int i = NU - 1; i >= 0; i--)
        {
            double s = Y[i];
#pragma unroll
            for (int m = i + 1; m < NU; m++)
                s -= L[m][i] * Kc[m];
            Kc[i] = s / L[i][i];
        }
        double y = 0., gain = 0.;
#pragma unroll
        for (int i = 0; i < NU; i++)
            if (g == i)
            {
                y = Y[i];
                gain = Kc[i];
            }
        d4_t YY = {0., 0., 0., 0.};
        YY = __builtin_amdgcn_mfma_f64_16x16x4f64(y, y, YY, 0, 0, 0);
        d4_t Pn;
#pragma unroll
        for (int r = 0; r < 4; r++)
        {
            const double fs = 0.5 * (F[r] + lds.M[col * RT + 4 * r + g]);
            Pn[r] = (qd[r] + fs) - YY[r];
        }
        WAVE_SYNC();
        if (waveOr((ok ? 0 : 1) | (isFinite(gain) ? 0 : 1) | tileNonFinite(Pn)))
        {
            kfail = failed;
            break;
        }
        if (k == K - 2)
        {
            if (g < NU && col < NX)
                Gb[((K - 1) * NU + g) * NX + col] = gain;
            if (Pb)
                storeTile<NX>(lane, Pb + (K - 1) * NX * NX, Pc);
            markNodeOk(lane, status + b * K, iters + b * K, K - 1, 0);
        }
        Pc = Pn;
        if (g < NU && col < NX)
            Gb[(k * NU + g) * NX + col] = gain;
        if (Pb)
        {
            storeTile<NX>(lane, Pb + k * NX * NX, Pc);
            storeTile<NX>(lane, Fb + k * NX * NX, Ph);
            storeInputTile<NX, NU>(lane, Cb + k * NX * NU, Gm);
        }
        markNodeOk(lane, status + b * K, iters + b * K, k, (K - 1 - k) * steps);
    }
    // a failed node never writes a non-finite value: zeros and its status, for the node of the segment that failed and every earlier one
    backwardEpilogue<NX, NU>(lane, kfail, Gb, Pb, status + b * K, iters + b * K);
    if (Pb)
    {
        const int segs = kfail + 1 < K - 1 ? kfail + 1 : K - 1;
        for (int e = lane; e < segs * NX * NX; e += WAVE)
            Fb[e] = 0.;
        for (int e = lane; e < segs * NX * NU; e += WAVE)
            Cb[e] = 0.;
    }
}

} // namespace lqr
} // namespace scpp

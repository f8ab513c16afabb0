// Batched LQR trajectory tracking: the two kernels behind include/scpp_hip_lqr.h.
//   lqr_gain_kernel<Plugin>   one frozen-time LQR gain per (trajectory, node): replaces LQRTracker::LQRTracker (LQRTracker.cpp:6-28) and
//                             ComputeLQR / careSolve / solveSchurIterative (LQR.cpp:7-109)
//   lqr_track_kernel<Plugin, SAT, HOLD, FF, NOISE>  one closed loop per flight on the nonlinear plant: replaces the loop of SC_tracking.cpp:48-75 with
//                             LQRTracker::getInput / interpolateGains (LQRTracker.cpp:43-65) and trajectoryData.hpp:41-78; SAT: with the
//                             plugin's input limits in the loop (the clip of LQR_sim.cpp:55-66)
//                             FF: with the feedforward term of the affine finite-horizon law (lqr_affine_kernel.h)
//                             NOISE: with process noise on the plant (lqr_noise.h)
// A component of its own: it reads the model plugins' flow maps, their generated Jacobian rows and the RKF78 tableau (csrc/common.h) and nothing
// else of the solver; the solver's sources are not touched by it.
#pragma once
#include "../common.h"
#include "../model_rocketquat.h"
#include "../model_lander3dof.h"
#include "lqr_noise.h"

namespace scpp
{
namespace lqr
{

constexpr int HALF = 32;                 // lanes per Hamiltonian: lane = row, two problems per wavefront
constexpr int SIGN_MAX_ITERATIONS = 100; // LQR.cpp:78; the reference tests `iterations > maxIterations`, i.e. at most 101 inversions
constexpr double SIGN_EPS = 1e-8;        // LQR.cpp:78
constexpr int ST_OK = 0, ST_STEP_CAP = 1, ST_ITERATION_LIMIT = -1, ST_NONFINITE = -2;

// ---- input limits of the tracking loop (scpp_hip_lqr_set_input_limits).  One row on the device is LIM_ROW doubles: (T_min, T_max, angle_max,
// tan(angle_max)); the host computes the tangent once, so the device, the emulation and a host twin clip with the same number.  Every product
// below is a statement of its own: under -ffp-contract=on nothing here is fused, and the rule rounds the same wherever it is compiled. ----
constexpr int LIM_ROW = 4;
// LQR_sim.cpp:55-66 in its order, on the thrust vector u[0..2]:  u_z = max(T_min, u_z);  c = tan(angle_max) u_z, |u_xy| > c: u_xy *= c / |u_xy|;
// |u| > T_max: u *= T_max / |u|.  With T_min <= T_max cos(angle_max) (the host checks it) the result satisfies all three constraints.
__host__ __device__ inline void saturateThrustVector(double *u, const double *lim)
{
    if (u[2] < lim[0])
        u[2] = lim[0];
    const double c = lim[3] * u[2];
    const double xx = u[0] * u[0], yy = u[1] * u[1];
    const double nxy = sqrt(xx + yy);
    if (nxy > c)
    {
        const double s = c / nxy;
        u[0] *= s;
        u[1] *= s;
    }
    const double x2 = u[0] * u[0], y2 = u[1] * u[1], z2 = u[2] * u[2];
    const double n = sqrt((x2 + y2) + z2);
    if (n > lim[1])
    {
        const double s = lim[1] / n;
        u[0] *= s;
        u[1] *= s;
        u[2] *= s;
    }
}

// ---- LQR traits of the model plugins.  LQR_TANGENT: the Riccati equation is solved on the tangent system x = N(x) xi (NR < NX columns, orthonormal),
// A_r = N'AN, B_r = N'B, Q_r = N'QN, K = K_r N'; the plugin supplies the rows of N. ----
struct RocketQuatLqr
{
    using Model = RocketQuatModel;
    static constexpr int ID = Model::MODEL_ID;
    // The quaternion direction dq || q is neither driven nor damped: with w_B = 0, p = (0,..,q,..,0) has p'A = 0 and p'B = 0 and the 28 x 28
    // Hamiltonian is exactly singular.  Tangent coordinates: m, r, v, w as they are, and the three columns of the
    // left-multiplication matrix of q other than q itself (orthogonal to q and to each other), normalised, on the quaternion rows.
    static constexpr bool LQR_TANGENT = true;
    static constexpr int NR = 13;
    __host__ __device__ static inline void tangentRow(int row, const double *x, double *n)
    {
        for (int c = 0; c < NR; c++)
            n[c] = 0.;
        if (row < 7)
            n[row] = 1.;
        else if (row > 10)
            n[row - 1] = 1.;
        else
        {
            const double qw = x[7], qx = x[8], qy = x[9], qz = x[10];
            const double s = 1. / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
            // L(q) = [[qw,-qx,-qy,-qz],[qx,qw,-qz,qy],[qy,qz,qw,-qx],[qz,-qy,qx,qw]], columns 1..3
            const double L[4][3] = {{-qx, -qy, -qz}, {qw, -qz, qy}, {qz, qw, -qx}, {-qy, qx, qw}};
            for (int c = 0; c < 3; c++)
                n[7 + c] = L[row - 7][c] * s;
        }
    }
    // u = (T_B, tau_z): the thrust vector is clipped, the roll torque passes through
    static constexpr bool THRUST_VECTOR = true;
    __host__ __device__ static inline void saturate(double *u, const double *lim) { saturateThrustVector(u, lim); }
};
struct Rocket2dLqr
{
    using Model = Rocket2dModel;
    static constexpr int ID = Model::MODEL_ID;
    static constexpr bool LQR_TANGENT = false;
    static constexpr int NR = Model::NX;
    // u = (gimbal, thrust): a box (rocket2d.cpp:77-83)
    static constexpr bool THRUST_VECTOR = false;
    __host__ __device__ static inline void saturate(double *u, const double *lim)
    {
        u[0] = u[0] < -lim[2] ? -lim[2] : (u[0] > lim[2] ? lim[2] : u[0]);
        u[1] = u[1] < lim[0] ? lim[0] : (u[1] > lim[1] ? lim[1] : u[1]);
    }
};
struct Lander3dofLqr
{
    using Model = Lander3dofModel;
    static constexpr int ID = Model::MODEL_ID;
    static constexpr bool LQR_TANGENT = false;
    static constexpr int NR = Model::NX;
    // u = T_I, the thrust vector in the inertial frame; angle_max is the pointing cone about (0, 0, 1)
    static constexpr bool THRUST_VECTOR = true;
    __host__ __device__ static inline void saturate(double *u, const double *lim) { saturateThrustVector(u, lim); }
};
template <class... P>
struct LqrPluginList
{
};
using LqrPlugins = LqrPluginList<RocketQuatLqr, Rocket2dLqr, Lander3dofLqr>;
// f(Plugin{}) for the plugin whose ID is `model`; false for an id nobody registered
template <class F, class... PL>
inline bool withLqrPluginOf(LqrPluginList<PL...>, int model, F &&f)
{
    return ((model == PL::ID ? (f(PL{}), true) : false) || ...);
}
template <class F>
inline bool withLqrPlugin(int model, F &&f)
{
    return withLqrPluginOf(LqrPlugins{}, model, f);
}

__device__ __forceinline__ bool isFinite(double v) { return fabs(v) <= 1.7976931348623157e308; } // false for a NaN

// ---- reductions over the 32 lanes of one problem: symmetric xor butterflies, so every lane of the half holds the bitwise identical result ----
__device__ __forceinline__ double halfSum(double v)
{
    for (int m = HALF / 2; m >= 1; m >>= 1)
        v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int halfOr(int v)
{
    for (int m = HALF / 2; m >= 1; m >>= 1)
        v |= __shfl_xor(v, m);
    return v;
}

// Gauss-Jordan elimination with partial pivoting, lane = row, the row in registers (every register index a compile-time constant).
// Rows are never moved: the pivot of column j is the largest |W[j]| among the rows not used yet (cross-lane arg-max, ties to the lower lane), its
// row reaches the other lanes of the half by a lane permute, and the lane remembers the step it was the pivot of (myStep); piv[j] is the pivot
// lane of step j (the same in every lane of the half).
//   INPLACE (NPIV == N):  W <- the inverse, stored as  lane piv[j], register c  =  inverse[j][piv[c]]   (the caller undoes the permutation)
//   else: columns NPIV.. are right-hand sides;  afterwards lane piv[j] holds  [e_j | x_j]
// Returns false (in every lane of the half) on a zero or non-finite pivot.
template <int N, int NPIV, bool INPLACE>
__device__ __forceinline__ bool gaussJordan(double (&W)[N], int nrows, int r, int base, int (&piv)[NPIV], int &myStep)
{
    myStep = -1;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NPIV; j++)
    {
        double bv = (myStep < 0 && r < nrows) ? fabs(W[j]) : -1.;
        if (!(bv >= 0.))
            bv = -1.; // a NaN never wins; the result is caught by the caller's finiteness test
        int bi = r;
        for (int m = HALF / 2; m >= 1; m >>= 1)
        {
            const double ov = __shfl_xor(bv, m);
            const int oi = __shfl_xor(bi, m);
            if (ov > bv || (ov == bv && oi < bi))
            {
                bv = ov;
                bi = oi;
            }
        }
        piv[j] = bi;
        if (!(bv > 0.) || !isFinite(bv))
            ok = false;
        double prow[N];
#pragma unroll
        for (int c = 0; c < N; c++)
            prow[c] = __shfl(W[c], base + bi);
        const double ipiv = ok ? 1. / prow[j] : 0.;
        const bool mine = (r == bi);
        if (mine)
            myStep = j;
        const double f = W[j];
#pragma unroll
        for (int c = 0; c < N; c++)
        {
            const double pc = prow[c] * ipiv;
            if (c == j)
                W[c] = INPLACE ? (mine ? ipiv : -f * ipiv) : (mine ? 1. : 0.);
            else
                W[c] = mine ? pc : W[c] - f * pc;
        }
    }
    return ok;
}

// LDS of one problem.  S is scratch: first the set-up products, then the transpose buffer that undoes the pivot permutation of every inverse.
template <class P>
struct GainLds
{
    static constexpr int NX = P::Model::NX, NU = P::Model::NU, NR = P::NR, N2 = 2 * NR;
    static constexpr int OFF_A = 0, OFF_T = OFF_A + NX * NX, OFF_AR = OFF_T + NX * NR, OFF_QR = OFF_AR + NR * NR, SETUP = OFF_QR + NR * NR;
    static constexpr int NS = SETUP > N2 * N2 ? SETUP : N2 * N2;
    double S[NS];
    double Bf[NX * NU]; // B, full state
    double Br[NR * NU]; // N'B
    double Nm[NX * NR]; // tangent basis (LQR_TANGENT only)
    double Kr[NU * NR];
};

// One gain per (instance, node).  X [B][K][nx], U [B][uRows][nu] of which the first nU rows are inputs (nU = K first-order hold, K-1 zero-order hold;
// uRows >= nU is the row stride of the buffer: a solver context keeps K rows whatever the hold), par [B][np], q [nx], r [nu] ->
// G [B][K][nu][nx], status [B][K], iters [B][K].
template <class P>
__global__ void __launch_bounds__(WAVE) lqr_gain_kernel(long nodes, int K, int nU, int uRows, const double *__restrict__ X, const double *__restrict__ U,
                                                         const double *__restrict__ par, int par_stride, const double *__restrict__ qw,
                                                         const double *__restrict__ rw, double *__restrict__ G, int *__restrict__ status,
                                                         int *__restrict__ iters)
{
    using Model = typename P::Model;
    using JR = typename Model::JacobianRows;
    using L = GainLds<P>;
    constexpr int NX = Model::NX, NU = Model::NU, NP = Model::NP, NR = P::NR, N2 = 2 * NR;
    static_assert(N2 <= HALF, "one lane per Hamiltonian row");
    __shared__ L lds2[2];
    const int lane = threadIdx.x & 63, half = lane >> 5, r = lane & (HALF - 1), base = half * HALF;
    const long node0 = long(blockIdx.x) * 2 + half;
    const bool valid = node0 < nodes;
    const long node = valid ? node0 : nodes - 1; // an idle half repeats the last node and writes nothing
    const long b = node / K;
    const int k = int(node % K);
    L &lds = lds2[half];

    // ---- 1. A, B = computeJacobians(X[k], U[k])   (LQRTracker.cpp:12-24; zero-order hold: U[min(k, K-2)]) ----
    double x[NX], u[NU], p[NP], q[NX], rinv[NU];
    const int ku = k < nU ? k : nU - 1;
    for (int j = 0; j < NX; j++)
    {
        x[j] = X[(b * K + k) * NX + j];
        q[j] = qw[j];
    }
    for (int j = 0; j < NU; j++)
    {
        u[j] = U[(b * uRows + ku) * NU + j];
        rinv[j] = 1. / rw[j]; // R diagonal: R_inverse.diagonal() = R.diagonal().cwiseInverse()  (LQR.cpp:71-72)
    }
    for (int j = 0; j < NP; j++)
        p[j] = par[b * par_stride + j];
    if (r < NX)
    {
        double aux[JR::NAUX > 0 ? JR::NAUX : 1], uaux[JR::NUAUX > 0 ? JR::NUAUX : 1], jr[NX + NU];
        JR::prepare(p, aux);
        JR::prepareInput(u, p, uaux);
        (void)JR::row(r, x, u, p, aux, uaux, jr);
#pragma unroll
        for (int c = 0; c < NX; c++)
            lds.S[L::OFF_A + r * NX + c] = jr[c];
#pragma unroll
        for (int a = 0; a < NU; a++)
            lds.Bf[r * NU + a] = jr[NX + a];
        if constexpr (P::LQR_TANGENT)
        {
            double n[NR];
            P::tangentRow(r, x, n);
#pragma unroll
            for (int c = 0; c < NR; c++)
                lds.Nm[r * NR + c] = n[c];
        }
    }
    WAVE_SYNC();
    if constexpr (P::LQR_TANGENT)
    {
        if (r < NX) // T = A N
            for (int c = 0; c < NR; c++)
            {
                double acc = 0.;
                for (int j = 0; j < NX; j++)
                    acc += lds.S[L::OFF_A + r * NX + j] * lds.Nm[j * NR + c];
                lds.S[L::OFF_T + r * NR + c] = acc;
            }
        WAVE_SYNC();
        if (r < NR) // A_r = N'T, B_r = N'B, Q_r = N'QN
        {
            for (int c = 0; c < NR; c++)
            {
                double acc = 0., qa = 0.;
                for (int j = 0; j < NX; j++)
                {
                    acc += lds.Nm[j * NR + r] * lds.S[L::OFF_T + j * NR + c];
                    qa += lds.Nm[j * NR + r] * q[j] * lds.Nm[j * NR + c];
                }
                lds.S[L::OFF_AR + r * NR + c] = acc;
                lds.S[L::OFF_QR + r * NR + c] = qa;
            }
            for (int a = 0; a < NU; a++)
            {
                double acc = 0.;
                for (int j = 0; j < NX; j++)
                    acc += lds.Nm[j * NR + r] * lds.Bf[j * NU + a];
                lds.Br[r * NU + a] = acc;
            }
        }
    }
    else
    {
        if (r < NR)
        {
            for (int c = 0; c < NR; c++)
            {
                lds.S[L::OFF_AR + r * NR + c] = lds.S[L::OFF_A + r * NX + c];
                lds.S[L::OFF_QR + r * NR + c] = (c == r) ? q[r] : 0.;
            }
            for (int a = 0; a < NU; a++)
                lds.Br[r * NU + a] = lds.Bf[r * NU + a];
        }
    }
    WAVE_SYNC();

    // ---- 2. Hamiltonian M = [[A, -B R^-1 B'], [-Q, -A']]   (LQR.cpp:75-76), row r in lane r ----
    double M[N2];
#pragma unroll
    for (int c = 0; c < N2; c++)
        M[c] = 0.;
    if (r < NR)
    {
#pragma unroll
        for (int c = 0; c < NR; c++)
        {
            M[c] = lds.S[L::OFF_AR + r * NR + c];
            double acc = 0.;
            for (int a = 0; a < NU; a++)
                acc += lds.Br[r * NU + a] * rinv[a] * lds.Br[c * NU + a];
            M[NR + c] = -acc;
        }
    }
    else if (r < N2)
    {
#pragma unroll
        for (int c = 0; c < NR; c++)
        {
            M[c] = -lds.S[L::OFF_QR + (r - NR) * NR + c];
            M[NR + c] = -lds.S[L::OFF_AR + c * NR + (r - NR)];
        }
    }
    WAVE_SYNC();

    // ---- 3. matrix sign function: M <- M - 0.5 (M - M^-1) until isApprox(Mnew, M, 1e-8)   (LQR.cpp:14-31) ----
    int st = ST_OK, it = 0;
    for (;;)
    {
        if (it > SIGN_MAX_ITERATIONS)
        {
            st = ST_ITERATION_LIMIT;
            break;
        }
        double W[N2];
#pragma unroll
        for (int c = 0; c < N2; c++)
            W[c] = M[c];
        int piv[N2], myStep;
        const bool ok = gaussJordan<N2, N2, true>(W, N2, r, base, piv, myStep);
        // undo the pivot permutation: lane piv[j], register c holds inverse[j][piv[c]]
        if (myStep >= 0)
        {
#pragma unroll
            for (int c = 0; c < N2; c++)
                lds.S[myStep * N2 + piv[c]] = W[c];
        }
        WAVE_SYNC();
        double d2 = 0., a2 = 0., b2 = 0.;
        if (r < N2)
        {
#pragma unroll
            for (int c = 0; c < N2; c++)
            {
                const double inv = lds.S[r * N2 + c];
                const double mn = M[c] - 0.5 * (M[c] - inv);
                const double d = mn - M[c];
                d2 += d * d;
                a2 += mn * mn;
                b2 += M[c] * M[c];
                M[c] = mn;
            }
        }
        WAVE_SYNC();
        d2 = halfSum(d2);
        a2 = halfSum(a2);
        b2 = halfSum(b2);
        it++;
        if (!ok || !isFinite(d2) || !isFinite(a2))
        {
            st = ST_NONFINITE;
            break;
        }
        if (d2 <= SIGN_EPS * SIGN_EPS * (a2 < b2 ? a2 : b2)) // Eigen isApprox: |a - b|_F^2 <= eps^2 min(|a|_F^2, |b|_F^2)
            break;
    }

    // ---- 4. P from [M12; M22 + I] P = -[M11 + I; M21]   (LQR.cpp:33-53): elimination with row pivoting over the 2n rows of the consistent
    //         system (the reference's full-pivot LU picks its n rows the same way) ----
    double T[N2];
#pragma unroll
    for (int c = 0; c < NR; c++)
    {
        T[c] = M[NR + c] + ((r == NR + c) ? 1. : 0.);
        T[NR + c] = -(M[c] + ((r == c) ? 1. : 0.));
    }
    int pivs[NR], myStep;
    const bool ok = gaussJordan<N2, NR, false>(T, N2, r, base, pivs, myStep);
    if (myStep >= 0)
    {
#pragma unroll
        for (int c = 0; c < NR; c++)
            lds.S[myStep * NR + c] = T[NR + c]; // P[myStep][c]
    }
    WAVE_SYNC();
    // ---- 5. K = R^-1 B'P   (LQR.cpp:104), K = K_r N' on a tangent system ----
    double kout[NU];
    int bad = (ok && st == ST_OK) ? 0 : 1;
    if (r < NR)
    {
#pragma unroll
        for (int a = 0; a < NU; a++)
        {
            double acc = 0.;
            for (int j = 0; j < NR; j++)
                acc += lds.Br[j * NU + a] * lds.S[j * NR + r];
            kout[a] = rinv[a] * acc;
            lds.Kr[a * NR + r] = kout[a];
        }
    }
    WAVE_SYNC();
    if constexpr (P::LQR_TANGENT)
    {
        if (r < NX)
        {
#pragma unroll
            for (int a = 0; a < NU; a++)
            {
                double acc = 0.;
                for (int c = 0; c < NR; c++)
                    acc += lds.Kr[a * NR + c] * lds.Nm[r * NR + c];
                kout[a] = acc;
            }
        }
    }
    if (r < NX)
        for (int a = 0; a < NU; a++)
            if (!isFinite(kout[a]))
                bad = 1;
    bad = halfOr(bad);
    if (bad && st == ST_OK)
        st = ST_NONFINITE;
    if (valid)
    {
        // a failed node never writes a non-finite gain: zeros and its status
        if (r < NX)
            for (int a = 0; a < NU; a++)
                G[(node * NU + a) * NX + r] = (st == ST_OK) ? kout[a] : 0.;
        if (r == 0)
        {
            status[node] = st;
            iters[node] = it;
        }
    }
}

// One closed loop per flight (one thread each: the state, the stage slopes and the gain row products live in registers).  F flights, `samples`
// per trajectory: flight f follows trajectory f / samples (its X, U, T, G, parameter row and limits row) from its own x_start[f]; nothing is
// replicated.
//   X [B][K][nx], U [B][uRows][nu] (nU rows used), T [B], par [B][np], G [B][K][nu][nx], x_start [F][nx], x_final [nx]; stop_tol > 0: also stop once
//   |x - x_final| < stop_tol (the regulator loop of LQR_sim.cpp:43-82, run on a constant two-node "trajectory")
//   out_x [F][nx], out_u [F][nu], out_s [F][4] = (t, |x_start - x_final|, |x_end - x_final|, max |x - x_ref|), out_i [F][2] = (steps, status)
//   record (first n_record flights, every write_steps-th step): rec_x [n_record][rec_cap][nx], rec_u [..][nu], rec_t [..], rec_n [n_record]
//   SAT: u = P::saturate(u_cmd) with the row lim [B or 1][LIM_ROW] of the trajectory; out_nsat [F] = plant steps with u != u_cmd, out_clip [F] =
//   largest |u_cmd - u|.  SAT == false reads and writes none of the three (the host zeroes the two outputs) and is the loop as it was.
//   HOLD: the feedback term is held over a segment (scpp_hip_lqr_set_feedback_hold): du = -G[i] (x - x_ref(t)) is latched at the first plant step
//   whose segment index i differs from the latched one (flight start included) and u_cmd = u_ref(t) + du on every plant step; everything else as
//   without it.  HOLD == false is the loop as it was.
//   FF: the affine law's second term (scpp_hip_lqr_set_feedforward): u_cmd = u_ref(t) - K_t (x - x_ref(t)) - k_t with k_t = ff[i] + a (ff[iu1] - ff[i]),
//   ff [B][K][nu] the row of the flight's trajectory, interpolated with the indices and the fraction of the gain; limits, record, stop tolerance
//   and the non-finite retirement act on this u_cmd.  FF == false reads no ff and is the loop as it was; FF with HOLD is not defined (the host
//   refuses it).
//   NOISE: the disturbed plant (scpp_hip_lqr_set_disturbance): plant step n = `steps` of flight b integrates dx/dt = f(x, u) + d with
//   d_r = nsd[r] z_r, nsd [nx] = sqrt(w_r / time_step) (the host computes it, so every build multiplies with the same number) and z the normals
//   of (seed, flight_offset + b, n, r); d is drawn once u is decided (sat included), is constant over the plant step and is added to the slope
//   of every stage of every substep.  NOISE == false reads none of the three arguments and is the loop as it was.
template <class P, bool SAT, bool HOLD = false, bool FF = false, bool NOISE = false>
__global__ void __launch_bounds__(WAVE) lqr_track_kernel(int B, int samples, int K, int nU, int uRows, const double *__restrict__ X, const double *__restrict__ U, const double *__restrict__ T,
                                 const double *__restrict__ par, int par_stride, const double *__restrict__ G,
                                 const double *__restrict__ x_start, const double *__restrict__ x_final, double time_step, int substeps,
                                 double stop_tol, int max_steps, int n_record, int write_steps, int rec_cap, double *__restrict__ out_x,
                                 double *__restrict__ out_u, double *__restrict__ out_s, int *__restrict__ out_i, double *__restrict__ rec_x,
                                 double *__restrict__ rec_u, double *__restrict__ rec_t, int *__restrict__ rec_n,
                                 const double *__restrict__ lim, int lim_stride, int *__restrict__ out_nsat, double *__restrict__ out_clip,
                                 const double *__restrict__ ff, const double *__restrict__ nsd, unsigned long long seed,
                                 unsigned long long flight_offset)
{
    static_assert(!(FF && HOLD), "the held loop's offset is another recursion");
    using Model = typename P::Model;
    constexpr int NX = Model::NX, NU = Model::NU, NP = Model::NP;
    const long b = long(blockIdx.x) * blockDim.x + threadIdx.x;
    if (b >= B)
        return;
    const long tr = b / samples; // the trajectory of this flight
    const bool foh = (nU == K);
    double p[NP], y[NX], u[NU], xf[NX], kk[RK_S][NX];
    for (int j = 0; j < NP; j++)
        p[j] = par[tr * par_stride + j];
    double lm[SAT ? LIM_ROW : 1];
    int n_sat = 0;
    double max_clip = 0.;
    if constexpr (SAT)
        for (int j = 0; j < LIM_ROW; j++)
            lm[j] = lim[tr * lim_stride + j];
    bool finite = true;
    double e0 = 0.;
    for (int j = 0; j < NX; j++)
    {
        y[j] = x_start[b * NX + j];
        xf[j] = x_final[j];
        finite = finite && isFinite(y[j]);
        e0 += (y[j] - xf[j]) * (y[j] - xf[j]);
    }
    for (int j = 0; j < NU; j++)
        u[j] = 0.;
    const double t_max = T[tr];
    finite = finite && isFinite(t_max);
    const double *Xb = X + tr * K * NX, *Ub = U + tr * uRows * NU, *Gb = G + tr * K * NU * NX;
    double t = 0., max_dev = 0.;
    int steps = 0, st = ST_OK, nrec = 0;
    double du[HOLD ? NU : 1];
    long latched = -1; // HOLD: the segment du was latched in
    if (!finite)
    {
        st = ST_NONFINITE; // retires at once (the reference throws "State has NaN", SC_tracking.cpp:71-74): zeros, no non-finite output
        for (int j = 0; j < NX; j++)
            y[j] = 0.;
        e0 = 0.;
    }
    const double dt = t_max / double(K - 1);
    const double h = time_step / double(substeps);
    while (st == ST_OK && t < t_max)
    {
        if (steps >= max_steps)
        {
            st = ST_STEP_CAP;
            break;
        }
        // LQRTracker::getInput (LQRTracker.cpp:43-65), trajectoryData.hpp:41-78
        const double tc = t < 0. ? 0. : (t > t_max ? t_max : t);
        const double a = fmod(tc, dt) / dt;
        long i = long(tc / dt);
        if (i > K - 2)
            i = K - 2; // tc / dt can round up to K-1 just below t_max, where the reference reads X.at(K): clamped
        const long i1 = i + 1, iu1 = foh ? i + 1 : i;
        double dx[NX], un[NU], dev = 0.;
        for (int j = 0; j < NX; j++)
        {
            const double x0 = Xb[i * NX + j], x1 = Xb[i1 * NX + j];
            dx[j] = y[j] - (x0 + a * (x1 - x0));
            dev += dx[j] * dx[j];
        }
        dev = sqrt(dev);
        max_dev = dev > max_dev ? dev : max_dev;
        if constexpr (HOLD)
        {
            if (i != latched)
            {
                for (int c = 0; c < NU; c++)
                {
                    double acc = 0.;
                    for (int j = 0; j < NX; j++)
                        acc += Gb[(i * NU + c) * NX + j] * dx[j];
                    du[c] = -acc;
                }
                latched = i;
            }
            for (int c = 0; c < NU; c++)
            {
                const double u0 = Ub[i * NU + c], u1 = Ub[iu1 * NU + c];
                un[c] = du[c] + (u0 + a * (u1 - u0));
            }
        }
        else
        {
            for (int c = 0; c < NU; c++)
            {
                const double u0 = Ub[i * NU + c], u1 = Ub[iu1 * NU + c];
                double acc = 0.;
                for (int j = 0; j < NX; j++)
                {
                    const double g0 = Gb[(i * NU + c) * NX + j], g1 = Gb[(iu1 * NU + c) * NX + j];
                    acc += (g0 + a * (g1 - g0)) * dx[j];
                }
                un[c] = -acc + (u0 + a * (u1 - u0));
                if constexpr (FF)
                {
                    const double *Fb = ff + tr * K * NU;
                    const double f0 = Fb[i * NU + c], f1 = Fb[iu1 * NU + c];
                    un[c] = un[c] - (f0 + a * (f1 - f0));
                }
            }
        }
        bool ufin = true;
        for (int c = 0; c < NU; c++)
            ufin = ufin && isFinite(un[c]);
        if (!ufin)
        {
            st = ST_NONFINITE; // a non-finite reference node, input or gain (a failed solver instance): the last applied input is kept
            break;
        }
        for (int c = 0; c < NU; c++)
            u[c] = un[c];
        if constexpr (SAT)
        {
            P::saturate(u, lm);
            bool clipped = false;
            double d2 = 0.;
            for (int c = 0; c < NU; c++)
            {
                const double d = un[c] - u[c];
                const double dd = d * d;
                clipped = clipped || (u[c] != un[c]);
                d2 = d2 + dd;
            }
            if (clipped)
            {
                const double clip = sqrt(d2);
                n_sat++;
                max_clip = clip > max_clip ? clip : max_clip;
            }
        }
        double d[NOISE ? NX : 1];
        if constexpr (NOISE)
            for (int j = 0; 2 * j < NX; j++)
            {
                double z0, z1;
                noiseNormalPair(seed, flight_offset + (unsigned long long)(b), uint32_t(steps), uint32_t(j), z0, z1);
                d[2 * j] = nsd[2 * j] * z0;
                if (2 * j + 1 < NX)
                    d[2 * j + 1] = nsd[2 * j + 1] * z1;
            }
        // scpp::simulate(model, time_step, u, u, x)   (simulation.cpp:25-42: RKF78, fixed steps; the input is constant over the step)
        double yn[NX];
        for (int j = 0; j < NX; j++)
            yn[j] = y[j];
        for (int step = 0; step < substeps; step++)
        {
#pragma unroll
            for (int s = 0; s < RK_S; s++)
            {
                double ys[NX];
                for (int j = 0; j < NX; j++)
                {
                    double acc = 0.;
#pragma unroll
                    for (int qq = 0; qq < s; qq++)
                        if (RK_A[s][qq] != 0.)
                            acc += RK_A[s][qq] * kk[qq][j];
                    ys[j] = yn[j] + h * acc;
                }
                Model::template systemFlowMap<double>(ys, u, p, kk[s]);
                if constexpr (NOISE)
                    for (int j = 0; j < NX; j++)
                        kk[s][j] += d[j];
            }
            for (int j = 0; j < NX; j++)
            {
                double acc = 0.;
#pragma unroll
                for (int s = 0; s < RK_S; s++)
                    if (RK_B[s] != 0.)
                        acc += RK_B[s] * kk[s][j];
                yn[j] += h * acc;
            }
        }
        bool fin = true;
        for (int j = 0; j < NX; j++)
            fin = fin && isFinite(yn[j]);
        if (!fin)
        {
            st = ST_NONFINITE; // keeps the last finite state
            break;
        }
        for (int j = 0; j < NX; j++)
            y[j] = yn[j];
        t += time_step;
        if (b < n_record && steps % write_steps == 0 && nrec < rec_cap)
        {
            const long o = b * rec_cap + nrec;
            for (int j = 0; j < NX; j++)
                rec_x[o * NX + j] = y[j];
            for (int j = 0; j < NU; j++)
                rec_u[o * NU + j] = u[j];
            rec_t[o] = t;
            nrec++;
        }
        steps++;
        if (stop_tol > 0.) // regulator mode: LQR_sim.cpp:78-81
        {
            double e = 0.;
            for (int j = 0; j < NX; j++)
                e += (y[j] - xf[j]) * (y[j] - xf[j]);
            if (sqrt(e) < stop_tol)
                break;
        }
    }
    double e1 = 0.;
    for (int j = 0; j < NX; j++)
    {
        out_x[b * NX + j] = y[j];
        e1 += (y[j] - xf[j]) * (y[j] - xf[j]);
    }
    for (int j = 0; j < NU; j++)
        out_u[b * NU + j] = u[j];
    const bool nan_start = !finite;
    out_s[b * 4 + 0] = t;
    out_s[b * 4 + 1] = nan_start ? 0. : sqrt(e0);
    out_s[b * 4 + 2] = nan_start ? 0. : sqrt(e1);
    out_s[b * 4 + 3] = max_dev;
    out_i[b * 2 + 0] = steps;
    out_i[b * 2 + 1] = st;
    if (b < n_record)
        rec_n[b] = nrec;
    if constexpr (SAT)
    {
        out_nsat[b] = n_sat;
        out_clip[b] = max_clip;
    }
}

} // namespace lqr
} // namespace scpp

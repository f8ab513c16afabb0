// Covariance of the sampled-data loop: the discrete covariance recursion swept forwards along every trajectory (include/scpp_hip_lqr.h,
// scpp_hip_lqr_propagate_covariance_discrete).  The correction du_i = -G[i] dx(t_i) is held over segment i, so
//
//   d[Phi | Gamma]/dt = A(t) [Phi | Gamma] + [0 | B(t)],   [Phi | Gamma](t_i) = [I | 0]        (the discrete gain sweep's own equation)
//   dM/dt = A(t) M + M A(t)' + W,   M(t_i) = 0,   Wd_i = M(t_{i+1})                             (A open loop: the held input does not react)
//   Acl_i = Phi_i - Gamma_i G[i],   S_{i+1} = Acl_i S_i Acl_i' + Wd_i,   S_0 = sigma0,          input covariance of node k: G[k] S_k G[k]'
//
// Mapping: ONE WAVEFRONT PER TRAJECTORY, S, Phi and M one 16 x 16 FP64 tile each in the accumulator layout (lqr_tile_sweep.h).
// TWO PASSES PER SEGMENT, each with the register footprint of a kernel that exists: M by rkf78TileStep on covarianceRhs (the continuous
// covariance sweep's right-hand side with A for A_cl, so M is symmetric to the bit), then [Phi | Gamma] by integrateTransition /
// integrateTransitionLane of the discrete gain sweep (RocketQuat, 14 + 4 > 16: Gamma one entry per lane).  The Jacobian is evaluated twice
// per stage; the one-pass shape (26 stage-slope tiles, 104 doubles per lane beside the Jacobian rows) was not built: the discrete gain
// kernel alone needs 228 of the 256 registers of two wavefronts per SIMD, so a second set of thirteen slopes does not fit without scratch.
// With W = 0 (w all zero; wave-uniform) the first pass is skipped as a whole and Wd is the zero tile, which is bitwise what it integrates to.
//
// The transpose rule of lqr_discrete_kernel.h, mfma(X, Y) = X'Y, gives Acl'S Acl from Acl, not Acl S Acl'; so the recursion runs on Acl':
//     Phi'              read back transposed from the LDS copy of the tile (ONE exchange per segment, the only one besides the symmetrisation)
//     (Gamma G)'        1   (A operand: G[g][col], B operand: Gamma[col][g]; the same two numbers per lane, the other way round, give Gamma G)
//     V = S Acl'        4   (A operand: S, symmetric)
//     F = Acl V         4   (A operand: Acl')
//     node k            8   S G' and G (S G'), as the continuous sweep
// F is symmetric only to rounding; it is SYMMETRISED ONCE PER NODE through LDS, F <- (F + F') / 2, as the discrete gain kernel treats
// Phi'(P Phi).  Wd and sigma0 are symmetric to the bit, so S is, at every node.
//
// Registers, from the compiler's kernel-resource-usage report (hipcc -O3, gfx950).  __launch_bounds__(64, 2), the discrete gain kernel's, holds
// the compiler to 256 registers per lane.  No scratch and no vector-register spill for any model; scalar values the compiler parks in lanes of
// a vector register (its "SGPRs Spill": 103 / 123 / 105 below, 99 / 107 / 99 in the discrete gain kernel) never touch memory.
//                   VGPR   AGPR   scratch bytes/lane   wavefronts per SIMD   LDS bytes
//     Lander3dof     170      0                    0                     2        6080
//     Rocket2D       200      0                    0                     2        6080
//     RocketQuat     229      0                    0                     2        6080
#pragma once
#include "lqr_covariance_kernel.h"
#include "lqr_discrete_kernel.h"

namespace scpp
{
namespace lqr
{

constexpr int COVARIANCE_DISCRETE_WAVES_PER_SIMD = 2; // as the discrete gain kernel, whose transition pass this kernel runs

// One sweep per trajectory; arguments, outputs and failure rules as lqr_covariance_kernel.  Segment i (nodes i, i+1) is integrated from a = 0 up
// to a = 1 with x = X[i] + a (X[i+1] - X[i]), u = U[i] + a (U[j] - U[i]), j = i+1 (first-order) or i (zero-order); the segment index is the loop's,
// never derived from a time.  The gain of segment i is G[i], whatever the input hold.
template <class P>
__global__ void __launch_bounds__(WAVE, COVARIANCE_DISCRETE_WAVES_PER_SIMD)
    lqr_covariance_discrete_kernel(int K, int nU, int uRows, int steps, const double *__restrict__ X, const double *__restrict__ U,
                                   const double *__restrict__ T, const double *__restrict__ par, int par_stride, const double *__restrict__ G,
                                   const int *__restrict__ gstatus, const double *__restrict__ S0, int s0_stride, const double *__restrict__ w,
                                   double *__restrict__ sd, double *__restrict__ icov, double *__restrict__ fcov, int *__restrict__ status,
                                   double *__restrict__ cov)
{
    using Model = typename P::Model;
    using JR = typename Model::JacobianRows;
    constexpr int NX = Model::NX, NU = Model::NU, NP = Model::NP;
    constexpr bool ONE_TILE = NX + NU <= RT;
    static_assert(NX <= RT && NU <= 4, "S is one 16 x 16 tile, the gain one 4-row chunk");
    __shared__ DiscreteLds lds;
    const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
    const long b = blockIdx.x;
    const bool foh = (nU == K);
    const double *Xb = X + b * K * NX, *Ub = U + b * uRows * NU;
    const ForwardIo io = forwardIo<NX, NU>(b, K, G, nullptr, sd, icov, fcov, cov, nullptr, nullptr);

    for (int e = lane; e < RT * RT; e += WAVE)
        lds.At[e] = 0.;
    lds.Bm[lane] = 0.;
    double p[NP], aux[JR::NAUX > 0 ? JR::NAUX : 1];
    loadParameters<P>(par, b, par_stride, p, aux);
    const d4_t wd = diagonalTile<NX>(lane, w);
    bool noise = false; // wave-uniform: every lane reads all of w
    for (int j = 0; j < NX; j++)
        noise = noise || w[j] != 0.;
    int bad = 0, incomplete;
    d4_t Sc = loadInitialTile<NX, false>(lane, S0 + b * s0_stride, nullptr, bad);
    const double t_max = T[b];
    scanForwardInputs<NX, NU, false>(lane, t_max, Xb, Ub, K, nU, io, gstatus ? gstatus + b * K : nullptr, bad, incomplete);
    WAVE_SYNC();

    const double h = t_max / double(K - 1) / double(steps);
    int kfail = bad ? 0 : K; // nodes kfail..K-1 carry zeros
    for (int k = 0; k < K && kfail == K; k++)
    {
        if (k > 0)
        {
            const int i = k - 1;
            loadSegment<NX, NU>(lds.seg, lane, Xb, Ub, i, foh ? k : i);
            WAVE_SYNC();
            // ---- pass 1: Wd_i = M(t_k), `steps` RKF78 steps from M = 0; skipped as a whole without a disturbance ----
            d4_t Md = {0., 0., 0., 0.};
            if (noise)
                for (int n = 0; n < steps; n++)
                    rkf78TileStep(Md, h, [&](int s, const d4_t Ms) __attribute__((always_inline)) {
                        const double a = (double(n) + RK_C[s]) / double(steps);
                        double Ac[4];
                        d4_t Ct;
                        transitionJacobian<P>(lds, lane, a, p, aux, Ac, Ct);
                        return covarianceRhs(Ms, Ac, wd);
                    });
            // ---- pass 2: [Phi | Gamma] of the segment; afterwards PhT is the lane's share of Phi' and ga its entry Gamma[col][g] ----
            d4_t Ph, PhT;
            double ga;
            int nf = tileNonFinite(Md);
#pragma unroll
            for (int r = 0; r < 4; r++)
                Ph[r] = (4 * r + g == col && col < NX) ? 1. : 0.;
            if constexpr (ONE_TILE)
            {
                integrateTransition<P>(lds, lane, steps, h, p, aux, Ph);
                nf |= tileNonFinite(Ph);
#pragma unroll
                for (int r = 0; r < 4; r++)
                    lds.M[(4 * r + g) * RT + col] = Ph[r];
                WAVE_SYNC();
                ga = g < NU ? lds.M[col * RT + NX + (g < NU ? g : 0)] : 0.;
            }
            else
            {
                double gam = 0.;
                integrateTransitionLane<P>(lds, lane, steps, h, p, aux, Ph, gam);
                nf |= tileNonFinite(Ph) | (isFinite(gam) ? 0 : 1);
                lds.Gs[lane] = gam;
#pragma unroll
                for (int r = 0; r < 4; r++)
                    lds.M[(4 * r + g) * RT + col] = Ph[r];
                WAVE_SYNC();
                ga = g < NU ? lds.Gs[col * 4 + (g < NU ? g : 0)] : 0.;
            }
#pragma unroll
            for (int r = 0; r < 4; r++)
            {
                const bool in = 4 * r + g < NX && col < NX;
                PhT[r] = in ? lds.M[col * RT + 4 * r + g] : 0.;
            }
            WAVE_SYNC();
            if (waveOr(nf))
            {
                kfail = k;
                break;
            }
            // ---- one step of the recursion: S_i -> S_k = Acl S_i Acl' + Wd ----
            const bool inG = g < NU && col < NX;
            const double gg = inG ? io.Gb[(i * NU + (inG ? g : 0)) * NX + (inG ? col : 0)] : 0.;
            d4_t AclT = {0., 0., 0., 0.};
            AclT = __builtin_amdgcn_mfma_f64_16x16x4f64(gg, ga, AclT, 0, 0, 0); // (Gamma G)': register r of lane l is (Gamma G)[col][4r + g]
#pragma unroll
            for (int r = 0; r < 4; r++)
                AclT[r] = PhT[r] - AclT[r];
            const d4_t V = tileTransposeProduct(Sc, AclT);
            const d4_t F = tileTransposeProduct(AclT, V);
#pragma unroll
            for (int r = 0; r < 4; r++)
                lds.M[(4 * r + g) * RT + col] = F[r];
            WAVE_SYNC();
#pragma unroll
            for (int r = 0; r < 4; r++)
                Sc[r] = 0.5 * (F[r] + lds.M[col * RT + 4 * r + g]) + Md[r];
            WAVE_SYNC();
        }
        if (!forwardNode<NX, NU, false>(lane, k, Sc, io))
        {
            kfail = k;
            break;
        }
    }
    forwardEpilogue<NX, NU, false>(lane, K, kfail, incomplete, Sc, io, status + b);
}

} // namespace lqr
} // namespace scpp

// The frame around a sweep's own segment advance, written once for every kernel that sweeps a tile along a trajectory.
//
// FORWARDS (lqr_covariance_kernel, lqr_moments_kernel, lqr_covariance_discrete_kernel): the load of S0 into the tile, the scan of the inputs,
// the node block and the epilogue.  MEAN = true is the moments sweep: the tile carries m in its border (row and column NX), the node block
// also writes m(t_k) and du_mean[k], the scan also reads the feedforward terms and mean0.  With MEAN = false nothing of that is compiled.
// BACKWARDS (lqr_riccati_kernel, lqr_affine_kernel, lqr_discrete_kernel): the model's parameters, the mark of a node that came out, and
// the zero-fill of the nodes that did not.
// The failure rule, both ways: nothing non-finite is ever written.  The node a tile goes non-finite at, and every node the sweep has not
// reached by then, carry zeros (and, backwards, ST_NONFINITE per node; forwards, one status per trajectory).
#pragma once
#include "lqr_tile_sweep.h"

namespace scpp
{
namespace lqr
{

constexpr int ST_GAINS_INCOMPLETE = 2;

// p [NP] and aux = JacobianRows::prepare(p) of trajectory b
template <class P>
__device__ __forceinline__ void loadParameters(const double *par, long b, int par_stride, double (&p)[P::Model::NP],
                                               double (&aux)[P::Model::JacobianRows::NAUX > 0 ? P::Model::JacobianRows::NAUX : 1])
{
    for (int j = 0; j < P::Model::NP; j++)
        p[j] = par[b * par_stride + j];
    P::Model::JacobianRows::prepare(p, aux);
}

// ---- forwards ----

// one trajectory's share of a forward sweep's arrays.  Fb (feedforward terms), mb and dub belong to the moments sweep; cvb == nullptr: not kept
struct ForwardIo
{
    const double *Gb, *Fb;
    double *sdb, *icb, *fcb, *cvb, *mb, *dub;
};
template <int NX, int NU>
__device__ __forceinline__ ForwardIo forwardIo(long b, int K, const double *G, const double *FF, double *sd, double *icov, double *fcov, double *cov,
                                               double *mean, double *dumean)
{
    return {G + b * K * NU * NX,
            FF ? FF + b * K * NU : nullptr,
            sd + b * K * NX,
            icov + b * K * NU * NU,
            fcov + b * NX * NX,
            cov ? cov + b * K * NX * NX : nullptr,
            mean ? mean + b * K * NX : nullptr,
            dumean ? dumean + b * K * NU : nullptr};
}

// the entry of m that the tile holds at (row, col): column NX above the corner, row NX left of it; -1 elsewhere
template <int NX>
__device__ __forceinline__ int meanIndex(int row, int col)
{
    return (col == NX && row < NX) ? row : ((row == NX && col < NX) ? col : -1);
}

// the tile at node 0: S0b [NX][NX] in the corner, zeros around it; MEAN: M0b [NX] in the border (nullptr: mean0 = 0), judged into `bad`
template <int NX, bool MEAN>
__device__ __forceinline__ d4_t loadInitialTile(int lane, const double *S0b, const double *M0b, int &bad)
{
    const int g = lane >> 4, col = lane & 15;
    d4_t Tc;
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        const int row = 4 * r + g;
        const bool in = row < NX && col < NX;
        double v = in ? S0b[in ? row * NX + col : 0] : 0.;
        if constexpr (MEAN)
        {
            const int mi = meanIndex<NX>(row, col);
            if (mi >= 0 && M0b)
            {
                v = M0b[mi];
                bad |= isFinite(v) ? 0 : 1;
            }
        }
        Tc[r] = v;
    }
    return Tc;
}

// bad: the final time, a state, an input, a gain or (MEAN, Fb given) a feedforward term is not finite, on top of what the caller found;
// incomplete: a gain carries a status other than ST_OK (gstatus_b == nullptr: gains without a status).  Both reduced over the wave.
template <int NX, int NU, bool MEAN>
__device__ __forceinline__ void scanForwardInputs(int lane, double t_max, const double *Xb, const double *Ub, int K, int nU, const ForwardIo &io,
                                                  const int *gstatus_b, int &bad, int &incomplete)
{
    bad |= referenceNonFinite<NX, NU>(lane, t_max, Xb, Ub, K, nU);
    for (int e = lane; e < K * NU * NX; e += WAVE)
        bad |= isFinite(io.Gb[e]) ? 0 : 1;
    if constexpr (MEAN)
        if (io.Fb)
            for (int e = lane; e < K * NU; e += WAVE)
                bad |= isFinite(io.Fb[e]) ? 0 : 1;
    incomplete = 0;
    if (gstatus_b)
        for (int e = lane; e < K; e += WAVE)
            incomplete |= gstatus_b[e] != ST_OK ? 1 : 0;
    bad = waveOr(bad);
    incomplete = waveOr(incomplete);
}

// the lane's share of the gain tile of node k (rows >= nu and columns >= nx zero): G[col][4c + g]
template <int NX, int NU>
__device__ __forceinline__ void loadGainTile(int lane, int k, const double *Gb, double (&Gt)[4])
{
    const int g = lane >> 4, col = lane & 15;
#pragma unroll
    for (int c = 0; c < 4; c++)
    {
        const bool in = col < NU && 4 * c + g < NX;
        Gt[c] = in ? Gb[(k * NU + (in ? col : 0)) * NX + (in ? 4 * c + g : 0)] : 0.;
    }
}

// G T G' = G (T G') of a symmetric tile T, 8 matrix-core instructions: register 0 of lane l is (G T G')[g][col]; Wp = T G' is handed out too
// (register r of lane l: (T G')[4r + g][col]).  forwardNode below keeps its own copy of these lines: the kernels that call it are compiled
// exactly as they were before this helper existed.
__device__ __forceinline__ d4_t gainCongruence(const d4_t &Tc, const double (&Gt)[4], d4_t &Wp)
{
    d4_t Sk = {0., 0., 0., 0.};
    Wp = Sk;
#pragma unroll
    for (int c = 0; c < 4; c++)
        Wp = __builtin_amdgcn_mfma_f64_16x16x4f64(Tc[c], Gt[c], Wp, 0, 0, 0);
#pragma unroll
    for (int c = 0; c < 4; c++)
        Sk = __builtin_amdgcn_mfma_f64_16x16x4f64(Gt[c], Wp[c], Sk, 0, 0, 0);
    return Sk;
}

// node k: the tile, its standard deviations and the input covariance G[k] S G[k]' = G (S G')  (8 matrix-core instructions); MEAN: S G' carries
// (G m)' in row NX, so m(t_k) and du_mean[k] = -G[k] m(t_k) - [FF[k]] come with it.  false, and nothing written, if anything is not finite.
template <int NX, int NU, bool MEAN>
__device__ __forceinline__ bool forwardNode(int lane, int k, const d4_t &Tc, const ForwardIo &io)
{
    const int g = lane >> 4, col = lane & 15;
    double Gt[4]; // the lane's share of the gain tile (rows >= nu and column NX zero): G[col][4c + g]
#pragma unroll
    for (int c = 0; c < 4; c++)
    {
        const bool in = col < NU && 4 * c + g < NX;
        Gt[c] = in ? io.Gb[(k * NU + (in ? col : 0)) * NX + (in ? 4 * c + g : 0)] : 0.;
    }
    d4_t Wp = {0., 0., 0., 0.}, Sk = {0., 0., 0., 0.};
#pragma unroll
    for (int c = 0; c < 4; c++)
        Wp = __builtin_amdgcn_mfma_f64_16x16x4f64(Tc[c], Gt[c], Wp, 0, 0, 0); // T G': register r of lane l is (T G')[4r + g][col]
#pragma unroll
    for (int c = 0; c < 4; c++)
        Sk = __builtin_amdgcn_mfma_f64_16x16x4f64(Gt[c], Wp[c], Sk, 0, 0, 0); // register 0 of lane l is (G S G')[g][col]
    int nf = isFinite(Sk[0]) ? 0 : 1;
    [[maybe_unused]] double du = 0.; // the lane of row NX, column q < nu: du_mean[k][q]
    if constexpr (MEAN)
    {
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (4 * r + g == NX && col < NU)
                du = io.Fb ? -Wp[r] - io.Fb[k * NU + col] : -Wp[r];
        nf |= isFinite(du) ? 0 : 1;
    }
#pragma unroll
    for (int r = 0; r < 4; r++)
        nf |= isFinite(Tc[r]) ? 0 : 1;
    if (waveOr(nf))
        return false;
    if (io.cvb)
        storeTile<NX>(lane, io.cvb + k * NX * NX, Tc);
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        if (4 * r + g == col && col < NX)
            io.sdb[k * NX + col] = sqrt(Tc[r] > 0. ? Tc[r] : 0.); // a diagonal entry negative from rounding: 0
        if constexpr (MEAN)
        {
            if (col == NX && 4 * r + g < NX)
                io.mb[k * NX + 4 * r + g] = Tc[r];
            if (4 * r + g == NX && col < NU)
                io.dub[k * NU + col] = du;
        }
    }
    if (g < NU && col < NU)
        io.icb[(k * NU + g) * NU + col] = Sk[0];
    return true;
}

// zeros for nodes kfail..K-1 (kfail == K: none), the final tile (zeros after a failure) and the trajectory's status
template <int NX, int NU, bool MEAN>
__device__ __forceinline__ void forwardEpilogue(int lane, int K, int kfail, int incomplete, const d4_t &Tc, const ForwardIo &io, int *status_b)
{
    for (int e = kfail * NX + lane; e < K * NX; e += WAVE)
    {
        io.sdb[e] = 0.;
        if constexpr (MEAN)
            io.mb[e] = 0.;
    }
    for (int e = kfail * NU * NU + lane; e < K * NU * NU; e += WAVE)
        io.icb[e] = 0.;
    if constexpr (MEAN)
        for (int e = kfail * NU + lane; e < K * NU; e += WAVE)
            io.dub[e] = 0.;
    if (io.cvb)
        for (int e = kfail * NX * NX + lane; e < K * NX * NX; e += WAVE)
            io.cvb[e] = 0.;
    const d4_t zero = {0., 0., 0., 0.};
    storeTile<NX>(lane, io.fcb, kfail == K ? Tc : zero);
    if (lane == 0)
        *status_b = kfail < K ? ST_NONFINITE : (incomplete ? ST_GAINS_INCOMPLETE : ST_OK);
}

// ---- backwards ----

// node k came out: its status, and the RKF78 steps behind it
__device__ __forceinline__ void markNodeOk(int lane, int *status_b, int *iters_b, int k, int steps_behind)
{
    if (lane == 0)
    {
        status_b[k] = ST_OK;
        iters_b[k] = steps_behind;
    }
}

// zeros and ST_NONFINITE for nodes 0..kfail (kfail == -1: none): gains, P (Pb == nullptr: not kept), status and iters
template <int NX, int NU>
__device__ __forceinline__ void backwardEpilogue(int lane, int kfail, double *Gb, double *Pb, int *status_b, int *iters_b)
{
    for (int e = lane; e < (kfail + 1) * NU * NX; e += WAVE)
        Gb[e] = 0.;
    if (Pb)
        for (int e = lane; e < (kfail + 1) * NX * NX; e += WAVE)
            Pb[e] = 0.;
    for (int e = lane; e <= kfail; e += WAVE)
    {
        status_b[e] = ST_NONFINITE;
        iters_b[e] = 0;
    }
}

} // namespace lqr
} // namespace scpp

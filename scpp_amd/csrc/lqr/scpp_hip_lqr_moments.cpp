// The moments sweep of libscpp_lqr.so (lqr_moments_kernel.h), in a translation unit of its own: see lqr_sweep_launch.h.
#include "lqr_moments_kernel.h"
#include "lqr_sweep_launch.h"

namespace scpp
{
namespace lqr
{

bool launchMomentsSweep(int model_id, hipStream_t stream, int B, int K, int nU, int uRows, int steps, const double *X, const double *U, const double *T,
                        const double *par, int par_stride, const double *G, const int *gstatus, const double *S0, int s0_stride, const double *w,
                        const double *FF, const double *M0, int m0_stride, double *sd, double *icov, double *fcov, int *status, double *cov,
                        double *mean, double *dumean)
{
    return withLqrPlugin(model_id, [&](auto pl) {
        hipLaunchKernelGGL((lqr_moments_kernel<decltype(pl)>), dim3(unsigned(B)), dim3(WAVE), 0, stream, K, nU, uRows, steps, X, U, T, par, par_stride, G,
                           gstatus, S0, s0_stride, w, FF, M0, m0_stride, sd, icov, fcov, status, cov, mean, dumean);
    });
}

} // namespace lqr
} // namespace scpp

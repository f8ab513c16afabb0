// The moments sweep of libscpp_lqr.so (lqr_moments_kernel.h), in a translation unit of its own: see lqr_moments_launch.h.
#include "lqr_moments_kernel.h"
#include "lqr_moments_launch.h"

namespace scpp
{
namespace lqr
{

template <class PL, class... Args>
static bool launchMomentsFor(hipStream_t stream, int B, Args... args)
{
    hipLaunchKernelGGL((lqr_moments_kernel<PL>), dim3(unsigned(B)), dim3(WAVE), 0, stream, args...);
    return true;
}
template <class... PL, class... Args>
static bool launchMomentsOf(LqrPluginList<PL...>, int model_id, hipStream_t stream, int B, Args... args)
{
    return ((model_id == PL::ID ? launchMomentsFor<PL>(stream, B, args...) : false) || ...);
}

bool launchMomentsSweep(int model_id, hipStream_t stream, int B, int K, int nU, int uRows, int steps, const double *X, const double *U, const double *T,
                        const double *par, int par_stride, const double *G, const int *gstatus, const double *S0, int s0_stride, const double *w,
                        const double *FF, const double *M0, int m0_stride, double *sd, double *icov, double *fcov, int *status, double *cov,
                        double *mean, double *dumean)
{
    return launchMomentsOf(LqrPlugins{}, model_id, stream, B, K, nU, uRows, steps, X, U, T, par, par_stride, G, gstatus, S0, s0_stride, w, FF, M0,
                           m0_stride, sd, icov, fcov, status, cov, mean, dumean);
}

} // namespace lqr
} // namespace scpp

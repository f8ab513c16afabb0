// The affine finite-horizon sweep of libscpp_lqr.so (lqr_affine_kernel.h), in a translation unit of its own: see lqr_affine_launch.h.
#include "lqr_affine_kernel.h"
#include "lqr_affine_launch.h"

namespace scpp
{
namespace lqr
{

template <class PL, class... Args>
static bool launchAffineFor(hipStream_t stream, int B, Args... args)
{
    hipLaunchKernelGGL((lqr_affine_kernel<PL>), dim3(unsigned(B)), dim3(WAVE), 0, stream, args...);
    return true;
}
template <class... PL, class... Args>
static bool launchAffineOf(LqrPluginList<PL...>, int model_id, hipStream_t stream, int B, Args... args)
{
    return ((model_id == PL::ID ? launchAffineFor<PL>(stream, B, args...) : false) || ...);
}

bool launchAffineSweep(int model_id, hipStream_t stream, int B, int K, int nU, int uRows, int steps, const double *X, const double *U, const double *T,
                       const double *par, int par_stride, const double *qw, const double *rw, const double *qfw, double *G, int *status, int *iters,
                       double *FF, double *Pout, double *pout, double *sout)
{
    return launchAffineOf(LqrPlugins{}, model_id, stream, B, K, nU, uRows, steps, X, U, T, par, par_stride, qw, rw, qfw, G, status, iters, FF, Pout, pout,
                          sout);
}

} // namespace lqr
} // namespace scpp

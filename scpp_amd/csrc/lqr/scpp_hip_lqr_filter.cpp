// The filter sweep of libscpp_lqr.so (lqr_filter_kernel.h), in a translation unit of its own: see lqr_sweep_launch.h.
#include "lqr_filter_kernel.h"
#include "lqr_sweep_launch.h"

namespace scpp
{
namespace lqr
{

bool launchFilterSweep(int model_id, hipStream_t stream, bool loop, int B, int K, int nU, int uRows, int steps, const double *X, const double *U,
                       const double *T, const double *par, int par_stride, const double *G, const int *gstatus, const double *S0, int s0_stride,
                       const double *w, const double *H, const double *v, int ny, double *L, double *esd, double *fecov, int *status, double *ecov,
                       double *ssd, double *icov, double *fscov, double *xcov)
{
    return withLqrPlugin(model_id, [&](auto pl) {
        using P = decltype(pl);
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(unsigned(B)), dim3(WAVE), 0, stream, K, nU, uRows, steps, X, U, T, par, par_stride, G, gstatus, S0,
                               s0_stride, w, H, v, ny, L, esd, fecov, status, ecov, ssd, icov, fscov, xcov);
        };
        if (loop)
            go(lqr_filter_kernel<P, true>);
        else
            go(lqr_filter_kernel<P, false>);
    });
}

} // namespace lqr
} // namespace scpp

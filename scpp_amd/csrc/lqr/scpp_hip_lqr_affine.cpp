// The affine finite-horizon sweep of libscpp_lqr.so (lqr_affine_kernel.h), in a translation unit of its own: see lqr_sweep_launch.h.
#include "lqr_affine_kernel.h"
#include "lqr_sweep_launch.h"

namespace scpp
{
namespace lqr
{

bool launchAffineSweep(int model_id, hipStream_t stream, int B, int K, int nU, int uRows, int steps, const double *X, const double *U, const double *T,
                       const double *par, int par_stride, const double *qw, const double *rw, const double *qfw, double *G, int *status, int *iters,
                       double *FF, double *Pout, double *pout, double *sout)
{
    return withLqrPlugin(model_id, [&](auto pl) {
        hipLaunchKernelGGL((lqr_affine_kernel<decltype(pl)>), dim3(unsigned(B)), dim3(WAVE), 0, stream, K, nU, uRows, steps, X, U, T, par, par_stride, qw,
                           rw, qfw, G, status, iters, FF, Pout, pout, sout);
    });
}

} // namespace lqr
} // namespace scpp

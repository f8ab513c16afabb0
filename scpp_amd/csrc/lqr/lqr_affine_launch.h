// The affine sweep's launch (scpp_hip_lqr_affine.cpp): lqr_affine_kernel.h is compiled in a translation unit of its own, so that the kernels of
// scpp_hip_lqr.cpp are compiled exactly as they are without it (the inliner weighs a function by the number of its callers in the unit).
#pragma once
#include "lqr_kernels.h"

namespace scpp
{
namespace lqr
{

// enqueues lqr_affine_kernel<Plugin of model_id> with B blocks on `stream`; false for a model nobody registered.  Arguments: lqr_affine_kernel.h.
bool launchAffineSweep(int model_id, hipStream_t stream, int B, int K, int nU, int uRows, int steps, const double *X, const double *U, const double *T,
                       const double *par, int par_stride, const double *qw, const double *rw, const double *qfw, double *G, int *status, int *iters,
                       double *FF, double *Pout, double *pout, double *sout);

} // namespace lqr
} // namespace scpp

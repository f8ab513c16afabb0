// The moments sweep's launch (scpp_hip_lqr_moments.cpp): lqr_moments_kernel.h is compiled in a translation unit of its own, so that the kernels of
// scpp_hip_lqr.cpp are compiled exactly as they are without it (lqr_affine_launch.h has the reason).
#pragma once
#include "lqr_kernels.h"

namespace scpp
{
namespace lqr
{

// enqueues lqr_moments_kernel<Plugin of model_id> with B blocks on `stream`; false for a model nobody registered.  Arguments: lqr_moments_kernel.h.
bool launchMomentsSweep(int model_id, hipStream_t stream, int B, int K, int nU, int uRows, int steps, const double *X, const double *U, const double *T,
                        const double *par, int par_stride, const double *G, const int *gstatus, const double *S0, int s0_stride, const double *w,
                        const double *FF, const double *M0, int m0_stride, double *sd, double *icov, double *fcov, int *status, double *cov,
                        double *mean, double *dumean);

} // namespace lqr
} // namespace scpp

// The launches of the affine sweep (scpp_hip_lqr_affine.cpp) and of the moments sweep (scpp_hip_lqr_moments.cpp).  Each of the two kernels is
// compiled in a translation unit of its own, so that the kernels of scpp_hip_lqr.cpp are compiled exactly as they are without it: the inliner
// weighs a function (the model's flow map, its Jacobian rows) by the number of its callers in the unit.
#pragma once
#include "lqr_kernels.h"

namespace scpp
{
namespace lqr
{

// enqueues lqr_affine_kernel<Plugin of model_id> with B blocks on `stream`; false for a model nobody registered.  Arguments: riccatiSweep.
bool launchAffineSweep(int model_id, hipStream_t stream, int B, int K, int nU, int uRows, int steps, const double *X, const double *U, const double *T,
                       const double *par, int par_stride, const double *qw, const double *rw, const double *qfw, double *G, int *status, int *iters,
                       double *FF, double *Pout, double *pout, double *sout);

// enqueues lqr_moments_kernel<Plugin of model_id> with B blocks on `stream`; false for a model nobody registered.  Arguments: covarianceSweep.
bool launchMomentsSweep(int model_id, hipStream_t stream, int B, int K, int nU, int uRows, int steps, const double *X, const double *U, const double *T,
                        const double *par, int par_stride, const double *G, const int *gstatus, const double *S0, int s0_stride, const double *w,
                        const double *FF, const double *M0, int m0_stride, double *sd, double *icov, double *fcov, int *status, double *cov,
                        double *mean, double *dumean);

} // namespace lqr
} // namespace scpp

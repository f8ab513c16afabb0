// The launches of the affine sweep (scpp_hip_lqr_affine.cpp), of the moments sweep (scpp_hip_lqr_moments.cpp) and of the filter sweep
// (scpp_hip_lqr_filter.cpp).  Each of these kernels is
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

// enqueues lqr_filter_kernel<Plugin of model_id, loop> (scpp_hip_lqr_filter.cpp) with B blocks on `stream`; false for a model nobody registered.
// Arguments: lqr_filter_kernel; without `loop`, G, gstatus, ssd, icov, fscov and xcov are neither read nor written.
bool launchFilterSweep(int model_id, hipStream_t stream, bool loop, int B, int K, int nU, int uRows, int steps, const double *X, const double *U,
                       const double *T, const double *par, int par_stride, const double *G, const int *gstatus, const double *S0, int s0_stride,
                       const double *w, const double *H, const double *v, int ny, double *L, double *esd, double *fecov, int *status, double *ecov,
                       double *ssd, double *icov, double *fscov, double *xcov);

} // namespace lqr
} // namespace scpp

// Closed-loop mean next to the covariance: the covariance sweep of lqr_covariance_kernel.h on the state z = [e; 1] (include/scpp_hip_lqr.h,
// scpp_hip_lqr_propagate_moments).
//
//   dS/dt = A_cl S + S A_cl' + W      S(0) = S0        A_cl = A - B K_t
//   dm/dt = A_cl m + d(t)             m(0) = mean0     d = c - [B k_t],   c = f(x_ref, u_ref) - dx_ref/dt
//   mean correction of node k: du_mean[k] = -G[k] m(t_k) - [ff[k]]
//
// The tile is T = [[S, m], [m', 0]] (nx + 1 <= 15) in the accumulator layout.  closedLoopJacobian and covarianceRhs are the covariance kernel's,
// unchanged: row and column NX of the LDS A_cl tile stay zero, so A_cl T + T A_cl' is [[A_cl S + S A_cl', A_cl m], [(A_cl m)', 0]] and the S block
// sees the covariance kernel's products plus 0 m' and m 0: S, and everything recorded from it, is that of the covariance sweep.  d enters OUTSIDE
// the products: the lanes that hold column NX (rows < NX) and row NX (columns < NX) add it to their slope, both from the same LDS value, so the
// tile stays symmetric to the bit by the covariance kernel's argument; m is downloaded from column NX.  S + m m' is never formed.
// Mapping: lane r < nx evaluates Jacobian row r inside closedLoopJacobian as in the covariance kernel and, with feedforward terms, once more for
// -B_r k_t (closedLoopJacobian does not hand its row out); lane nx, idle there, evaluates the flow map at the same point and writes c.
// The body is covarianceSweep<P, true> of lqr_covariance_kernel.h; this header is the entry point.
#pragma once
#include "lqr_covariance_kernel.h"

namespace scpp
{
namespace lqr
{

// arguments: covarianceSweep
template <class P>
__global__ void __launch_bounds__(WAVE) lqr_moments_kernel(int K, int nU, int uRows, int steps, const double *__restrict__ X, const double *__restrict__ U,
                                                            const double *__restrict__ T, const double *__restrict__ par, int par_stride,
                                                            const double *__restrict__ G, const int *__restrict__ gstatus,
                                                            const double *__restrict__ S0, int s0_stride, const double *__restrict__ w,
                                                            const double *__restrict__ FF, const double *__restrict__ M0, int m0_stride,
                                                            double *__restrict__ sd, double *__restrict__ icov, double *__restrict__ fcov,
                                                            int *__restrict__ status, double *__restrict__ cov, double *__restrict__ mean,
                                                            double *__restrict__ dumean)
{
    __shared__ MomentsLds lds;
    covarianceSweep<P, true>(lds, K, nU, uRows, steps, X, U, T, par, par_stride, G, gstatus, S0, s0_stride, w, FF, M0, m0_stride, sd, icov, fcov,
                             status, cov, mean, dumean);
}

} // namespace lqr
} // namespace scpp

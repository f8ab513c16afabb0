// Affine finite-horizon LQR: the Riccati sweep of lqr_riccati_kernel.h on the deviation of a nominal that does NOT obey the dynamics
// (include/scpp_hip_lqr.h, scpp_hip_lqr_compute_gains_affine).
//
//   de/dt = A e + B du + c(t),   c = f(x_ref, u_ref) - dx_ref/dt,   V = e'P e + 2 p'e + s
//   -dP/dt = A'P + P A - P B R^-1 B'P + Q            P(T) = Qf
//   -dp/dt = (A - B R^-1 B'P)'p + P c                p(T) = 0
//   -ds/dt = 2 p'c - p'B R^-1 B'p                    s(T) = 0
//   du = -K e - k,   K_k = R^-1 B_k'P(t_k),   k_k = R^-1 B_k'p(t_k)
//
// It is the Riccati equation of the augmented state z = [e; 1]:  A_aug = [[A, c], [0, 0]],  B_aug = [B; 0],  Q_aug = diag(Q, 0),
// P_aug = [[P, p], [p', s]].  nx + 1 <= 15, so P_aug is the ONE 16 x 16 tile of the Riccati kernel, and riccatiRhs is used unchanged: column NX
// of the LDS Jacobian tile carries c, row NX stays zero.  The P block sees the same products as in the Riccati kernel plus p 0 and 0 p, so P and K
// are those of the Riccati sweep; P_aug is symmetric to the bit by the Riccati kernel's argument.
// Mapping: lane r < nx evaluates Jacobian row r as in the Riccati kernel; lane nx, idle there, evaluates the flow map at the same point and writes
// column nx.  The two branches run one after the other in the wave (DESIGN.md 5.2 has what that costs).
// The body is riccatiSweep<P, true> of lqr_riccati_kernel.h; this header is the entry point.
#pragma once
#include "lqr_riccati_kernel.h"

namespace scpp
{
namespace lqr
{

// arguments: riccatiSweep
template <class P>
__global__ void __launch_bounds__(WAVE) lqr_affine_kernel(int K, int nU, int uRows, int steps, const double *__restrict__ X, const double *__restrict__ U,
                                                           const double *__restrict__ T, const double *__restrict__ par, int par_stride,
                                                           const double *__restrict__ qw, const double *__restrict__ rw, const double *__restrict__ qfw,
                                                           double *__restrict__ G, int *__restrict__ status, int *__restrict__ iters,
                                                           double *__restrict__ FF, double *__restrict__ Pout, double *__restrict__ pout,
                                                           double *__restrict__ sout)
{
    __shared__ RiccatiLds lds;
    riccatiSweep<P, true>(lds, K, nU, uRows, steps, X, U, T, par, par_stride, qw, rw, qfw, G, status, iters, FF, Pout, pout, sout);
}

} // namespace lqr
} // namespace scpp

/* scpp_hip_lqr.h -- C ABI of the batched LQR trajectory tracker (libscpp_lqr.so; gfx950).
 *
 * A component of its own next to scpp_hip.h: it uses the solver only through what the solver hands out (trajectories in SI units as
 * scpp_hip_download / scpp_hip_stream_download return them, or the device pointers of scpp_hip_device_ptrs) and shares no state with it.
 *
 * What each entry point replaces in the reference:
 *   LQRTracker::LQRTracker                scpp_core/src/LQRTracker.cpp:6-28       scpp_hip_lqr_compute_gains
 *       ComputeLQR / careSolve / solveSchurIterative   scpp_core/src/LQR.cpp:7-109
 *   LQRTracker::loadParameters            scpp_core/src/LQRTracker.cpp:30-41      scpp_hip_lqr_set_weights (the caller reads LQR.info)
 *   LQRTracker::getInput, interpolateGains  LQRTracker.cpp:43-65, trajectoryData.hpp:41-78
 *   the closed loop of SC_tracking        scpp/src/SC_tracking.cpp:48-75          scpp_hip_lqr_track
 *       scpp::simulate (RKF78, fixed steps)   scpp_core/src/simulation.cpp:25-42
 *   LQRAlgorithm::initialize / solve, the loop of LQR_sim   LQRAlgorithm.cpp:11-33, LQR_sim.cpp:43-82   the same, see scpp_hip_lqr_set_stop_tolerance
 *       LQR_sim's input clipping (LQR_sim.cpp:55-66)                                          scpp_hip_lqr_set_input_limits: the same three
 *       steps in the same order for the models whose input is a thrust vector; the reference's code addresses u.z() of the two-input
 *       Rocket2D, the only model it builds LQR_sim for, and does not compile: Rocket2D gets the box of rocket2d.cpp:77-83 instead
 *   nothing: the reference flies one start per trajectory                                     scpp_hip_lqr_track_samples
 *   nothing: the reference has no finite-horizon controller                                   scpp_hip_lqr_set_terminal_weights,
 *       (the differential Riccati equation along the trajectory)               scpp_hip_lqr_compute_gains_riccati, _download_riccati
 *   nothing: the reference has no covariance analysis                                         scpp_hip_lqr_set_covariance_inputs,
 *       (the closed-loop Lyapunov equation along the trajectory)               scpp_hip_lqr_propagate_covariance, _download_covariance
 *       (the covariance recursion of the loop that holds its correction)       scpp_hip_lqr_propagate_covariance_discrete
 *   nothing: the reference has no sampled-data controller                                     scpp_hip_lqr_compute_gains_discrete, _download_discrete,
 *       (the discrete Riccati recursion over the segments' transition matrices) scpp_hip_lqr_set_feedback_hold
 *   nothing: the reference has no feedforward for a nominal that misses its nodes             scpp_hip_lqr_compute_gains_affine, _download_affine,
 *       (the Riccati sweep on the state [e; 1])                                scpp_hip_lqr_set_feedforward_terms, _set_feedforward
 *   nothing: the reference does not predict where its loop's centre goes                      scpp_hip_lqr_propagate_moments, _download_moments
 *       (the covariance sweep on the state [e; 1])
 *   nothing: the reference's controller reads the true state                                  scpp_hip_lqr_set_measurement, scpp_hip_lqr_filter,
 *       (the Kalman-Bucy filter and the output-feedback loop's covariance)     scpp_hip_lqr_download_filter
 *   nothing: the reference's plant is never disturbed                                         scpp_hip_lqr_set_disturbance, _disturbance_normals
 *       (process noise in the loop)
 *
 * Deviations, all deliberate:
 *   - RocketQuat gains are computed on the tangent system of the unit-quaternion constraint (13 states): the reference's 28 x 28 Hamiltonian
 *     is exactly singular wherever w_B = 0.
 *   - zero-order hold: node k linearises at U[min(k, K-2)]; the reference special-cases k == K-2 and reads U.at(K-1) out of range at k = K-1.
 *   - the node index is clamped to K-2 where t / dt rounds up to K-1 just below the flight time (the reference reads X.at(K)).
 *   - a loop whose state or input goes non-finite (a non-finite reference node included) retires with status -2 and keeps its last
 *     finite state and input (the reference throws); the errors are norms in double (the reference
 *     truncates them to size_t).
 *   - the record keeps every write_steps-th step.
 *   - scpp_hip_lqr_compute_gains_riccati is an addition, not a replacement: -dP/dt = A'P + PA - P B R^-1 B'P + Q, P(T) = Qf, integrated
 *     backwards segment by segment with fixed-step RKF78 (the tableau and solution weights of the plant step), on the full state of every model
 *     (RocketQuat: 14 states, no tangent projection: the finite-horizon equation needs no stabilisability).  P is kept symmetric BY CONSTRUCTION
 *     (P A and A'P are both formed, from the same products in the same order, and the quadratic term as S S' with S = P B R^-1/2); it is never
 *     symmetrised.  Inside segment i the reference is x = X[i] + a (X[i+1] - X[i]), u = U[i] + a (U[j] - U[i]), j = i+1 (first-order hold) or i
 *     (zero-order hold), a in [0, 1]; the segment index is that of the segment being integrated and is never recomputed from the time.
 *   - scpp_hip_lqr_propagate_covariance is an addition as well: linear covariance analysis of the closed loop,
 *     dS/dt = A_cl(t) S + S A_cl(t)' + W, S(0) = S0, A_cl(t) = A(t) - B(t) K(t), W = diag(w) a constant disturbance intensity, w >= 0 (default 0),
 *     S0 a full symmetric matrix.  For one trajectory of K nodes and flight time T, dt = T / (K - 1); the sweep runs segment by segment from
 *     segment 0 up to K-2.  Inside segment i at fraction a in [0, 1]: x = X[i] + a (X[i+1] - X[i]), u = U[i] + a (U[j] - U[i]),
 *     K_t = G[i] + a (G[j] - G[i]), j = i+1 (first-order hold) or i (zero-order hold): exactly the interpolation the tracking kernel applies to
 *     state, input and gain.  The segment index is the loop's and is never recomputed from the time.  A, B are the generated Jacobian rows at
 *     (x, u), on the full state of every model (RocketQuat: 14 states).  G is whatever gains the context holds: frozen-time, Riccati or
 *     scpp_hip_lqr_set_gains.  The integrator is fixed-step RKF78 with the plant step's tableau and 8th-order weights, steps >= 1 steps per
 *     segment; stage s of step n sits at a = (n + c_s) / steps.  Node k records S(t_k) and the input covariance G[k] S(t_k) G[k]' with the
 *     node's own gain; node 0 records S0 exactly.  S is kept symmetric BY CONSTRUCTION (A_cl S and S A_cl' are both formed, from the same
 *     products in the same order); it is never symmetrised, which is why S0 has to be symmetric to the bit.
 *   - scpp_hip_lqr_compute_gains_discrete is an addition too: the gains of a loop that updates its correction only at the nodes and holds it
 *     over a segment (scpp_hip_lqr_set_feedback_hold flies such a loop).  For one trajectory of K nodes and flight time T, dt = T / (K - 1).
 *     Inside segment i at fraction a in [0, 1] the reference is x = X[i] + a (X[i+1] - X[i]), u = U[i] + a (U[j] - U[i]), j = i+1 (first-order
 *     hold) or i (zero-order hold); the segment index is the loop's and is never recomputed from the time.  A correction du_i is added to the
 *     reference input and held constant over segment i, under either hold of the reference.  The deviation then obeys
 *     dx_{i+1} = Phi_i dx_i + Gamma_i du_i with d[Phi | Gamma]/dt = A(t) [Phi | Gamma] + [0 | B(t)], [Phi | Gamma](t_i) = [I | 0]; A, B are the
 *     generated Jacobian rows at (x, u) on the full state of every model (RocketQuat: 14 states, no tangent system).  The equation is integrated
 *     forwards over the segment with steps >= 1 fixed RKF78 steps (the plant step's tableau and 8th-order weights); stage s of step n sits at
 *     a = (n + c_s) / steps.  The recursion runs backwards, i = K-2 .. 0, from P_{K-1} = Qf, with the stage weights Q dt and R dt (one LQR.info
 *     means the same under this law and under the Riccati-ODE law, which the recursion tends to as dt -> 0):
 *         S_i = R dt + Gamma_i'P_{i+1} Gamma_i,   N_i = Gamma_i'P_{i+1} Phi_i,   L_i L_i' = S_i (Cholesky, lower),   Y_i = L_i^-1 N_i,
 *         K_i = L_i^-T Y_i,                       P_i = Q dt + Phi_i'P_{i+1} Phi_i - Y_i'Y_i.
 *     Node K-1 has no segment behind it: its gain is a copy of K_{K-2} and its P is Qf.  P is symmetric TO THE BIT at every node: Y'Y is by
 *     construction, and Phi'(P Phi) is symmetrised once per node, (F + F') / 2.  scpp_hip_lqr_propagate_covariance does NOT know this law's
 *     hold: it describes the continuous loop u = u_ref - K_t (x - x_ref), whatever gains it is given.  The covariance of the held loop is
 *     scpp_hip_lqr_propagate_covariance_discrete:
 *   - scpp_hip_lqr_propagate_covariance_discrete is an addition: linear covariance analysis of the loop du_i = -G[i] dx(t_i), held over
 *     segment i (the loop of scpp_hip_lqr_set_feedback_hold(1)).  Taken unchanged from the discrete gain sweep: the reference inside segment i,
 *     x = X[i] + a (X[i+1] - X[i]), u = U[i] + a (U[j] - U[i]), j = i+1 (first-order hold) or i (zero-order hold); the segment index, the
 *     loop's and never recomputed from a time; RKF78 with the plant step's tableau and 8th-order weights, steps >= 1 steps per segment, stage
 *     s of step n at a = (n + c_s) / steps; A and B, the generated Jacobian rows on the full state of every model (RocketQuat: 14 states).
 *     G is whatever gains the context holds: discrete, Riccati, frozen or scpp_hip_lqr_set_gains.  A disturbance of constant intensity
 *     W = diag(w) acts during the segment:
 *         d[Phi | Gamma]/dt = A(t) [Phi | Gamma] + [0 | B(t)],   [Phi | Gamma](t_i) = [I | 0]     (the discrete gain sweep's own equation)
 *         dM/dt = A(t) M + M A(t)' + W,   M(t_i) = 0,   Wd_i = M(t_{i+1})     (what the segment accumulates; A is the open-loop Jacobian,
 *                                                                              because the held input does not react inside a segment)
 *         Acl_i = Phi_i - Gamma_i G[i],   S_{i+1} = Acl_i S_i Acl_i' + Wd_i,   S_0 = sigma0.
 *     Node k records S_k, sqrt(diag S_k) and the input covariance G[k] S_k G[k]': for k <= K-2 the covariance of the correction actually held
 *     over segment k; node K-1 reports it with the node's own gain, for uniformity with the continuous sweep.  Node 0 records sigma0 exactly.
 *     S is symmetric TO THE BIT at every node: M is by construction (A M and M A' are both formed, from the same products in the same
 *     order), Acl (S Acl') is symmetrised once per node, (F + F') / 2, as the discrete gain sweep treats Phi'(P Phi), and sigma0 has to be
 *     symmetric to the bit, as for the continuous sweep.  With w NULL or all zero the M integration is skipped as a whole; the result is
 *     bitwise that of Wd = 0.
 *
 *   - scpp_hip_lqr_compute_gains_affine is an addition: the finite-horizon law for a nominal that does not obey the dynamics.  One trajectory
 *     has K nodes and flight time T, dt = T / (K - 1).  Inside segment i at fraction a in [0, 1] the reference is exactly the Riccati sweep's:
 *     x = X[i] + a (X[i+1] - X[i]), u = U[i] + a (U[j] - U[i]), j = i+1 (first-order hold) or i (zero-order hold); the segment index is the
 *     loop's and is never recomputed from a time.  The defect of the reference is c = f(x, u) - (X[i+1] - X[i]) / dt, f the plant's flow map
 *     (SI parameters) on the full state of every model (RocketQuat: 14 states).  Along such a nominal the deviation of the loop
 *     u = u_ref + du obeys de/dt = A e + B du + c(t).  The cost is that of the finite-horizon law, int e'Qe + du'R du dt + e(T)'Qf e(T); the value
 *     function is V = e'P e + 2 p'e + s with
 *         -dP/dt = A'P + P A - P B R^-1 B'P + Q          P(T) = Qf     (the Riccati sweep's own equation)
 *         -dp/dt = (A - B R^-1 B'P)'p + P c               p(T) = 0
 *         -ds/dt = 2 p'c - p'B R^-1 B'p                   s(T) = 0
 *         du = -K e - k,   K_k = R^-1 B_k'P(t_k),   k_k = R^-1 B_k'p(t_k)      (B_k at (X[k], U[min(k, nU-1)]), as for the gains)
 *     s(t_k) is the predicted cost-to-go of a flight that is exactly on the nominal at node k.  The three equations are ONE Riccati equation,
 *     that of the state [e; 1] with A_aug = [[A, c], [0, 0]], B_aug = [B; 0], Q_aug = diag(Q, 0), Qf_aug = diag(Qf, 0) and
 *     P_aug = [[P, p], [p', s]], and are integrated as such: the integrator, the stage positions and the construction that keeps the matrix
 *     symmetric to the bit are those of scpp_hip_lqr_compute_gains_riccati.  P and K are those of that sweep at the same step count (the
 *     augmentation adds products with exact zeros to them).  scpp_hip_lqr_set_feedforward(1) flies u_cmd = u_ref(t) - K_t (x - x_ref(t)) - k_t,
 *     k_t interpolated with the indices and the fraction of the gain.  The loop that holds its correction over a segment
 *     (scpp_hip_lqr_set_feedback_hold(1)) has no such term here: its optimal offset is an affine DISCRETE recursion, which is not built, and the
 *     two together are refused.  The covariance sweeps describe the dispersion about the mean, which does not depend on c: they are valid under
 *     either setting; they do not propagate the mean itself, scpp_hip_lqr_propagate_moments does:
 *   - scpp_hip_lqr_propagate_moments is an addition: the mean deviation of the continuous loop next to its covariance.  Everything about the
 *     reference inside segment i is that of scpp_hip_lqr_propagate_covariance: x, u and K_t interpolated with a and the loop's segment index,
 *     RKF78 with the plant step's tableau, steps >= 1 steps per segment, stage s of step n at a = (n + c_s) / steps, generated Jacobian rows
 *     on the full state.  With the loop u = u_ref - K_t e - [k_t]:
 *         dS/dt = A_cl S + S A_cl' + W          S(0) = sigma0     (the covariance sweep's own equation)
 *         dm/dt = A_cl m + d(t)                 m(0) = mean0      A_cl = A - B K_t
 *         d(t)  = c(t) - [B(t) k_t]             c = f(x, u) - (X[i+1] - X[i]) / dt     (the defect of the affine sweep)
 *     k_t = ff[i] + a (ff[j] - ff[i]) with the gain's indices and fraction.  feedforward == 1 takes k_t from the feedforward terms the context
 *     holds, computed or supplied; feedforward == 0 means d = c.  Order of the sum: c_r = f_r - xdot_r; bk_r = ((0 - B_r0 k_0) - B_r1 k_1) - ...
 *     over the inputs in order, each step one fused multiply-add; d_r = c_r + bk_r (bk_r = 0 without the term).  The two equations are ONE
 *     Lyapunov equation, that of z = [e; 1] with the tile [[S, m], [m', 0]] (nx + 1 <= 15); A_cl enters the products with a zero row and column
 *     nx, and d is added to the slope of m outside them, so S and everything recorded from it are those of scpp_hip_lqr_propagate_covariance at
 *     the same step count (the augmentation adds products with exact zeros), and S + m m' is never formed.  Node k records m(t_k) and
 *     du_mean[k] = -G[k] m(t_k) - [ff[k]], the mean correction on top of u_ref; node 0 records mean0 exactly.  It is a linearisation about the
 *     nominal, it describes the continuous loop only (the mean of the loop that holds its correction belongs with the affine discrete
 *     recursion, which is not built), and it knows no input limits.
 *   - input limits (scpp_hip_lqr_set_input_limits) are an addition to the tracking loop, off by default: with limits (T_min, T_max, angle_max)
 *     the loop applies u = sat(u_cmd), u_cmd = -K_t (x - x_ref) + u_ref computed as without them.  A non-finite u_cmd retires the flight with
 *     status -2 before sat.  Thrust-vector models (RocketQuat: u = (T_B, tau_z), sat acts on u[0..2] and u[3] passes through; Lander3dof:
 *     u = T_I), in this order:  1. u_z = max(T_min, u_z);  2. c = tan(angle_max) u_z, and if |u_xy| > c then u_xy *= c / |u_xy|;
 *     3. if |u| > T_max then u *= T_max / |u|.  With T_min <= T_max cos(angle_max), which the host demands, the result lies in the input set of
 *     the models' constraint tables (u_z >= T_min, |u_xy| <= tan(angle_max) u_z, |u| <= T_max); without it step 3 could undo step 1.
 *     Rocket2D (u = (gimbal, thrust)): gimbal clamped to [-angle_max, angle_max], thrust to [T_min, T_max].  A point inside the set is returned
 *     bitwise.  It is a clip: the gains do not know about it and there is no anti-windup.  Per flight: n_sat = the plant steps on which
 *     u != u_cmd in any component, max_clip = the largest |u_cmd - u|_2 met; out_u and the record hold the applied input u.
 *   - process noise (scpp_hip_lqr_set_disturbance) is an addition to the tracking loop, off by default: the disturbed plant.  With a
 *     disturbance set, plant step n of flight f integrates dx/dt = f(x, u) + d; n is the loop's own 0-based step counter and the step takes
 *     t_n to t_n + time_step.  d_r = sqrt(w_r / time_step) z_r is constant over the plant step and is added to the slope of every RKF78 stage
 *     of every substep; w_r is the intensity, in state^2 per second, that scpp_hip_lqr_set_covariance_inputs takes, z_r are independent
 *     standard normals, and w_r == 0 gives d_r = 0.  This is the piecewise-constant realisation of white noise of intensity W = diag(w): one
 *     step accumulates W time_step to first order.  z is a pure function of (seed, flight index, n, r) and there is no generator state:
 *     Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85) with the counter (n, j, g lo32, g hi32),
 *     j = r / 2 the pair index and g = flight_offset + f the global flight index, and the key (seed lo32, seed hi32).  From the output words
 *     c0..c3: m1 = (uint64(c0) << 20) | (c1 >> 12), m2 likewise from c2, c3; u = (double(m) + 0.5) 2^-52, exact and strictly inside (0, 1);
 *     rho = sqrt(-2 ln u1), z[2j] = rho cos(2 pi u2), z[2j+1] = rho sin(2 pi u2); an odd nx drops the last z.  The draw happens after u has
 *     been decided (sat included) and before the plant step; a retired flight draws nothing more.  The record, max_dev, limits, feedback
 *     hold, feedforward, the stop tolerance, sample fans and the non-finite retirement behave as without it, in every combination of limits,
 *     hold and feedforward that exists without it.  Limitations: the noise is white, diagonal and held over a plant step; there is no
 *     measurement noise, no coloured noise, and the gains know nothing of it.
 *   - scpp_hip_lqr_track_samples flies `samples` starts per trajectory: flight f of F = B samples follows trajectory f / samples (its X, U, t,
 *     gains, parameter row and limits row) from x_start[f]; trajectories and gains are neither copied nor recomputed.
 *
 * Conventions as in scpp_hip.h: every function returns 0 or a negative SCPP_E_* code, nothing throws; host buffers are caller-owned, float64
 * (int32 where said), C-contiguous; one host thread per context.  All work goes on the context's own stream; nothing synchronises the device.
 */
#ifndef SCPP_HIP_LQR_H
#define SCPP_HIP_LQR_H

#ifdef __cplusplus
extern "C"
{
#endif

#ifndef SCPP_OK
#define SCPP_OK 0
#define SCPP_E_ARG -1
#define SCPP_E_HIP -2
#define SCPP_E_UNSUPPORTED -3
#define SCPP_E_STATE -4
#endif

/* per-node gain status and per-instance tracking status */
#define SCPP_LQR_OK 0
#define SCPP_LQR_STEP_CAP 1         /* tracking: stopped by max_steps before the flight time */
#define SCPP_LQR_GAINS_INCOMPLETE 2 /* covariance, informational: some node of the trajectory has a gain status != 0, i.e. a zero gain; the sweep ran on it */
#define SCPP_LQR_ITERATION_LIMIT -1 /* gains: 101 sign iterations without convergence (LQR.cpp:19-20) */
#define SCPP_LQR_NONFINITE -2       /* gains: singular or non-finite Hamiltonian; tracking: non-finite state */

    typedef struct scpp_hip_lqr_ctx scpp_hip_lqr_ctx;

    const char *scpp_hip_lqr_version(void);
    /* model_id as in scpp_hip.h (0 RocketQuat, 1 Rocket2D, 2 Lander3dof); K >= 2 nodes; foh != 0: U [B][K][nu], else U [B][K-1][nu].
       Weights start as Q = I, R = I.  SCPP_E_ARG for an unknown model, K < 2, batch_max < 1. */
    int scpp_hip_lqr_create(scpp_hip_lqr_ctx **ctx, int device_id, int model_id, int K, int batch_max, int foh);
    int scpp_hip_lqr_destroy(scpp_hip_lqr_ctx *ctx);
    int scpp_hip_lqr_dims(scpp_hip_lqr_ctx *ctx, int *nx, int *nu, int *np, int *nr /* order of the Riccati equation */);
    /* diagonals of Q and R (LQR.info: state_weights, input_weights); every entry must be finite and > 0, else SCPP_E_ARG */
    int scpp_hip_lqr_set_weights(scpp_hip_lqr_ctx *ctx, const double *q /* [nx] */, const double *r /* [nu] */);
    /* flow-map parameters in SI units (flow_params(nondimensionalize=False)); B == 1 broadcasts one row to every instance, otherwise B must
       equal the number of trajectories: scpp_hip_lqr_compute_gains / _track return SCPP_E_STATE when it does not */
    int scpp_hip_lqr_set_flow_params(scpp_hip_lqr_ctx *ctx, const double *par /* [B][np] */, int B);
    /* trajectories in SI units: X [B][K][nx], U [B][K or K-1][nu], flight time t [B]; invalidates gains */
    int scpp_hip_lqr_set_trajectories(scpp_hip_lqr_ctx *ctx, const double *X, const double *U, const double *t, int B);
    /* the same from device memory: not copied, the caller keeps the buffers alive and orders its own stream before the next call here.
       u_rows is the row stride of dU per trajectory, dU [B][u_rows][nu] with u_rows >= the K or K-1 inputs of this context (SCPP_E_ARG
       otherwise).  scpp_hip_device_ptrs of a solved context hands out the redimensionalised result buffers X [B][K][nx], U [B][K][nu]
       (K rows whatever the hold: pass u_rows = K, a zero-order-hold tracker then skips the unused last row) and sigma [B]. */
    int scpp_hip_lqr_set_trajectories_device(scpp_hip_lqr_ctx *ctx, const void *dX, const void *dU, const void *dt, int B, int u_rows);
    /* one gain per (instance, node); *n_ok (optional) = nodes with status 0.  SCPP_E_STATE without trajectories or flow parameters. */
    int scpp_hip_lqr_compute_gains(scpp_hip_lqr_ctx *ctx, int *n_ok);
    /* diagonal of the terminal weight Qf of the finite-horizon gains; NULL: Qf = Q (the default).  Every entry finite and > 0, else SCPP_E_ARG. */
    int scpp_hip_lqr_set_terminal_weights(scpp_hip_lqr_ctx *ctx, const double *qf /* [nx] */);
    /* finite-horizon gains: one Riccati sweep per trajectory from P(T) = Qf, steps >= 1 RKF78 steps per segment (SCPP_E_ARG otherwise), one
       K_k = R^-1 B_k'P(t_k) per node with B_k at (X[k], U[min(k, nU-1)]), node K-1: R^-1 B'Qf; full [nu][nx] shape.  Gains, status and the
       count land where scpp_hip_lqr_download_gains reads them (the count: RKF78 steps behind the node, (K-1-k) steps) and scpp_hip_lqr_track
       flies them.  A trajectory with a non-finite node, input or flight time gets SCPP_LQR_NONFINITE and zero gains on every node; a P that
       turns non-finite in segment k does the same for node k and every earlier node.  keep_p != 0 also keeps P(t_k) for
       scpp_hip_lqr_download_riccati (the buffer, B K nx nx doubles, is allocated on the first such request).  *n_ok (optional) = nodes with
       status 0.  SCPP_E_STATE as scpp_hip_lqr_compute_gains. */
    int scpp_hip_lqr_compute_gains_riccati(scpp_hip_lqr_ctx *ctx, int steps, int keep_p, int *n_ok);
    /* P [B][K][nx][nx] of the last sweep (zeros on failed nodes); SCPP_E_STATE unless the last gain computation was a sweep with keep_p != 0 */
    int scpp_hip_lqr_download_riccati(scpp_hip_lqr_ctx *ctx, double *P);
    /* affine finite-horizon gains (the definition is above): one sweep of [[P, p], [p', s]] per trajectory from P(T) = Qf, p(T) = 0, s(T) = 0.
       Preconditions and SCPP_E_* answers are those of scpp_hip_lqr_compute_gains_riccati.  Gains, status and the count land where
       scpp_hip_lqr_download_gains reads them, the feedforward terms k_k where scpp_hip_lqr_download_affine does.  A trajectory with a
       non-finite node, input or flight time gets SCPP_LQR_NONFINITE and zeros on every node; a P, p or s that turns non-finite in segment k (a
       non-finite flow map at a finite reference point included) does the same for node k and every earlier node.  Nothing non-finite is ever
       written.  keep != 0 also keeps P, p and s of every node (allocated on the first such request).  *n_ok (optional) = nodes with status 0. */
    int scpp_hip_lqr_compute_gains_affine(scpp_hip_lqr_ctx *ctx, int steps, int keep, int *n_ok);
    /* ff [B][K][nu] = k_k, P [B][K][nx][nx], p [B][K][nx], s [B][K] of the last affine sweep (zeros on failed nodes); any pointer may be NULL.
       SCPP_E_STATE unless the last gain computation was scpp_hip_lqr_compute_gains_affine, and for P, p, s after a sweep with keep == 0. */
    int scpp_hip_lqr_download_affine(scpp_hip_lqr_ctx *ctx, double *ff /* [B][K][nu] */, double *P, double *p /* [B][K][nx] */, double *s /* [B][K] */);
    /* user-supplied feedforward terms [B][K][nu] for the gains the context holds (computed or scpp_hip_lqr_set_gains); non-finite entries are
       refused (SCPP_E_ARG); SCPP_E_STATE without gains.  Feedforward terms, computed or supplied, are invalidated by new trajectories, flow
       parameters, scpp_hip_lqr_set_gains and every scpp_hip_lqr_compute_gains* other than the affine one. */
    int scpp_hip_lqr_set_feedforward_terms(scpp_hip_lqr_ctx *ctx, const double *ff /* [B][K][nu] */);
    /* whether the tracking loop applies the feedforward term.  mode 0 (the default): the loop as it is without one.  mode 1:
       u_cmd = u_ref(t) - K_t (x - x_ref(t)) - k_t, k_t = ff[i] + a (ff[j] - ff[i]) with the indices and the fraction of the gain; flight f of a
       sample fan reads the row of trajectory f / samples; input limits, the record, the stop tolerance and the non-finite retirement act on this
       u_cmd.  Anything else: SCPP_E_ARG.  Under mode 1 scpp_hip_lqr_track / _track_samples return SCPP_E_STATE when the context holds no
       feedforward terms and SCPP_E_UNSUPPORTED when the feedback hold is 1.  The mode stays until it is set again. */
    int scpp_hip_lqr_set_feedforward(scpp_hip_lqr_ctx *ctx, int mode);
    /* sampled-data gains (the definition is above): one discrete Riccati recursion per trajectory from P_{K-1} = Qf
       (scpp_hip_lqr_set_terminal_weights; default Q), steps >= 1 RKF78 steps per segment for [Phi | Gamma] (SCPP_E_ARG otherwise).  Gains,
       status and the count land where scpp_hip_lqr_download_gains reads them (the count: RKF78 steps behind the node, (K-1-k) steps); node
       K-1 carries a copy of node K-2's gain.  A trajectory with a non-finite node, input or flight time gets SCPP_LQR_NONFINITE and zero gains
       on every node; a P, Phi, Gamma or pivot of S that turns non-finite or non-positive in segment k does the same for node k and every
       earlier node (segment K-2 takes node K-1 with it, whose gain it defines).  Nothing non-finite is ever written.  keep != 0 also keeps
       P of every node and Phi, Gamma of every segment for scpp_hip_lqr_download_discrete (the buffers are allocated on the first such
       request).  *n_ok (optional) = nodes with status 0.  SCPP_E_STATE as scpp_hip_lqr_compute_gains. */
    int scpp_hip_lqr_compute_gains_discrete(scpp_hip_lqr_ctx *ctx, int steps, int keep, int *n_ok);
    /* P [B][K][nx][nx], Phi [B][K-1][nx][nx], Gamma [B][K-1][nx][nu] of the last discrete sweep (zeros on failed nodes and their segments); any
       pointer may be NULL.  SCPP_E_STATE unless the last gain computation was scpp_hip_lqr_compute_gains_discrete with keep != 0. */
    int scpp_hip_lqr_download_discrete(scpp_hip_lqr_ctx *ctx, double *P, double *Phi, double *Gamma);
    /* when the tracking loop updates its feedback term.  mode 0 (the default): on every plant step, u_cmd = u_ref(t) - K_t (x - x_ref(t)).
       mode 1: held over a segment: du = -G[i] (x - x_ref(t)) is latched at the first plant step whose segment index i differs from the
       latched one (flight start counts as such a step), and u_cmd = u_ref(t) + du on every plant step, u_ref interpolated as in mode 0.
       max_dev, the non-finite retirement, input limits (the clip acts on u_cmd), the record, sample fans and the stop tolerance work as in
       mode 0.  Anything else: SCPP_E_ARG.  The mode stays until it is set again; it invalidates neither gains nor a covariance sweep (each
       sweep describes one loop whatever the mode: scpp_hip_lqr_propagate_covariance the continuous loop of mode 0,
       scpp_hip_lqr_propagate_covariance_discrete the held loop of mode 1). */
    int scpp_hip_lqr_set_feedback_hold(scpp_hip_lqr_ctx *ctx, int mode);
    /* gains [B][K][nu][nx], status [B][K] int32, iters [B][K] int32 (sign iterations, or RKF78 steps behind the node); any pointer may be NULL */
    int scpp_hip_lqr_download_gains(scpp_hip_lqr_ctx *ctx, double *gains, int *status, int *iters);
    /* user-supplied gains [B][K][nu][nx] for the trajectories set before; non-finite entries are refused (SCPP_E_ARG) */
    int scpp_hip_lqr_set_gains(scpp_hip_lqr_ctx *ctx, const double *gains);
    /* inputs of the covariance sweep: sigma0 [B][nx][nx], the initial state covariance of every trajectory (B == 1: one matrix for all of
       them), and w [nx], the diagonal of the disturbance intensity W (NULL: W = 0).  SCPP_E_ARG for a non-finite sigma0 entry, a sigma0 that
       is not symmetric TO THE BIT (the kernel relies on it), a negative diagonal entry of sigma0, a negative or non-finite w, B neither 1
       nor the number of trajectories; SCPP_E_STATE without trajectories.  The inputs stay until they are set again. */
    int scpp_hip_lqr_set_covariance_inputs(scpp_hip_lqr_ctx *ctx, const double *sigma0 /* [B or 1][nx][nx] */, int B, const double *w /* [nx] or NULL */);
    /* one forward sweep per trajectory under the gains the context holds, steps >= 1 RKF78 steps per segment (SCPP_E_ARG otherwise).
       SCPP_E_STATE without trajectories, flow parameters, gains or covariance inputs (or with rows for another number of trajectories).
       Per-trajectory status: SCPP_LQR_OK; SCPP_LQR_GAINS_INCOMPLETE; SCPP_LQR_NONFINITE: a non-finite node, input, flight time or gain (zeros
       in every output), or an S (or input covariance) that turned non-finite in segment k (node k+1 and every later node, and final_cov, are
       zeros; earlier nodes keep their values).  Nothing non-finite is ever written.  keep_cov != 0 also keeps S(t_k) of every node (the
       buffer, B K nx nx doubles, is allocated on the first such request).  *n_ok (optional) = trajectories with status 0.  The sweep changes
       neither the gains nor the tracking state; computing or setting gains, new trajectories, flow parameters or covariance inputs
       invalidate it. */
    int scpp_hip_lqr_propagate_covariance(scpp_hip_lqr_ctx *ctx, int steps, int keep_cov, int *n_ok);
    /* the same for the loop that holds its correction over a segment (the definition is above): one forward sweep of
       S_{i+1} = Acl_i S_i Acl_i' + Wd_i per trajectory under the gains the context holds, steps >= 1 RKF78 steps per segment for
       [Phi | Gamma] and for Wd.  Preconditions, SCPP_E_* answers, inputs (scpp_hip_lqr_set_covariance_inputs), per-trajectory status and what
       invalidates the sweep are those of scpp_hip_lqr_propagate_covariance; a Phi, Gamma, Wd, S or input covariance that turns non-finite in
       segment k zeroes node k+1, every later node and final_cov.  The result lands where scpp_hip_lqr_download_covariance reads it, which
       returns the last sweep of either kind.  Neither sweep changes gains, tracking state or the feedback-hold mode. */
    int scpp_hip_lqr_propagate_covariance_discrete(scpp_hip_lqr_ctx *ctx, int steps, int keep_cov, int *n_ok);
    /* state_std [B][K][nx] = sqrt of the diagonal of S(t_k) (an entry negative from rounding counts as 0), input_cov [B][K][nu][nu] =
       G[k] S(t_k) G[k]' (symmetric to rounding), final_cov [B][nx][nx] = S(T), status [B] int32, cov [B][K][nx][nx] = S(t_k); any pointer may
       be NULL.  SCPP_E_STATE before a sweep, and for cov after a sweep with keep_cov == 0. */
    int scpp_hip_lqr_download_covariance(scpp_hip_lqr_ctx *ctx, double *state_std /* [B][K][nx] */, double *input_cov /* [B][K][nu][nu] */,
                                         double *final_cov /* [B][nx][nx] */, int *status /* [B] */, double *cov /* [B][K][nx][nx], keep_cov only */);
    /* the covariance sweep of the continuous loop together with the loop's mean (the definition is above): one forward sweep of
       [[S, m], [m', 0]] per trajectory.  mean0 [rows][nx], rows == 1: one row for every trajectory; NULL: mean0 = 0 (rows is not read).
       Preconditions, SCPP_E_* answers, inputs (scpp_hip_lqr_set_covariance_inputs), status values and what invalidates the sweep are those of
       scpp_hip_lqr_propagate_covariance; in addition SCPP_E_ARG for feedforward not 0 or 1, a non-finite mean0, rows neither 1 nor the number
       of trajectories, and SCPP_E_STATE for feedforward == 1 without feedforward terms.  SCPP_LQR_NONFINITE: a non-finite node, input, flight
       time, gain or (feedforward == 1) feedforward term (zeros in every output), or a tile or du_mean that turned non-finite in segment k, a
       non-finite flow map at a finite point included (node k+1 and every later node, the mean and final_cov included, are zeros).  Nothing
       non-finite is ever written.  The covariance part lands where scpp_hip_lqr_download_covariance reads it, which returns the last sweep of
       any of the three kinds.  The sweep reads neither the feedforward mode nor the feedback hold and changes neither. */
    int scpp_hip_lqr_propagate_moments(scpp_hip_lqr_ctx *ctx, int steps, int keep_cov, int feedforward, const double *mean0 /* [rows][nx] or NULL */,
                                       int rows /* 1 or B */, int *n_ok);
    /* mean [B][K][nx] = m(t_k), input_mean [B][K][nu] = du_mean[k]; either pointer may be NULL.  SCPP_E_STATE unless the last sweep was
       scpp_hip_lqr_propagate_moments. */
    int scpp_hip_lqr_download_moments(scpp_hip_lqr_ctx *ctx, double *mean /* [B][K][nx] */, double *input_mean /* [B][K][nu] */);
    /* LQG: the measurement of the filter sweep, y = H e + v with e the deviation from the reference, H [ny][nx] constant and one for all
       trajectories, v white with intensity V = diag(v) (units measurement^2 s, the convention of the disturbance intensity w).  SCPP_E_ARG
       unless 1 <= ny <= 16, H finite, v finite and > 0.  H == NULL clears the measurement (ny and v are not read).  Either way an earlier
       filter result is invalidated. */
    int scpp_hip_lqr_set_measurement(scpp_hip_lqr_ctx *ctx, const double *H /* [ny][nx] or NULL */, int ny, const double *v /* [ny] */);
    /* one forward sweep per trajectory of the Kalman-Bucy error covariance Sg of eps = e - e^ and, with closed_loop, of the covariance Xh
       of the estimate under the output-feedback loop du = -K_t e^:
           dSg/dt = A Sg + Sg A' + W - Sg H' V^-1 H Sg     Sg(0) = sigma0     L(t) = Sg H' V^-1
           dXh/dt = A_cl Xh + Xh A_cl' + Sg H' V^-1 H Sg   Xh(0) = 0          A_cl = A - B K_t
       sigma0 and W = diag(w) are those of scpp_hip_lqr_set_covariance_inputs.  A is the open-loop Jacobian at the interpolated reference,
       K_t the interpolated gain, the segments, holds, integrator (steps >= 1 RKF78 steps per segment, taken as given) and Jacobian rows
       those of scpp_hip_lqr_propagate_covariance, both tiles in the same step.  Because E[e^ eps'] = 0 for these gains, the state covariance
       of the loop is Sg + Xh; the covariance of the commanded correction at node k is G[k] Xh(t_k) G[k]', not G (Sg + Xh) G'.  Sg and Xh are
       symmetric to the bit; with H = 0, Sg is bitwise the S of scpp_hip_lqr_propagate_covariance under zero gains and Xh is zero.  A fixed-step
       explicit scheme: the filter's initial transient has the rate rho = max_m (H sigma0 H')_mm / v_m, and h rho <= 1/8 keeps the scheme's error
       at the level of the other sweeps (README, "Kalman-Bucy filter"); the front ends choose steps by that rule, this call does not.
       SCPP_E_ARG for steps < 1; SCPP_E_STATE without trajectories, flow parameters, covariance inputs (or with inputs for another number of
       trajectories) or a measurement and, with closed_loop, without gains.  Per-trajectory status: SCPP_LQR_OK; SCPP_LQR_NONFINITE for a
       non-finite node, input, flight time or (closed_loop) gain (zeros in every output), or a tile, gain L_k or input covariance that turned
       non-finite in segment k (node k+1, every later node and the final matrices are zeros); with closed_loop SCPP_LQR_GAINS_INCOMPLETE as for
       the covariance sweep.  Nothing non-finite is ever written.  *n_ok = trajectories with SCPP_LQR_OK (NULL: not counted).  keep: Sg(t_k)
       and, with closed_loop, Xh(t_k) of every node are kept for the download.  The result is invalidated by whatever changes the
       trajectories, the flow parameters, the covariance inputs or the measurement and, when swept with closed_loop, by whatever changes the
       gains.  The sweep changes nothing else in the context: gains, covariance and moments results and flights are what they were. */
    int scpp_hip_lqr_filter(scpp_hip_lqr_ctx *ctx, int steps, int closed_loop, int keep, int *n_ok);
    /* L [B][K][nx][ny] = Sg(t_k) H' V^-1, error_std [B][K][nx] = sqrt diag Sg(t_k), final_error_cov [B][nx][nx] = Sg(T), status [B] int32,
       error_cov [B][K][nx][nx] = Sg(t_k); of a sweep with closed_loop also state_std [B][K][nx] = sqrt diag (Sg + Xh)(t_k), input_cov
       [B][K][nu][nu] = G[k] Xh(t_k) G[k]', final_state_cov [B][nx][nx] = (Sg + Xh)(T), estimate_cov [B][K][nx][nx] = Xh(t_k).  Any pointer may
       be NULL.  SCPP_E_STATE before a sweep, for error_cov or estimate_cov after a sweep without keep, and for any of the last four after a
       sweep without closed_loop. */
    int scpp_hip_lqr_download_filter(scpp_hip_lqr_ctx *ctx, double *L /* [B][K][nx][ny] */, double *error_std /* [B][K][nx] */,
                                     double *final_error_cov /* [B][nx][nx] */, int *status /* [B] */,
                                     double *error_cov /* [B][K][nx][nx], keep only */, double *state_std /* [B][K][nx] */,
                                     double *input_cov /* [B][K][nu][nu] */, double *final_state_cov /* [B][nx][nx] */,
                                     double *estimate_cov /* [B][K][nx][nx], keep only */);
    /* regulator mode (LQRAlgorithm.cpp:11-33, LQR_sim.cpp:43-82): with stop_tol > 0 a loop also ends once |x - x_final| < stop_tol.  The
       caller sets a constant two-node "trajectory" (X = x_final, U = u_eq, t = sim_time) and the one gain of the operating point
       (scpp_hip_lqr_set_gains), so that u = -K (x - x_final) + u_eq; the same two kernels, no third.  0 (the default) switches it off. */
    int scpp_hip_lqr_set_stop_tolerance(scpp_hip_lqr_ctx *ctx, double stop_tol);
    /* input limits of the tracking loop, SI units: lim [B][3] = (T_min, T_max, angle_max in radians) per trajectory; B == 1 broadcasts one
       row, otherwise B must equal the number of trajectories: scpp_hip_lqr_track / _track_samples return SCPP_E_STATE when it does not.
       NULL (the default) switches limits off.  SCPP_E_ARG for a non-finite entry, T_min < 0, T_max <= T_min, angle_max outside (0, pi/2),
       and, for the thrust-vector models, T_min > T_max cos(angle_max).  The limits stay until they are set again (new trajectories do not
       clear them); they invalidate neither gains nor a covariance sweep, which describe the unlimited linear loop. */
    int scpp_hip_lqr_set_input_limits(scpp_hip_lqr_ctx *ctx, const double *lim /* [B or 1][3] or NULL */, int B);
    /* process noise of the tracking loop (the definition is above): w [nx] >= 0, the diagonal of the disturbance intensity in state^2 per
       second; flight f of a call draws with the global index flight_offset + f, so a fan split over several calls flies the flights of
       one call.  NULL (the default) switches the noise off.  SCPP_E_ARG for a negative or non-finite w, which leaves the previous setting
       in place.  The setting stays until it is set again; it invalidates nothing: gains and sweeps are untouched. */
    int scpp_hip_lqr_set_disturbance(scpp_hip_lqr_ctx *ctx, const double *w /* [nx] or NULL */, unsigned long long seed,
                                     unsigned long long flight_offset);
    /* z [flights][steps][nx]: the normals the loop draws under `seed` for the global flights flight0 .. flight0 + flights - 1 on the plant
       steps step0 .. step0 + steps - 1, computed on the device by the function the loop uses.  SCPP_E_ARG for flights < 1, steps < 1,
       step0 < 0 or a NULL z.  Reads and changes no setting. */
    int scpp_hip_lqr_disturbance_normals(scpp_hip_lqr_ctx *ctx, unsigned long long seed, unsigned long long flight0, int flights, int step0,
                                         int steps, double *z /* [flights][steps][nx] */);
    /* B closed loops from x_start [B][nx] towards x_final [nx] along the trajectories: time_step > 0 (reference: 0.01), substeps >= 1 RKF78
       steps per plant step (reference: 20), at most max_steps >= 1 plant steps; the first n_record instances record every write_steps-th
       step.  *n_finite (optional) = loops that did not retire non-finite. */
    int scpp_hip_lqr_track(scpp_hip_lqr_ctx *ctx, const double *x_start, const double *x_final, int B, double time_step, int substeps,
                           int max_steps, int n_record, int write_steps, int *n_finite);
    /* F = B samples closed loops, `samples` >= 1 (SCPP_E_ARG otherwise) per trajectory, flight f along trajectory f / samples from
       x_start[f]; B is the number of trajectories.  Everything else as scpp_hip_lqr_track, which is this call with samples = 1; n_record
       counts flights (n_record <= F).  The downloads below then return F rows.  The per-flight buffers grow on demand. */
    int scpp_hip_lqr_track_samples(scpp_hip_lqr_ctx *ctx, const double *x_start /* [B*samples][nx] */, const double *x_final, int B, int samples,
                                   double time_step, int substeps, int max_steps, int n_record, int write_steps, int *n_finite);
    /* n_sat [F] int32, max_clip [F] of the last flights (zeros when they flew without limits); either pointer may be NULL.  SCPP_E_STATE
       before any flight. */
    int scpp_hip_lqr_track_download_saturation(scpp_hip_lqr_ctx *ctx, int *n_sat /* [F] */, double *max_clip /* [F] */);
    /* x [B][nx], u [B][nu] (last input), t [B], steps [B] int32, status [B] int32, err0 / err1 [B] = |x - x_final| at start / end,
       max_dev [B] = largest |x - x_ref| met; any pointer may be NULL */
    int scpp_hip_lqr_track_download(scpp_hip_lqr_ctx *ctx, double *x, double *u, double *t, int *steps, int *status, double *err0,
                                    double *err1, double *max_dev);
    /* rows of the record of the last scpp_hip_lqr_track: *n_record, *rec_cap = ceil(max_steps / write_steps) */
    int scpp_hip_lqr_track_record_size(scpp_hip_lqr_ctx *ctx, int *n_record, int *rec_cap);
    /* X [n_record][rec_cap][nx], U [n_record][rec_cap][nu], t [n_record][rec_cap], n [n_record] int32 = rows written per instance */
    int scpp_hip_lqr_track_record(scpp_hip_lqr_ctx *ctx, double *X, double *U, double *t, int *n);
    int scpp_hip_lqr_synchronize(scpp_hip_lqr_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif

"""numpy restatement of the reference's LQR path (TEST INFRASTRUCTURE, never imported by the product):

    sign_iteration / care_sign / compute_lqr   scpp_core/src/LQR.cpp:7-109
    tracker_gains                              scpp_core/src/LQRTracker.cpp:6-28
    get_input / track                          LQRTracker.cpp:43-65, trajectoryData.hpp:41-78, scpp/src/SC_tracking.cpp:48-75

It takes its Jacobians from oracle_flow and its plant step from oracle_simulate (oracle/capi.cpp), so it shares no code with the kernels in
scpp_amd/csrc/lqr/.  scipy.linalg.solve_continuous_are is the solver-independent pin (scipy_gain).

The one deviation from the reference, shared with the engine: a model with a unit-quaternion state (RocketQuat) solves the Riccati equation on
the tangent system (tangent_basis); `tangent=False` runs the reference's literal 14-state path, which is singular wherever w_B = 0.
"""
import numpy as np

import oracle_lib

ROCKETQUAT, ROCKET2D, LANDER3DOF = 0, 1, 2
MAX_ITERATIONS, EPS = 100, 1e-8


def tangent_basis(model, x):
    """N(x) [nx][nr]: identity on every state but the quaternion; on the quaternion rows the three columns of the left-multiplication
    matrix of q other than q itself, normalised.  None for a model without a constrained state."""
    if model != ROCKETQUAT:
        return None
    qw, qx, qy, qz = x[7:11]
    s = 1.0 / np.sqrt(qw * qw + qx * qx + qy * qy + qz * qz)
    N = np.zeros((14, 13))
    N[:7, :7] = np.eye(7)
    N[11:, 10:] = np.eye(3)
    N[7:11, 7:10] = np.array([[-qx, -qy, -qz], [qw, -qz, qy], [qz, qw, -qx], [-qy, qx, qw]]) * s
    return N


def is_approx(a, b, eps):
    """Eigen's isApprox for matrices: |a - b|_F^2 <= eps^2 min(|a|_F^2, |b|_F^2)"""
    return np.sum((a - b) ** 2) <= eps * eps * min(np.sum(a * a), np.sum(b * b))


def sign_iteration(M, eps=EPS, max_iterations=MAX_ITERATIONS):
    """solveSchurIterative, LQR.cpp:7-55.  Returns (P, iterations, status): 0 converged, -1 iteration limit, -2 non-finite / singular."""
    n = M.shape[0] // 2
    Ml = M.copy()
    it = 0
    while True:
        if it > max_iterations:
            return None, it, -1
        try:
            Minv = np.linalg.inv(Ml)
        except np.linalg.LinAlgError:
            return None, it + 1, -2
        Mnew = Ml - 0.5 * (Ml - Minv)
        if not np.all(np.isfinite(Mnew)):
            return None, it + 1, -2
        conv = is_approx(Mnew, Ml, eps)
        Ml = Mnew
        it += 1
        if conv:
            break
    Uf = np.vstack([Ml[:n, n:], Ml[n:, n:] + np.eye(n)])
    Vf = np.vstack([Ml[:n, :n] + np.eye(n), Ml[n:, :n]])
    P = np.linalg.lstsq(Uf, -Vf, rcond=None)[0]  # the consistent over-determined system the reference hands to a full-pivot LU
    return P, it, 0


def hamiltonian(A, B, q, r):
    """LQR.cpp:75-76 with Q (matrix) and R = diag(r)"""
    Rinv = np.diag(1.0 / np.asarray(r))
    return np.block([[A, -B @ Rinv @ B.T], [-q, -A.T]])


def compute_lqr(A, B, Q, r):
    """ComputeLQR, LQR.cpp:81-109 (Q a matrix, R = diag(r)).  Returns (K, iterations, status)."""
    P, it, st = sign_iteration(hamiltonian(A, B, Q, r))
    if st != 0:
        return np.zeros((B.shape[1], A.shape[0])), it, st
    K = np.diag(1.0 / np.asarray(r)) @ (B.T @ P)
    if not np.all(np.isfinite(K)):
        return np.zeros_like(K), it, -2
    return K, it, 0


def reduced_system(model, x, A, B, q, tangent=True):
    N = tangent_basis(model, x) if tangent else None
    Q = np.diag(np.asarray(q, dtype=np.float64))
    if N is None:
        return A, B, Q, None
    return N.T @ A @ N, N.T @ B, N.T @ Q @ N, N


def node_gain(model, x, u, par, q, r, tangent=True, perturb=None):
    """One node: Jacobians from the oracle, the (tangent) Riccati equation by the sign iteration.  `perturb`: a function applied to (A, B)
    before the solve (the generator's robustness check of the iteration count)."""
    _, A, B = oracle_lib.flow(model, x, u, par)
    if perturb is not None:
        A, B = perturb(A, B)
    Ar, Br, Qr, N = reduced_system(model, x, A, B, q, tangent)
    K, it, st = compute_lqr(Ar, Br, Qr, r)
    if N is not None:
        K = K @ N.T
    return K, it, st


def scipy_gain(model, x, u, par, q, r, tangent=True):
    """The same gain from scipy.linalg.solve_continuous_are (Schur / QZ method: no sign iteration)."""
    import scipy.linalg

    _, A, B = oracle_lib.flow(model, x, u, par)
    Ar, Br, Qr, N = reduced_system(model, x, A, B, q, tangent)
    R = np.diag(np.asarray(r, dtype=np.float64))
    P = scipy.linalg.solve_continuous_are(Ar, Br, Qr, R)
    K = np.linalg.solve(R, Br.T @ P)
    return K @ N.T if N is not None else K


def input_index(k, K, nU):
    """node k linearises at U[min(k, nU-1)]: the zero-order-hold rule (the reference special-cases k == K-2 and reads out of range at K-1)"""
    return min(k, nU - 1)


def tracker_gains(model, X, U, par, q, r, tangent=True, perturb=None):
    """LQRTracker::LQRTracker: gains [K][nu][nx], iterations [K], status [K] of one trajectory"""
    K, nU = X.shape[0], U.shape[0]
    G = np.zeros((K, U.shape[1], X.shape[1]))
    it = np.zeros(K, dtype=np.int32)
    st = np.zeros(K, dtype=np.int32)
    for k in range(K):
        G[k], it[k], st[k] = node_gain(model, X[k], U[input_index(k, K, nU)], par, q, r, tangent, perturb)
    return G, it, st


def get_input(X, U, G, t_max, t, x):
    """LQRTracker::getInput with approxStateAtTime / inputAtTime / interpolateGains as written (exact fmod, rounded division); the node index
    is clamped to K-2 where the reference would read X.at(K)."""
    K, nU = X.shape[0], U.shape[0]
    foh = nU == K
    tc = min(max(t, 0.0), t_max)
    dt = t_max / (K - 1)
    a = np.fmod(tc, dt) / dt
    i = min(int(tc / dt), K - 2)
    iu1 = i + 1 if foh else i
    x_ref = X[i] + a * (X[i + 1] - X[i])
    u_ref = U[i] + a * (U[iu1] - U[i])
    Kt = G[i] + a * (G[iu1] - G[i])
    return -Kt @ (x - x_ref) + u_ref, x_ref


def track(model, par, X, U, G, t_max, x_start, x_final, time_step=0.01, max_steps=1 << 30, halves=1):
    """SC_tracking.cpp:48-75 for one trajectory.  `halves` = 2 takes every plant step as two oracle_simulate calls of half the time step
    (the one integration variant available: oracle_simulate has 20 fixed sub-steps)."""
    x = np.array(x_start, dtype=np.float64)
    x_final = np.asarray(x_final, dtype=np.float64)
    out = dict(err0=float(np.linalg.norm(x - x_final)), max_dev=0.0, status=0, steps=0, t=0.0, u=np.zeros(U.shape[1]))
    if not (np.all(np.isfinite(x)) and np.isfinite(t_max)):
        out.update(status=-2, x=np.zeros_like(x), err0=0.0, err1=0.0)
        return out
    t, steps = 0.0, 0
    u = np.zeros(U.shape[1])
    while t < t_max:
        if steps >= max_steps:
            out["status"] = 1
            break
        u, x_ref = get_input(X, U, G, t_max, t, x)
        out["max_dev"] = max(out["max_dev"], float(np.linalg.norm(x - x_ref)))
        xn = x
        for _ in range(halves):
            xn = oracle_lib.simulate(model, par, time_step / halves, u, u, xn)
        if not np.all(np.isfinite(xn)):
            out["status"] = -2
            break
        x = xn
        t += time_step
        steps += 1
    out.update(x=x, u=u, t=t, steps=steps, err1=float(np.linalg.norm(x - x_final)))
    return out

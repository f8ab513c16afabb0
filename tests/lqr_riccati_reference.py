"""Checkers of the finite-horizon LQR gains (TEST INFRASTRUCTURE, never imported by the product; shares no code with scpp_amd/csrc/lqr/).

The definition (include/scpp_hip_lqr.h): for one trajectory of K nodes and flight time T, dt = T / (K - 1),

    -dP/dt = A(t)'P + P A(t) - P B(t) R^-1 B(t)'P + Q,    P(T) = Qf,    K_k = R^-1 B_k'P(t_k)

integrated segment by segment from segment K-2 down to 0; inside segment i, t = t_i + a dt, the reference is x = X[i] + a (X[i+1] - X[i]),
u = U[i] + a (U[j] - U[i]) with j = i+1 (first-order hold) or i (zero-order hold); the segment index is the one being integrated, never
recomputed from t.  A, B are the oracle's Jacobians (oracle_lib.flow) at (x, u); B_k is taken at (X[k], U[min(k, nU-1)]).

    exact   scipy.integrate.solve_ivp, DOP853, rtol 1e-12, restarted at every node with the segment index held fixed
    twin    numpy fixed-step RKF78 (the oracle's tableau, oracle_lib.rkf78_tableau) of the same definition, `steps` steps per segment
"""
import numpy as np

import oracle_lib


def reference_point(X, U, i, a):
    j = i + 1 if U.shape[0] == X.shape[0] else i
    return X[i] + a * (X[i + 1] - X[i]), U[i] + a * (U[j] - U[i])


def segment_of_time(K, a, i):
    """what a sweep that re-derives the segment from t would use: t = (i + a) dt -> (floor, fraction); a stage at a = 1 lands in segment i+1"""
    s = i + a
    ii = min(int(np.floor(s)), K - 2)
    return ii, s - ii


def rhs(model, par, X, U, i, a, P, q, rinv, perturb=None, retime=False):
    """dP/dtau (tau = T - t) at fraction a of segment i"""
    if retime:
        i, a = segment_of_time(X.shape[0], a, i)
    x, u = reference_point(X, U, i, a)
    _, A, B = oracle_lib.flow(model, x, u, par)
    if perturb is not None:
        A, B = perturb(A, B)
    W = P @ B
    return (P @ A + A.T @ P) - (W * rinv) @ W.T + np.diag(q)


def node_gain(model, par, X, U, k, P, r):
    """K_k = R^-1 B_k'P with B_k at (X[k], U[min(k, nU-1)]): the frozen-time kernel's linearisation point"""
    _, _, B = oracle_lib.flow(model, X[k], U[min(k, U.shape[0] - 1)], par)
    return (B.T @ P) / np.asarray(r, dtype=np.float64)[:, None]


def gains_of(model, par, X, U, P, r):
    return np.stack([node_gain(model, par, X, U, k, P[k], r) for k in range(X.shape[0])])


def twin(model, par, X, U, T, q, r, qf=None, steps=5, perturb=None, retime=False, tableau=None):
    """fixed-step RKF78, `steps` steps per segment.  Returns P [K][nx][nx], gains [K][nu][nx].  `perturb`: applied to (A, B) of every
    right-hand side (the generator's rounding floor); `retime`: the segment re-derived from t (what the definition forbids); `tableau`:
    (c, a, b) instead of the oracle's (the generator's wrong-row check)."""
    c, a_, b_ = oracle_lib.rkf78_tableau() if tableau is None else tableau
    K, nx = X.shape
    q = np.asarray(q, dtype=np.float64)
    rinv = 1.0 / np.asarray(r, dtype=np.float64)
    P = np.zeros((K, nx, nx))
    P[K - 1] = np.diag(q if qf is None else np.asarray(qf, dtype=np.float64))
    h = T / (K - 1) / steps
    for i in range(K - 2, -1, -1):
        Pc = P[i + 1].copy()
        for n in range(steps):
            kk = []
            for s in range(13):
                Ps = Pc.copy()
                if s:
                    acc = np.zeros_like(Pc)
                    for m in range(s):
                        if a_[s, m] != 0.0:
                            acc += a_[s, m] * kk[m]
                    Ps = Pc + h * acc
                kk.append(rhs(model, par, X, U, i, 1.0 - (n + c[s]) / steps, Ps, q, rinv, perturb, retime))
            acc = np.zeros_like(Pc)
            for s in range(13):
                if b_[s] != 0.0:
                    acc += b_[s] * kk[s]
            Pc = Pc + h * acc
        P[i] = Pc
    return P, gains_of(model, par, X, U, P, r)


def exact(model, par, X, U, T, q, r, qf=None, rtol=1e-12):
    """tight-tolerance answer: DOP853 per segment (restarted at every node, so the right-hand side it sees is smooth)"""
    import scipy.integrate

    K, nx = X.shape
    q = np.asarray(q, dtype=np.float64)
    rinv = 1.0 / np.asarray(r, dtype=np.float64)
    dt = T / (K - 1)
    P = np.zeros((K, nx, nx))
    P[K - 1] = np.diag(q if qf is None else np.asarray(qf, dtype=np.float64))
    for i in range(K - 2, -1, -1):
        def f(tau, y, i=i):
            return rhs(model, par, X, U, i, 1.0 - tau / dt, y.reshape(nx, nx), q, rinv).ravel()

        scale = np.abs(P[i + 1]).max()
        sol = scipy.integrate.solve_ivp(f, (0.0, dt), P[i + 1].ravel(), method="DOP853", rtol=rtol, atol=1e-13 * scale)
        assert sol.success, sol.message
        Pi = sol.y[:, -1].reshape(nx, nx)
        P[i] = 0.5 * (Pi + Pi.T)
    return P, gains_of(model, par, X, U, P, r)


def rel_gap(a, b):
    """max |a - b| relative to max |b| of the whole trajectory"""
    return float(np.abs(a - b).max() / np.abs(b).max())

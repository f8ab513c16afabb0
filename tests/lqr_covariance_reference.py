"""Checkers of the closed-loop covariance sweep (TEST INFRASTRUCTURE, never imported by the product; shares no code with scpp_amd/csrc/lqr/).

The definition (include/scpp_hip_lqr.h): for one trajectory of K nodes and flight time T, dt = T / (K - 1),

    dS/dt = A_cl(t) S + S A_cl(t)' + W,    S(0) = S0,    A_cl(t) = A(t) - B(t) K(t),    W = diag(w),    input covariance of node k: G[k] S(t_k) G[k]'

integrated segment by segment from segment 0 up to K-2; inside segment i at fraction a in [0, 1] the reference is x = X[i] + a (X[i+1] - X[i]),
u = U[i] + a (U[j] - U[i]), K_t = G[i] + a (G[j] - G[i]) with j = i+1 (first-order hold) or i (zero-order hold); the segment index is the one
being integrated, never recomputed from t.  A, B are the oracle's Jacobians (oracle_lib.flow) at (x, u).

    exact   scipy.integrate.solve_ivp, DOP853, rtol 1e-12, restarted at every node with the segment index held fixed
    twin    numpy fixed-step RKF78 (the oracle's tableau, oracle_lib.rkf78_tableau) of the same definition, `steps` steps per segment
"""
import numpy as np

import oracle_lib


def closed_loop(model, par, X, U, G, i, a, perturb=None):
    """A_cl = A - B K_t at fraction a of segment i"""
    j = i + 1 if U.shape[0] == X.shape[0] else i
    x, u = X[i] + a * (X[i + 1] - X[i]), U[i] + a * (U[j] - U[i])
    Kt = G[i] + a * (G[j] - G[i])
    _, A, B = oracle_lib.flow(model, x, u, par)
    if perturb is not None:
        A, B = perturb(A, B)
    return A - B @ Kt


def rhs(model, par, X, U, G, i, a, S, w, perturb=None):
    Acl = closed_loop(model, par, X, U, G, i, a, perturb)
    return (Acl @ S + S @ Acl.T) + np.diag(w)


def input_cov(G, S):
    """G[k] S(t_k) G[k]' of every node"""
    return np.einsum("kai,kij,kbj->kab", G, S, G)


def _inputs(X, S0, w):
    nx = X.shape[1]
    return np.array(S0, dtype=np.float64).reshape(nx, nx), (np.zeros(nx) if w is None else np.asarray(w, dtype=np.float64))


def twin(model, par, X, U, T, G, S0, w=None, steps=5, perturb=None, tableau=None):
    """fixed-step RKF78, `steps` steps per segment.  Returns S [K][nx][nx], input covariance [K][nu][nu].  `perturb`: applied to (A, B) of every
    right-hand side (the generator's rounding floor); `tableau`: (c, a, b) instead of the oracle's (the generator's wrong-sign control)."""
    c, a_, b_ = oracle_lib.rkf78_tableau() if tableau is None else tableau
    K, nx = X.shape
    S0, w = _inputs(X, S0, w)
    S = np.zeros((K, nx, nx))
    S[0] = S0
    h = T / (K - 1) / steps
    for i in range(K - 1):
        Sc = S[i].copy()
        for n in range(steps):
            kk = []
            for s in range(13):
                Ss = Sc
                if s:
                    acc = np.zeros_like(Sc)
                    for m in range(s):
                        if a_[s, m] != 0.0:
                            acc += a_[s, m] * kk[m]
                    Ss = Sc + h * acc
                kk.append(rhs(model, par, X, U, G, i, (n + c[s]) / steps, Ss, w, perturb))
            acc = np.zeros_like(Sc)
            for s in range(13):
                if b_[s] != 0.0:
                    acc += b_[s] * kk[s]
            Sc = Sc + h * acc
        S[i + 1] = Sc
    return S, input_cov(G, S)


def exact(model, par, X, U, T, G, S0, w=None, rtol=1e-12):
    """tight-tolerance answer: DOP853 per segment (restarted at every node, so the right-hand side it sees is smooth)"""
    import scipy.integrate

    K, nx = X.shape
    S0, w = _inputs(X, S0, w)
    dt = T / (K - 1)
    S = np.zeros((K, nx, nx))
    S[0] = S0
    scale = max(np.abs(S0).max(), np.abs(w).max() * T)
    for i in range(K - 1):
        def f(t, y, i=i):
            return rhs(model, par, X, U, G, i, t / dt, y.reshape(nx, nx), w).ravel()

        sol = scipy.integrate.solve_ivp(f, (0.0, dt), S[i].ravel(), method="DOP853", rtol=rtol, atol=1e-13 * scale)
        assert sol.success, sol.message
        Si = sol.y[:, -1].reshape(nx, nx)
        S[i + 1] = 0.5 * (Si + Si.T)
    return S, input_cov(G, S)


def rel_gap(a, b):
    """max |a - b| relative to max |b| of the whole trajectory"""
    return float(np.abs(a - b).max() / np.abs(b).max())


def scaled_gap(a, b):
    """max over nodes and entries of |a - b|_ij / (d_i d_j), d_i^2 = the largest diagonal entry i of b over the trajectory: the gap in units of
    each state's (input's) own standard deviation.  The states differ by orders of magnitude (a mass in kg next to a quaternion), so a gap
    relative to max|b| would check the largest state alone."""
    d = np.sqrt(np.abs(np.diagonal(b, axis1=-2, axis2=-1)).reshape(-1, b.shape[-1]).max(axis=0))
    d = np.where(d > 0.0, d, 1.0)
    return float((np.abs(a - b) / (d[:, None] * d[None, :])).max())


def symmetric_factor(S0):
    """L with L L' = S0 (Cholesky; S0 positive definite)"""
    return np.linalg.cholesky(S0)


def sigma_point_starts(x0, S0, eps):
    """the 2 nx + 1 starts of the sigma-point cross-check: x0 +- eps L e_j (j = 0..nx-1: plus, then minus), and x0 itself last"""
    L = symmetric_factor(S0)
    return np.concatenate([x0[None, :] + eps * L.T, x0[None, :] - eps * L.T, x0[None, :]])


def sigma_point_covariance(x_end, eps):
    """(1 / 2 eps^2) sum_j dx_j dx_j' over the 2 nx disturbed flights, dx_j measured from the undisturbed flight (the last row): Phi S0 Phi' in
    the linear limit, without sampling noise"""
    d = x_end[:-1] - x_end[-1]
    return d.T @ d / (2.0 * eps * eps)

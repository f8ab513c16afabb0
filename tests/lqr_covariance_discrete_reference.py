"""Checkers of the covariance sweep of the sampled-data loop (TEST INFRASTRUCTURE, never imported by the product; shares no code with
scpp_amd/csrc/lqr/).

The definition (include/scpp_hip_lqr.h): one trajectory of K nodes and flight time T, dt = T / (K - 1).  Inside segment i at
fraction a the reference is x = X[i] + a (X[i+1] - X[i]), u = U[i] + a (U[j] - U[i]), j = i+1 (first-order hold) or i (zero-order hold); the
segment index is the loop's.  The loop is du_i = -G[i] dx(t_i), held over segment i; W = diag(w) acts during the segment:

    d[Phi | Gamma]/dt = A(t) [Phi | Gamma] + [0 | B(t)],    [Phi | Gamma](t_i) = [I | 0]          (lqr_discrete_reference.transitions)
    dM/dt = A(t) M + M A(t)' + W,    M(t_i) = 0,    Wd_i = M(t_{i+1})                              (A: the open-loop Jacobian)
    Acl_i = Phi_i - Gamma_i G[i],    S_{i+1} = Acl_i S_i Acl_i' + Wd_i,    S_0 = sigma0,            input covariance of node k: G[k] S_k G[k]'

with A, B the oracle's Jacobians (oracle_lib.flow).

    disturbances        numpy fixed-step RKF78 (the oracle's tableau) of the M equation, `steps` steps per segment: the twin's Wd
    exact_disturbances  scipy.integrate.solve_ivp, DOP853, rtol 1e-12, one segment at a time with the segment index held fixed
    recursion           exactly the formulas above, Acl (S Acl') symmetrised once per node as the definition says
    twin / exact        transitions + disturbances + recursion
    constant_system     [Phi | Gamma] and Wd of a constant (A, B, W) from matrix exponentials (Van Loan's block form) in mpmath, and the
                        recursion iterated in mpmath
"""
import numpy as np

import oracle_lib
from lqr_covariance_reference import input_cov  # noqa: F401  (re-exported)
from lqr_discrete_reference import exact_transitions, transitions
from lqr_riccati_reference import reference_point, rel_gap  # noqa: F401  (rel_gap is re-exported)


def disturbance_rhs(model, par, X, U, i, a, M, w, perturb=None):
    """dM/dt at fraction a of segment i"""
    x, u = reference_point(X, U, i, a)
    _, A, B = oracle_lib.flow(model, x, u, par)
    if perturb is not None:
        A, B = perturb(A, B)
    return (A @ M + M @ A.T) + np.diag(w)


def disturbances(model, par, X, U, T, w, steps=5, perturb=None):
    """the twin's Wd [K-1][nx][nx] by fixed-step RKF78; w None or all zero: zeros, nothing integrated"""
    K, nx = X.shape
    out = np.zeros((K - 1, nx, nx))
    if w is None or not np.any(np.asarray(w) != 0.0):
        return out
    w = np.asarray(w, dtype=np.float64)
    c, a_, b_ = oracle_lib.rkf78_tableau()
    h = T / (K - 1) / steps
    for i in range(K - 1):
        Mc = np.zeros((nx, nx))
        for n in range(steps):
            kk = []
            for s in range(13):
                Ms = Mc
                if s:
                    acc = np.zeros_like(Mc)
                    for m in range(s):
                        if a_[s, m] != 0.0:
                            acc += a_[s, m] * kk[m]
                    Ms = Mc + h * acc
                kk.append(disturbance_rhs(model, par, X, U, i, (n + c[s]) / steps, Ms, w, perturb))
            acc = np.zeros_like(Mc)
            for s in range(13):
                if b_[s] != 0.0:
                    acc += b_[s] * kk[s]
            Mc = Mc + h * acc
        out[i] = Mc
    return out


def exact_disturbances(model, par, X, U, T, w, rtol=1e-12):
    import scipy.integrate

    K, nx = X.shape
    out = np.zeros((K - 1, nx, nx))
    if w is None or not np.any(np.asarray(w) != 0.0):
        return out
    w = np.asarray(w, dtype=np.float64)
    dt = T / (K - 1)
    for i in range(K - 1):
        def f(t, y, i=i):
            return disturbance_rhs(model, par, X, U, i, t / dt, y.reshape(nx, nx), w).ravel()

        sol = scipy.integrate.solve_ivp(f, (0.0, dt), np.zeros(nx * nx), method="DOP853", rtol=rtol, atol=1e-14 * np.abs(w).max() * dt)
        assert sol.success, sol.message
        Mi = sol.y[:, -1].reshape(nx, nx)
        out[i] = 0.5 * (Mi + Mi.T)
    return out


def recursion(PhiGamma, Wd, G, S0, gain_shift=0):
    """S [K][nx][nx] and the input covariance [K][nu][nu].  gain_shift = 1: segment i closed with G[i+1] (a WRONG loop, the generator's control)"""
    nseg, nx = PhiGamma.shape[0], PhiGamma.shape[1]
    S = np.zeros((nseg + 1, nx, nx))
    S[0] = np.array(S0, dtype=np.float64).reshape(nx, nx)
    for i in range(nseg):
        Acl = PhiGamma[i, :, :nx] - PhiGamma[i, :, nx:] @ G[i + gain_shift]
        F = Acl @ (S[i] @ Acl.T)
        S[i + 1] = 0.5 * (F + F.T) + Wd[i]
    return S, input_cov(G[:nseg + 1], S)


def twin(model, par, X, U, T, G, S0, w=None, steps=5, perturb=None):
    """(S, input covariance) of one trajectory by the scheme of the definition"""
    PG = transitions(model, par, X, U, T, steps, perturb)
    return recursion(PG, disturbances(model, par, X, U, T, w, steps, perturb), G, S0)


def exact(model, par, X, U, T, G, S0, w=None, PhiGamma=None):
    PG = exact_transitions(model, par, X, U, T) if PhiGamma is None else PhiGamma
    return recursion(PG, exact_disturbances(model, par, X, U, T, w), G, S0)


def kinds(S, I):
    """the three kinds the tests compare: S, state_std, input_cov"""
    return dict(S=S, state_std=np.sqrt(np.maximum(np.diagonal(S, axis1=-2, axis2=-1), 0.0)), input_cov=I)


def constant_system(A, B, w, G, S0, dt, K, dps=40):
    """S [K][nx][nx], input covariance [K][nu][nu] of a constant system under the gains G [K][nu][nx], in mpmath: [Phi | Gamma] = the upper rows of
    expm([[A, B], [0, 0]] dt), Wd = Phi F12 with expm([[-A, W], [0, A']] dt) = [[., F12], [0, Phi']] (Van Loan), then the recursion"""
    import mpmath as mp

    mp.mp.dps = dps
    nx, nu = B.shape
    aug = mp.zeros(nx + nu)
    van = mp.zeros(2 * nx)
    for r in range(nx):
        for c in range(nx):
            aug[r, c] = mp.mpf(float(A[r, c]))
            van[r, c] = -mp.mpf(float(A[r, c]))
            van[nx + r, nx + c] = mp.mpf(float(A[c, r]))
        for c in range(nu):
            aug[r, nx + c] = mp.mpf(float(B[r, c]))
        van[r, nx + r] = mp.mpf(float(w[r]))
    E = mp.expm(aug * mp.mpf(float(dt)))
    V = mp.expm(van * mp.mpf(float(dt)))
    Phi, Gam = E[:nx, :nx], E[:nx, nx:]
    Wd = Phi * V[:nx, nx:]
    Wd = (Wd + Wd.T) / 2
    S = mp.matrix(np.asarray(S0, dtype=np.float64).tolist())
    Ss, Is = [], []
    for k in range(K):
        Gm = mp.matrix(np.asarray(G[k], dtype=np.float64).tolist())
        Acl = Phi - Gam * Gm
        Ss.append(np.array(S.tolist(), dtype=np.float64))
        Is.append(np.array((Gm * S * Gm.T).tolist(), dtype=np.float64))
        S = Acl * S * Acl.T + Wd
    return np.array(Ss), np.array(Is)

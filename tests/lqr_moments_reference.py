"""Checkers of the closed-loop mean sweep (TEST INFRASTRUCTURE, never imported by the product; shares no code with scpp_amd/csrc/lqr/).

The definition (include/scpp_hip_lqr.h): for one trajectory of K nodes and flight time T, dt = T / (K - 1); inside segment i at
fraction a the reference is x = X[i] + a (X[i+1] - X[i]), u = U[i] + a (U[j] - U[i]), K_t = G[i] + a (G[j] - G[i]), k_t = ff[i] + a (ff[j] - ff[i]),
j = i+1 (first-order hold) or i (zero-order hold), the segment index being the one integrated, never recomputed from a time.  With the loop
u = u_ref - K_t e - [k_t]:

    dm/dt = (A - B K_t) m + d(t),   m(0) = mean0,   d = c - [B k_t],   c = f(x, u) - (X[i+1] - X[i]) / dt
    du_mean[k] = -G[k] m(t_k) - [ff[k]]

The equation for m is integrated AS WRITTEN, on the vector m: nothing here forms the augmented tile the kernel sweeps.  f, A, B are the
oracle's (oracle_lib.flow).  The covariance block is lqr_covariance_reference's.

    exact   scipy.integrate.solve_ivp, DOP853, rtol 1e-12, restarted at every node with the segment index held fixed
    twin    numpy fixed-step RKF78 (oracle_lib.rkf78_tableau), `steps` steps per segment
    flight  one recorded flight of lqr_affine_reference.track from X[0], read at the nodes: x(t_k) - X[k]
"""
import math

import numpy as np

import oracle_lib
import lqr_affine_reference as ar


def rhs(model, par, X, U, G, ff, i, a, dt, m, perturb=None):
    """dm/dt at fraction a of segment i (ff None: d = c)"""
    j = i + 1 if U.shape[0] == X.shape[0] else i
    x, u = X[i] + a * (X[i + 1] - X[i]), U[i] + a * (U[j] - U[i])
    Kt = G[i] + a * (G[j] - G[i])
    f, A, B = oracle_lib.flow(model, x, u, par)
    if perturb is not None:
        f, A, B = perturb(f, A, B)
    d = f - (X[i + 1] - X[i]) / dt
    if ff is not None:
        d = d - B @ (ff[i] + a * (ff[j] - ff[i]))
    return (A - B @ Kt) @ m + d


def input_mean(G, ff, m):
    """-G[k] m(t_k) - [ff[k]] of every node"""
    du = -np.einsum("kai,ki->ka", G, m)
    return du if ff is None else du - ff


def _mean0(X, mean0):
    return np.zeros(X.shape[1]) if mean0 is None else np.array(mean0, dtype=np.float64).reshape(X.shape[1])


def twin(model, par, X, U, T, G, ff=None, mean0=None, steps=5, perturb=None, tableau=None):
    """fixed-step RKF78, `steps` steps per segment -> m [K][nx], du_mean [K][nu].  `perturb`: applied to (f, A, B) of every right-hand side;
    `tableau`: (c, a, b) instead of the oracle's."""
    c, a_, b_ = oracle_lib.rkf78_tableau() if tableau is None else tableau
    K, nx = X.shape
    dt = T / (K - 1)
    h = dt / steps
    m = np.zeros((K, nx))
    m[0] = _mean0(X, mean0)
    for i in range(K - 1):
        y = m[i].copy()
        for n in range(steps):
            kk = []
            for s in range(13):
                ys = y
                if s:
                    acc = np.zeros_like(y)
                    for q in range(s):
                        if a_[s, q] != 0.0:
                            acc += a_[s, q] * kk[q]
                    ys = y + h * acc
                kk.append(rhs(model, par, X, U, G, ff, i, (n + c[s]) / steps, dt, ys, perturb))
            acc = np.zeros_like(y)
            for s in range(13):
                if b_[s] != 0.0:
                    acc += b_[s] * kk[s]
            y = y + h * acc
        m[i + 1] = y
    return m, input_mean(G, ff, m)


def exact(model, par, X, U, T, G, ff=None, mean0=None, rtol=1e-12):
    """tight-tolerance answer: DOP853 per segment (restarted at every node, so the right-hand side it sees is smooth)"""
    import scipy.integrate

    K, nx = X.shape
    dt = T / (K - 1)
    m = np.zeros((K, nx))
    m[0] = _mean0(X, mean0)
    for i in range(K - 1):
        def f(t, y, i=i):
            return rhs(model, par, X, U, G, ff, i, t / dt, dt, y)

        # m starts at zero and is made of cancellation on a nominal that nearly obeys the dynamics: its scale over one segment is what the
        # mid-segment drive feeds it
        dm = float(np.abs(rhs(model, par, X, U, G, ff, i, 0.5, dt, np.zeros(nx))).max())
        scale = max(float(np.abs(m[i]).max()), dm * dt, 1e-30)
        sol = scipy.integrate.solve_ivp(f, (0.0, dt), m[i], method="DOP853", rtol=rtol, atol=1e-13 * scale)
        assert sol.success, sol.message
        m[i + 1] = sol.y[:, -1]
    return m, input_mean(G, ff, m)


ulp_perturb = ar.ulp_perturb


def rel_gap(a, b):
    """max |a - b| relative to max |b| of the whole trajectory"""
    return float(np.abs(a - b).max() / np.abs(b).max())


def probe_mean(sigma0):
    """the mean0 of the structure tests: one standard deviation of sigma0 in every state, signs alternating"""
    sd = np.sqrt(np.diag(sigma0))
    return sd * np.where(np.arange(sd.shape[0]) % 2, -1.0, 1.0)


def outer_gap(S, m_v, m_0):
    """max over the nodes of |S_k - dm_k dm_k'|, dm = m(v) - m(0), relative to max|S|: zero in exact arithmetic when S(0) = v v' and W = 0"""
    dm = m_v - m_0
    return float(np.abs(S - np.einsum("ki,kj->kij", dm, dm)).max() / np.abs(S).max())


def plant_step(T, K, target=0.01):
    """the plant step of the flight test and the steps per segment: dt / ceil(dt / target), so that nodes fall on plant steps"""
    dt = T / (K - 1)
    n = int(math.ceil(dt / target))
    return dt / n, n


def blend(a0, a1, scale):
    """a0 + scale (a1 - a0): the nominal, gains and terms of the flight test between the plain and the bent case"""
    return a0 + scale * (a1 - a0)


def node_deviation(X, x_start, rec_x, per_segment):
    """x(t_k) - X[k] of a flight recorded at every plant step (rec_x[n]: the state after step n), per_segment plant steps per segment"""
    K = X.shape[0]
    assert rec_x.shape[0] >= (K - 1) * per_segment, (rec_x.shape, K, per_segment)
    xk = np.concatenate([np.asarray(x_start, dtype=np.float64)[None, :], rec_x[per_segment - 1:(K - 1) * per_segment:per_segment]])
    return xk - X


def flight(model, par, X, U, T, G, ff):
    """the reference flight from X[0] under (G, ff) at the plant step of plant_step, read at the nodes -> x(t_k) - X[k], [K][nx]"""
    step, n = plant_step(T, X.shape[0])
    fl = ar.track(model, par, X, U, G, ff, T, X[0], X[-1], time_step=step)
    assert fl["status"] == 0, fl["status"]
    return node_deviation(X, X[0], fl["rec_x"], n)

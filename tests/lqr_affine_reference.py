"""Checkers of the affine finite-horizon LQR law (TEST INFRASTRUCTURE, never imported by the product; shares no code with scpp_amd/csrc/lqr/).

The definition (include/scpp_hip_lqr.h): for one trajectory of K nodes and flight time T, dt = T / (K - 1); inside segment i at
fraction a the reference is x = X[i] + a (X[i+1] - X[i]), u = U[i] + a (U[j] - U[i]), j = i+1 (first-order hold) or i (zero-order hold), the
segment index being the one integrated, never recomputed from a time.  The defect is c = f(x, u) - (X[i+1] - X[i]) / dt, and

    -dP/dt = A'P + P A - P B R^-1 B'P + Q          P(T) = Qf
    -dp/dt = (A - B R^-1 B'P)'p + P c               p(T) = 0
    -ds/dt = 2 p'c - p'B R^-1 B'p                   s(T) = 0
    K_k = R^-1 B_k'P(t_k),   k_k = R^-1 B_k'p(t_k)      (B_k at (X[k], U[min(k, nU-1)]))

The three equations are integrated AS WRITTEN, on the triple (P, p, s): nothing here forms the augmented matrix the kernel sweeps.  f, A, B are
the oracle's (oracle_lib.flow).

    exact   scipy.integrate.solve_ivp, DOP853, rtol 1e-12, restarted at every node with the segment index held fixed
    twin    numpy fixed-step RKF78 (oracle_lib.rkf78_tableau), `steps` steps per segment
    track   the loop of lqr_saturation_reference.track with u_cmd = u_ref - K_t (x - x_ref) - k_t, and the record of every step
    cost    the cost of a recorded flight: sum over the plant steps of time_step (e'Q e + du'R du), e and du at the start of the step against
            the interpolated reference, plus e'Qf e of the last recorded state against X[K-1]
"""
import math

import numpy as np

import oracle_lib
from lqr_reference import get_input
from lqr_riccati_reference import reference_point, rel_gap  # noqa: F401  (rel_gap: for the tests)
from lqr_saturation_reference import saturate


def pack(P, p, s):
    return np.concatenate([P.ravel(), p, [s]])


def unpack(y, nx):
    return y[:nx * nx].reshape(nx, nx), y[nx * nx:nx * nx + nx], float(y[-1])


def rhs(model, par, X, U, i, a, dt, y, q, rinv, perturb=None):
    """d(P, p, s)/dtau (tau = T - t) at fraction a of segment i, packed"""
    nx = X.shape[1]
    P, p, _ = unpack(y, nx)
    x, u = reference_point(X, U, i, a)
    f, A, B = oracle_lib.flow(model, x, u, par)
    if perturb is not None:
        f, A, B = perturb(f, A, B)
    c = f - (X[i + 1] - X[i]) / dt
    W = P @ B
    w = B.T @ p
    dP = (P @ A + A.T @ P) - (W * rinv) @ W.T + np.diag(q)
    dp = A.T @ p - W @ (rinv * w) + P @ c
    ds = 2.0 * (p @ c) - w @ (rinv * w)
    return pack(dP, dp, ds)


def node_terms(model, par, X, U, P, p, r):
    """K [K][nu][nx], k [K][nu] with B_k at (X[k], U[min(k, nU-1)])"""
    r = np.asarray(r, dtype=np.float64)
    G, ff = [], []
    for k in range(X.shape[0]):
        _, _, B = oracle_lib.flow(model, X[k], U[min(k, U.shape[0] - 1)], par)
        G.append((B.T @ P[k]) / r[:, None])
        ff.append((B.T @ p[k]) / r)
    return np.stack(G), np.stack(ff)


def _result(model, par, X, U, Y, r):
    K, nx = X.shape
    P = np.stack([unpack(y, nx)[0] for y in Y])
    p = np.stack([unpack(y, nx)[1] for y in Y])
    s = np.array([unpack(y, nx)[2] for y in Y])
    G, ff = node_terms(model, par, X, U, P, p, r)
    return dict(P=P, p=p, s=s, K=G, k=ff)


def twin(model, par, X, U, T, q, r, qf=None, steps=5, perturb=None, tableau=None):
    """fixed-step RKF78, `steps` steps per segment -> dict P [K][nx][nx], p [K][nx], s [K], K [K][nu][nx], k [K][nu].  `perturb`: applied to
    (f, A, B) of every right-hand side; `tableau`: (c, a, b) instead of the oracle's."""
    c, a_, b_ = oracle_lib.rkf78_tableau() if tableau is None else tableau
    K, nx = X.shape
    q = np.asarray(q, dtype=np.float64)
    rinv = 1.0 / np.asarray(r, dtype=np.float64)
    dt = T / (K - 1)
    h = dt / steps
    Y = [None] * K
    Y[K - 1] = pack(np.diag(q if qf is None else np.asarray(qf, dtype=np.float64)), np.zeros(nx), 0.0)
    for i in range(K - 2, -1, -1):
        y = Y[i + 1].copy()
        for n in range(steps):
            kk = []
            for s in range(13):
                ys = y
                if s:
                    acc = np.zeros_like(y)
                    for m in range(s):
                        if a_[s, m] != 0.0:
                            acc += a_[s, m] * kk[m]
                    ys = y + h * acc
                kk.append(rhs(model, par, X, U, i, 1.0 - (n + c[s]) / steps, dt, ys, q, rinv, perturb))
            acc = np.zeros_like(y)
            for s in range(13):
                if b_[s] != 0.0:
                    acc += b_[s] * kk[s]
            y = y + h * acc
        Y[i] = y
    return _result(model, par, X, U, Y, r)


def exact(model, par, X, U, T, q, r, qf=None, rtol=1e-12):
    """tight-tolerance answer: DOP853 per segment (restarted at every node, so the right-hand side it sees is smooth)"""
    import scipy.integrate

    K, nx = X.shape
    q = np.asarray(q, dtype=np.float64)
    rinv = 1.0 / np.asarray(r, dtype=np.float64)
    dt = T / (K - 1)
    Y = [None] * K
    Y[K - 1] = pack(np.diag(q if qf is None else np.asarray(qf, dtype=np.float64)), np.zeros(nx), 0.0)
    for i in range(K - 2, -1, -1):
        def f(tau, y, i=i):
            return rhs(model, par, X, U, i, 1.0 - tau / dt, dt, y, q, rinv)

        # absolute tolerances per block: p and s start at zero and stay far below max|P| on a nominal that nearly obeys the dynamics; their
        # scale over one segment is what the mid-segment defect feeds them: |p| ~ |P| |c| dt, |s| ~ |p| |c| dt
        P1, p1, s1 = unpack(Y[i + 1], nx)
        xm, um = reference_point(X, U, i, 0.5)
        cm = float(np.abs(oracle_lib.flow(model, xm, um, par)[0] - (X[i + 1] - X[i]) / dt).max())
        sp = max(float(np.abs(p1).max()), np.abs(P1).max() * cm * dt, 1e-30)
        ss = max(abs(s1), sp * cm * dt, 1e-30)
        atol = pack(np.full((nx, nx), 1e-13 * np.abs(P1).max()), np.full(nx, 1e-13 * sp), 1e-13 * ss)
        sol = scipy.integrate.solve_ivp(f, (0.0, dt), Y[i + 1], method="DOP853", rtol=rtol, atol=atol)
        assert sol.success, sol.message
        Pi, pi, si = unpack(sol.y[:, -1], nx)
        Y[i] = pack(0.5 * (Pi + Pi.T), pi, si)
    return _result(model, par, X, U, Y, r)


def ulp_perturb(rng):
    """(f, A, B) -> the three with every entry moved by 1 ulp, sign at random"""
    eps = np.finfo(float).eps

    def g(f, A, B):
        return tuple(v * (1.0 + eps * rng.choice([-1.0, 1.0], v.shape)) for v in (f, A, B))

    return g


def feedforward_at(ff, K, nU, t_max, t):
    """k_t with the indices and the fraction of lqr_reference.get_input"""
    tc = min(max(t, 0.0), t_max)
    dt = t_max / (K - 1)
    a = np.fmod(tc, dt) / dt
    i = min(int(tc / dt), K - 2)
    j = i + 1 if nU == K else i
    return ff[i] + a * (ff[j] - ff[i])


def track(model, par, X, U, G, ff, t_max, x_start, x_final, lim=None, time_step=0.01, max_steps=1 << 30):
    """the tracking loop with the feedforward term (ff None: without).  Returns x, u, steps, status, err1, max_dev, n_sat (steps on which
    the limits changed the input) and the record of every
    step: rec_x [steps][nx] (the state after the step), rec_u [steps][nu] (the input applied in it)."""
    x = np.array(x_start, dtype=np.float64)
    x_final = np.asarray(x_final, dtype=np.float64)
    K, nU = X.shape[0], U.shape[0]
    t, steps, status, max_dev, n_sat = 0.0, 0, 0, 0.0, 0
    u = np.zeros(U.shape[1])
    rx, ru = [], []
    while t < t_max:
        if steps >= max_steps:
            status = 1
            break
        ucmd, x_ref = get_input(X, U, G, t_max, t, x)
        if ff is not None:
            ucmd = ucmd - feedforward_at(ff, K, nU, t_max, t)
        max_dev = max(max_dev, float(np.linalg.norm(x - x_ref)))
        if not np.all(np.isfinite(ucmd)):
            status = -2
            break
        u = ucmd if lim is None else saturate(model, ucmd, lim)
        n_sat += int((u != ucmd).any())
        xn = oracle_lib.simulate(model, par, time_step, u, u, x)
        if not np.all(np.isfinite(xn)):
            status = -2
            break
        x = xn
        rx.append(x)
        ru.append(u)
        t += time_step
        steps += 1
    return dict(x=x, u=u, t=t, steps=steps, status=status, max_dev=max_dev, n_sat=n_sat, err1=float(np.linalg.norm(x - x_final)),
                rec_x=np.array(rx).reshape(-1, X.shape[1]), rec_u=np.array(ru).reshape(-1, U.shape[1]))


def cost(X, U, t_max, q, r, qf, x_start, rec_x, rec_u, time_step=0.01, moved=None):
    """the cost of a recorded flight (the definition is in the module's docstring).  moved = (dx, du): returns instead the first-order bound on
    how far the cost moves when every recorded state entry moves by at most dx and every recorded input entry by at most du:
    sum of time_step 2 (|Q e|_1 dx + |R du|_1 du) over the steps, plus 2 |Qf e|_1 dx."""
    K, nU = X.shape[0], U.shape[0]
    dt = t_max / (K - 1)
    q, r, qf = (np.asarray(v, dtype=np.float64) for v in (q, r, qf))
    J = 0.0
    x = np.asarray(x_start, dtype=np.float64)
    if moved is not None:
        for n in range(rec_x.shape[0]):
            tc = min(n * time_step, t_max)
            a = math.fmod(tc, dt) / dt
            i = min(int(tc / dt), K - 2)
            j = i + 1 if nU == K else i
            e = x - (X[i] + a * (X[i + 1] - X[i]))
            du = rec_u[n] - (U[i] + a * (U[j] - U[i]))
            J += time_step * 2.0 * (float(np.abs(q * e).sum()) * (moved[0] if n else 0.0) + float(np.abs(r * du).sum()) * moved[1])
            x = rec_x[n]
        return J + 2.0 * float(np.abs(qf * (x - X[K - 1])).sum()) * moved[0]
    for n in range(rec_x.shape[0]):
        tc = min(n * time_step, t_max)
        a = math.fmod(tc, dt) / dt
        i = min(int(tc / dt), K - 2)
        j = i + 1 if nU == K else i
        e = x - (X[i] + a * (X[i + 1] - X[i]))
        du = rec_u[n] - (U[i] + a * (U[j] - U[i]))
        J += time_step * (float(e @ (q * e)) + float(du @ (r * du)))
        x = rec_x[n]
    e = x - X[K - 1]
    return J + float(e @ (qf * e))

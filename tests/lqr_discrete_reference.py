"""Checkers of the sampled-data LQR gains and of the node-rate feedback hold (TEST INFRASTRUCTURE, never imported by the product; shares no
code with scpp_amd/csrc/lqr/).

The definition (include/scpp_hip_lqr.h): one trajectory of K nodes and flight time T, dt = T / (K - 1).  Inside segment i at
fraction a the reference is x = X[i] + a (X[i+1] - X[i]), u = U[i] + a (U[j] - U[i]), j = i+1 (first-order hold) or i (zero-order hold); the
segment index is the loop's, never recomputed from the time.  A correction du_i held over segment i gives dx_{i+1} = Phi_i dx_i + Gamma_i du_i,

    d[Phi | Gamma]/dt = A(t) [Phi | Gamma] + [0 | B(t)],    [Phi | Gamma](t_i) = [I | 0]

with A, B the oracle's Jacobians (oracle_lib.flow) at (x, u), and backwards from P_{K-1} = Qf

    S_i = R dt + Gamma_i'P_{i+1} Gamma_i,   N_i = Gamma_i'P_{i+1} Phi_i,   L_i L_i' = S_i,   Y_i = L_i^-1 N_i
    K_i = L_i^-T Y_i,                       P_i = Q dt + Phi_i'P_{i+1} Phi_i - Y_i'Y_i

Node K-1: its gain is a copy of K_{K-2}, its P is Qf.

    transitions        numpy fixed-step RKF78 (the oracle's tableau) of the transition equation, `steps` steps per segment, stage s of step n
                       at a = (n + c_s) / steps: the twin
    exact_transitions  scipy.integrate.solve_ivp, DOP853, rtol 1e-12, restarted at every node with the segment index held fixed
    recursion          exactly the formulas above
    track_held         lqr_reference.track with the latch: du = -G[i] (x - x_ref(t)) at the first plant step whose segment index differs from
                       the latched one, u = u_ref(t) + du on every plant step
"""
import math

import numpy as np

import oracle_lib
from lqr_riccati_reference import reference_point, rel_gap, segment_of_time  # noqa: F401  (rel_gap is re-exported)


def transition_rhs(model, par, X, U, i, a, PG, perturb=None, retime=False):
    """d[Phi | Gamma]/dt at fraction a of segment i"""
    if retime:
        i, a = segment_of_time(X.shape[0], a, i)
    x, u = reference_point(X, U, i, a)
    _, A, B = oracle_lib.flow(model, x, u, par)
    if perturb is not None:
        A, B = perturb(A, B)
    F = A @ PG
    F[:, X.shape[1]:] += B
    return F


def transitions(model, par, X, U, T, steps=5, perturb=None, tableau=None, retime=False):
    """the twin: [Phi | Gamma] [K-1][nx][nx + nu] of every segment by fixed-step RKF78.  `perturb`: applied to (A, B) of every right-hand side
    (the generator's rounding floor); `tableau`: (c, a, b) instead of the oracle's (the generator's wrong-row check); `retime`: the segment
    re-derived from t (what the definition forbids)."""
    c, a_, b_ = oracle_lib.rkf78_tableau() if tableau is None else tableau
    K, nx = X.shape
    nu = U.shape[1]
    h = T / (K - 1) / steps
    out = np.zeros((K - 1, nx, nx + nu))
    for i in range(K - 1):
        Tc = np.hstack([np.eye(nx), np.zeros((nx, nu))])
        for n in range(steps):
            kk = []
            for s in range(13):
                Ts = Tc
                if s:
                    acc = np.zeros_like(Tc)
                    for m in range(s):
                        if a_[s, m] != 0.0:
                            acc += a_[s, m] * kk[m]
                    Ts = Tc + h * acc
                kk.append(transition_rhs(model, par, X, U, i, (n + c[s]) / steps, Ts, perturb, retime))
            acc = np.zeros_like(Tc)
            for s in range(13):
                if b_[s] != 0.0:
                    acc += b_[s] * kk[s]
            Tc = Tc + h * acc
        out[i] = Tc
    return out


def exact_transitions(model, par, X, U, T, rtol=1e-12):
    """tight-tolerance answer: DOP853 per segment (restarted at every node, so the right-hand side it sees is smooth)"""
    import scipy.integrate

    K, nx = X.shape
    nu = U.shape[1]
    dt = T / (K - 1)
    out = np.zeros((K - 1, nx, nx + nu))
    y0 = np.hstack([np.eye(nx), np.zeros((nx, nu))]).ravel()
    for i in range(K - 1):
        def f(t, y, i=i):
            return transition_rhs(model, par, X, U, i, t / dt, y.reshape(nx, nx + nu)).ravel()

        sol = scipy.integrate.solve_ivp(f, (0.0, dt), y0, method="DOP853", rtol=rtol, atol=1e-14)
        assert sol.success, sol.message
        out[i] = sol.y[:, -1].reshape(nx, nx + nu)
    return out


def recursion(PhiGamma, q, r, qf, dt):
    """P [K][nx][nx], gains [K][nu][nx] from [Phi | Gamma] [K-1][nx][nx + nu]: the formulas of the definition, as written"""
    import scipy.linalg

    nseg, nx = PhiGamma.shape[0], PhiGamma.shape[1]
    K = nseg + 1
    q, r = np.asarray(q, dtype=np.float64), np.asarray(r, dtype=np.float64)
    nu = r.shape[0]
    P = np.zeros((K, nx, nx))
    G = np.zeros((K, nu, nx))
    P[K - 1] = np.diag(q if qf is None else np.asarray(qf, dtype=np.float64))
    for i in range(K - 2, -1, -1):
        Phi, Gam = PhiGamma[i, :, :nx], PhiGamma[i, :, nx:]
        S = np.diag(r * dt) + Gam.T @ P[i + 1] @ Gam
        N = Gam.T @ P[i + 1] @ Phi
        L = np.linalg.cholesky(S)
        Y = scipy.linalg.solve_triangular(L, N, lower=True)
        G[i] = scipy.linalg.solve_triangular(L.T, Y, lower=False)
        F = Phi.T @ P[i + 1] @ Phi
        P[i] = np.diag(q * dt) + 0.5 * (F + F.T) - Y.T @ Y
    G[K - 1] = G[K - 2]
    return P, G


def twin(model, par, X, U, T, q, r, qf=None, steps=5, perturb=None, tableau=None, retime=False):
    """(PhiGamma, P, gains) of one trajectory: transitions() then recursion()"""
    PG = transitions(model, par, X, U, T, steps, perturb, tableau, retime)
    P, G = recursion(PG, q, r, qf, T / (X.shape[0] - 1))
    return PG, P, G


def exact(model, par, X, U, T, q, r, qf=None):
    PG = exact_transitions(model, par, X, U, T)
    P, G = recursion(PG, q, r, qf, T / (X.shape[0] - 1))
    return PG, P, G


def closed_loop_product(PhiGamma, G):
    """prod_i (Phi_i - Gamma_i K_i), i = K-2 .. 0 applied last to first: dx_{K-1} = M dx_0 for the sampled loop"""
    nx = PhiGamma.shape[1]
    M = np.eye(nx)
    for i in range(PhiGamma.shape[0]):
        M = (PhiGamma[i, :, :nx] - PhiGamma[i, :, nx:] @ G[i]) @ M
    return M


def segment_and_fraction(K, t_max, t):
    """the tracking loop's own arithmetic (lqr_reference.get_input): clamped time, exact fmod, rounded division, index clamped to K-2"""
    tc = min(max(t, 0.0), t_max)
    dt = t_max / (K - 1)
    return min(int(tc / dt), K - 2), math.fmod(tc, dt) / dt


def track_held(model, par, X, U, G, t_max, x_start, x_final, lim=None, time_step=0.01, max_steps=1 << 30, write_steps=0, saturate=None):
    """lqr_reference.track with the latch (and, with lim, lqr_saturation_reference's clip through `saturate`).  The same t += time_step and
    int(tc / dt) arithmetic as the device, so the latch falls on the device's plant step.  write_steps > 0: also the record (x after the step,
    applied u, t) of every write_steps-th step.  Adds n_sat, max_clip and n_latch (the latches taken)."""
    K, nU = X.shape[0], U.shape[0]
    foh = nU == K
    x = np.array(x_start, dtype=np.float64)
    x_final = np.asarray(x_final, dtype=np.float64)
    out = dict(err0=float(np.linalg.norm(x - x_final)), max_dev=0.0, status=0, steps=0, t=0.0, u=np.zeros(U.shape[1]), n_sat=0, max_clip=0.0,
               n_latch=0, rec_x=[], rec_u=[], rec_t=[])
    if not (np.all(np.isfinite(x)) and np.isfinite(t_max)):
        out.update(status=-2, x=np.zeros_like(x), err0=0.0, err1=0.0)
        return out
    t, steps = 0.0, 0
    u = np.zeros(U.shape[1])
    latched, du = -1, np.zeros(U.shape[1])
    while t < t_max:
        if steps >= max_steps:
            out["status"] = 1
            break
        i, a = segment_and_fraction(K, t_max, t)
        j = i + 1 if foh else i
        x_ref = X[i] + a * (X[i + 1] - X[i])
        out["max_dev"] = max(out["max_dev"], float(np.linalg.norm(x - x_ref)))
        if i != latched:
            du = -(G[i] @ (x - x_ref))
            latched = i
            out["n_latch"] += 1
        ucmd = du + (U[i] + a * (U[j] - U[i]))
        if not np.all(np.isfinite(ucmd)):
            out["status"] = -2
            break
        u = ucmd
        if lim is not None:
            u = saturate(model, ucmd, lim)
            if (u != ucmd).any():
                out["n_sat"] += 1
                out["max_clip"] = max(out["max_clip"], math.sqrt(sum(float(d) * float(d) for d in ucmd - u)))
        xn = oracle_lib.simulate(model, par, time_step, u, u, x)
        if not np.all(np.isfinite(xn)):
            out["status"] = -2
            break
        x = xn
        t += time_step
        if write_steps > 0 and steps % write_steps == 0:
            out["rec_x"].append(x.copy())
            out["rec_u"].append(np.array(u))
            out["rec_t"].append(t)
        steps += 1
    out.update(x=x, u=u, t=t, steps=steps, err1=float(np.linalg.norm(x - x_final)))
    return out

"""Checkers of the filter sweep (TEST INFRASTRUCTURE, never imported by the product; shares no code with scpp_amd/csrc/lqr/).

The definition (include/scpp_hip_lqr.h): for one trajectory of K nodes and flight time T, dt = T / (K - 1), a measurement
y = H e + v with H [ny][nx] constant and v white with intensity V = diag(v),

    dSg/dt = A Sg + Sg A' + W - Sg H' V^-1 H Sg,     Sg(0) = S0,    L(t) = Sg H' V^-1,    W = diag(w)      (A: the OPEN-loop Jacobian)
    dXh/dt = A_cl Xh + Xh A_cl' + Sg H' V^-1 H Sg,   Xh(0) = 0,     A_cl = A - B K_t
    state covariance of the loop du = -K_t e^: Sg + Xh;  covariance of the commanded correction at node k: G[k] Xh(t_k) G[k]'

integrated segment by segment; inside segment i at fraction a in [0, 1] the reference is x = X[i] + a (X[i+1] - X[i]),
u = U[i] + a (U[j] - U[i]), K_t = G[i] + a (G[j] - G[i]) with j = i+1 (first-order hold) or i (zero-order hold); the segment index is the one
being integrated, never recomputed from t.  A, B are the oracle's Jacobians (oracle_lib.flow) at (x, u).  G None: the filter alone (Xh = 0).

    exact        scipy.integrate.solve_ivp, DOP853, rtol 1e-12, on (Sg, Xh) together, restarted at every node
    twin         numpy fixed-step RKF78 (the oracle's tableau) of the same definition, `steps` steps per segment
    joint_exact  the 2 nx x 2 nx Lyapunov equation of z = (e, eps) under du = -K_t (e - eps) with the gain L(t) of `exact`'s own Riccati
                 equation carried along: Cov(e) without the identity Cov(e) = Sg + Xh
"""
import numpy as np

import oracle_lib
from lqr_covariance_reference import rel_gap, scaled_gap  # noqa: F401  (the gaps' units are the covariance sweep's)


def jacobians(model, par, X, U, G, i, a, perturb=None):
    """A, A_cl = A - B K_t (None without gains) at fraction a of segment i"""
    j = i + 1 if U.shape[0] == X.shape[0] else i
    x, u = X[i] + a * (X[i + 1] - X[i]), U[i] + a * (U[j] - U[i])
    _, A, B = oracle_lib.flow(model, x, u, par)
    if perturb is not None:
        A, B = perturb(A, B)
    if G is None:
        return A, None, B
    Kt = G[i] + a * (G[j] - G[i])
    return A, A - B @ Kt, B


def rhs(model, par, X, U, G, i, a, Sg, Xh, w, H, v, perturb=None):
    A, Acl, _ = jacobians(model, par, X, U, G, i, a, perturb)
    Y = H @ Sg
    S = Y.T @ (Y / v[:, None])
    Fs = (A @ Sg + Sg @ A.T) + np.diag(w) - S
    Fx = np.zeros_like(Sg) if Acl is None else (Acl @ Xh + Xh @ Acl.T) + S
    return Fs, Fx


def gain(Sg, H, v):
    """L = Sg H' V^-1 of every node: [K][nx][ny]"""
    return np.einsum("kij,mj->kim", Sg, H) / v[None, None, :]


def input_cov(G, Xh):
    """G[k] Xh(t_k) G[k]' of every node"""
    return np.einsum("kai,kij,kbj->kab", G, Xh, G)


def _inputs(X, S0, w, H, v):
    nx = X.shape[1]
    H = np.asarray(H, dtype=np.float64).reshape(-1, nx)
    return (np.array(S0, dtype=np.float64).reshape(nx, nx), (np.zeros(nx) if w is None else np.asarray(w, dtype=np.float64)), H,
            np.asarray(v, dtype=np.float64).reshape(H.shape[0]))


def _result(G, Sg, Xh, H, v):
    out = dict(Sg=Sg, Xh=Xh, L=gain(Sg, H, v))
    if G is not None:
        out["I"] = input_cov(G, Xh)
    return out


def twin(model, par, X, U, T, G, S0, w, H, v, steps=5, perturb=None, tableau=None):
    """fixed-step RKF78, `steps` steps per segment.  Returns dict(Sg [K][nx][nx], Xh, L [K][nx][ny], I [K][nu][nu] with gains).  `perturb`:
    applied to (A, B) of every right-hand side (the generator's rounding floor); `tableau`: (c, a, b) instead of the oracle's."""
    c, a_, b_ = oracle_lib.rkf78_tableau() if tableau is None else tableau
    K, nx = X.shape
    S0, w, H, v = _inputs(X, S0, w, H, v)
    Sg, Xh = np.zeros((K, nx, nx)), np.zeros((K, nx, nx))
    Sg[0] = S0
    h = T / (K - 1) / steps
    for i in range(K - 1):
        y = np.stack([Sg[i], Xh[i]])
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
                kk.append(np.stack(rhs(model, par, X, U, G, i, (n + c[s]) / steps, ys[0], ys[1], w, H, v, perturb)))
            acc = np.zeros_like(y)
            for s in range(13):
                if b_[s] != 0.0:
                    acc += b_[s] * kk[s]
            y = y + h * acc
        Sg[i + 1], Xh[i + 1] = y
    return _result(G, Sg, Xh, H, v)


def exact(model, par, X, U, T, G, S0, w, H, v, rtol=1e-12):
    """tight-tolerance answer: DOP853 per segment on (Sg, Xh) (restarted at every node, so the right-hand side it sees is smooth)"""
    import scipy.integrate

    K, nx = X.shape
    S0, w, H, v = _inputs(X, S0, w, H, v)
    dt = T / (K - 1)
    Sg, Xh = np.zeros((K, nx, nx)), np.zeros((K, nx, nx))
    Sg[0] = S0
    sd = np.sqrt(np.maximum(np.diag(S0), w * T))
    sd = np.where(sd > 0.0, sd, 1.0)
    atol = 1e-13 * np.tile(np.outer(sd, sd).ravel(), 2)
    for i in range(K - 1):
        def f(t, y, i=i):
            Fs, Fx = rhs(model, par, X, U, G, i, t / dt, y[:nx * nx].reshape(nx, nx), y[nx * nx:].reshape(nx, nx), w, H, v)
            return np.concatenate([Fs.ravel(), Fx.ravel()])

        sol = scipy.integrate.solve_ivp(f, (0.0, dt), np.concatenate([Sg[i].ravel(), Xh[i].ravel()]), method="DOP853", rtol=rtol, atol=atol)
        assert sol.success, sol.message
        a, b = sol.y[:nx * nx, -1].reshape(nx, nx), sol.y[nx * nx:, -1].reshape(nx, nx)
        Sg[i + 1], Xh[i + 1] = 0.5 * (a + a.T), 0.5 * (b + b.T)
    return _result(G, Sg, Xh, H, v)


def joint_exact(model, par, X, U, T, G, S0, w, H, v, rtol=1e-12):
    """Cov(e)(t_k) [K][nx][nx] from the joint system of z = (e, eps), eps = e - e^, under du = -K_t e^ = -K_t (e - eps):
        de   = (A - B K_t) e + B K_t eps + n_w                     dZ/dt = F Z + Z F' + N W_n N',   Z(0) = [[S0, S0], [S0, S0]]
        deps = (A - L H) eps + n_w - L n_v                          (e^(0) = 0: e(0) = eps(0))
    with L = Sg H' V^-1 of the filter's Riccati equation, integrated alongside.  No use is made of Cov(e) = Sg + Xh."""
    import scipy.integrate

    K, nx = X.shape
    S0, w, H, v = _inputs(X, S0, w, H, v)
    dt = T / (K - 1)
    n2 = 4 * nx * nx
    Z = np.block([[S0, S0], [S0, S0]])
    Sg = S0.copy()
    out = np.zeros((K, nx, nx))
    out[0] = S0
    sd = np.sqrt(np.maximum(np.diag(S0), w * T))
    sd = np.where(sd > 0.0, sd, 1.0)
    sd2 = np.concatenate([sd, sd])
    atol = 1e-13 * np.concatenate([np.outer(sd2, sd2).ravel(), np.outer(sd, sd).ravel()])
    W = np.diag(w)
    for i in range(K - 1):
        def f(t, y, i=i):
            Zc, Sc = y[:n2].reshape(2 * nx, 2 * nx), y[n2:].reshape(nx, nx)
            A, Acl, B = jacobians(model, par, X, U, G, i, t / dt)
            Lt = (Sc @ H.T) / v[None, :]
            F = np.block([[Acl, A - Acl], [np.zeros((nx, nx)), A - Lt @ H]])
            LVL = (Lt * v[None, :]) @ Lt.T
            Q = np.block([[W, W], [W, W + LVL]])
            dS = (A @ Sc + Sc @ A.T) + W - LVL
            return np.concatenate([(F @ Zc + Zc @ F.T + Q).ravel(), dS.ravel()])

        sol = scipy.integrate.solve_ivp(f, (0.0, dt), np.concatenate([Z.ravel(), Sg.ravel()]), method="DOP853", rtol=rtol, atol=atol)
        assert sol.success, sol.message
        Z, Sg = sol.y[:n2, -1].reshape(2 * nx, 2 * nx), sol.y[n2:, -1].reshape(nx, nx)
        Z, Sg = 0.5 * (Z + Z.T), 0.5 * (Sg + Sg.T)
        out[i + 1] = Z[:nx, :nx]
    return out


# the fixture's cases (hold, gain law, w1: W = diag(w) / w0: W = 0) and the quantities a gap is measured for
CASES = [(hold, law, "w1") for hold in ("foh", "zoh") for law in ("frozen", "riccati")] + [("foh", "riccati", "w0")]
QUANTITIES = ("Sg", "Xh", "L", "I", "sd")
EPS = np.finfo(float).eps


def ulp_perturb(rng):
    def f(A, B):
        return A * (1.0 + EPS * rng.choice([-1.0, 1.0], A.shape)), B * (1.0 + EPS * rng.choice([-1.0, 1.0], B.shape))

    return f


def gaps(a, b, H, v):
    """the five gaps of result a against result b (dicts of lqr_filter_reference.twin / exact), in the units named above"""
    Pa, Pb = a["Sg"] + a["Xh"], b["Sg"] + b["Xh"]
    d = np.sqrt(np.abs(np.diagonal(b["Sg"], axis1=1, axis2=2)).max(axis=0))
    dy = np.sqrt(np.abs(np.einsum("mi,kij,mj->km", H, b["Sg"], H)).max(axis=0))
    sc = np.where(d > 0, d, 1.0)[:, None] * np.where(dy > 0, dy, 1.0)[None, :] / v[None, :]
    sa, sb = np.sqrt(np.diagonal(Pa, axis1=1, axis2=2)), np.sqrt(np.diagonal(Pb, axis1=1, axis2=2))
    return dict(Sg=scaled_gap(a["Sg"], b["Sg"]), Xh=scaled_gap(Pb + (a["Xh"] - b["Xh"]), Pb), L=float((np.abs(a["L"] - b["L"]) / sc[None]).max()),
                I=scaled_gap(a["I"], b["I"]), sd=float((np.abs(sa - sb) / sb.max(axis=0)[None, :]).max()))


def perturbed_twin(model, par, X, U, T, G, S0, w, H, v, steps, rng):
    """the twin with Jacobians, H (for L) and G (for G Xh G') perturbed by 1 ulp"""
    p = twin(model, par, X, U, T, G, S0, w, H, v, steps=steps, perturb=ulp_perturb(rng))
    p["L"] = gain(p["Sg"], H * (1.0 + EPS * rng.choice([-1.0, 1.0], H.shape)), v)
    p["I"] = input_cov(G * (1.0 + EPS * rng.choice([-1.0, 1.0], G.shape)), p["Xh"])
    return p


def selection(nx, states):
    """H [len(states)][nx] that picks the given states"""
    H = np.zeros((len(states), nx))
    H[np.arange(len(states)), list(states)] = 1.0
    return H


def auto_steps(sigma0, H, v, dt_max, floor=5, ratio=8.0):
    """the front ends' step rule: (steps, rho) with steps the smallest >= floor such that h rho <= 1 / ratio, h = dt_max / steps,
    rho = max_m (H sigma0 H')_mm / v_m over every sigma0 given"""
    S = np.asarray(sigma0, dtype=np.float64).reshape(-1, H.shape[1], H.shape[1])
    rho = float((np.einsum("mi,bij,mj->bm", H, S, H) / np.asarray(v)[None, :]).max())
    return max(int(floor), int(np.ceil(ratio * rho * float(dt_max) * (1.0 - 1e-12)))), rho

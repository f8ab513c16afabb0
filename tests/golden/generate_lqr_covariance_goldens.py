"""Goldens of the covariance-sweep tests (tests/test_lqr_covariance.py):
    python tests/golden/generate_lqr_covariance_goldens.py  ->  tests/golden/lqr_covariance_<model>.npz

numpy / scipy / the oracle only (tests/lqr_covariance_reference.py, tests/lqr_reference.py); nothing here touches the kernels under test.
Inputs, read only: the trajectories of tests/golden/lqr_<model>.npz with their frozen-time gains (G_ref) and the finite-horizon gains of
tests/golden/lqr_riccati_<model>.npz (G_exact).  STEPS = 5 RKF78 steps per segment.

Stored per model: sigma0 (a full, positive definite initial covariance: standard deviations of 2 % of the largest |state| along the golden
trajectories, at most 5, plus 0.01 -- so that no state, the mass in kg least of all, dwarfs the others --, a random correlation), w
(disturbance intensity: 2 % of the initial variance per second).  Per hold, gain law
(frozen / riccati), disturbance (w0: W = 0, w1: W = diag(w)) and trajectory:
    S_exact, I_exact    the tight-tolerance answer (DOP853, rtol 1e-12, restarted at every node): S(t_k) as its packed upper triangle, G S G'
    gap_scheme_S / _I   twin vs exact, every entry in units of its two states' (inputs') largest standard deviation along the trajectory
                        (lqr_covariance_reference.scaled_gap): the truncation error of the scheme at STEPS
    gap_round_S / _I    twin vs a copy of itself whose Jacobians are perturbed by 1 ulp at every right-hand side: the rounding floor of the sweep.
                        The copy's G S G' is formed with a gain perturbed by 1 ulp as well: the two copies of S differ by the sweep's floor, but
                        the node product is a rounded computation of its own (2 nx nu products per entry, which cancel: max|G S G'| is
                        orders below sum |G||S||G|'), and with the same gain on both sides that rounding would be left out of the floor
                        (it came out BELOW one ulp of the result for some cases, which no computed quantity can meet).
    wrong_sign_gap      twin with the sign of ONE tableau entry flipped (a[9][8]) vs exact
Asserted here, with the reference alone (the tests rely on each):
    * the wrong-sign twin misses the tests' bar (gap_scheme + 10 gap_round) by a factor >= 100, so the bar resolves a wrong tableau entry;
    * the exact S(t_k) is positive semi-definite at every node to 1e-12 of max|S|.
The sigma-point cross-check (first-order hold, trajectory 0, frozen-time gains, W = 0): the 2 nx + 1 flights x_nom(0) +- eps L e_j, L L' = sigma0,
flown by the numpy restatement of the tracking loop (lqr_reference.track), S_mc = (1 / 2 eps^2) sum_j dx_j dx_j' at the final time against the
exact S(T), at two values of eps and two of the time step (which term dominates is printed); eps is halved from 0.5 until halving it again
moves the gap by less than a tenth; stored: xc_eps, xc_gap (at the golden time step).
Rocket2D also stores the stationary case: a constant two-node system at the operating point under the gain of scipy's algebraic Riccati
solution, W = diag(w), the horizon (a multiple of 5 s, 20 steps per second) at which the twin's S(T) is within 1e-8 of
scipy.linalg.solve_continuous_lyapunov(A_cl, -W): stat_horizon, stat_steps, stat_gap.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lqr_covariance_reference as cr  # noqa: E402
import lqr_reference as ref  # noqa: E402
import oracle_lib  # noqa: E402

MODELS = {"rocketquat": 0, "rocket2d": 1, "lander3dof": 2}
STEPS = 5
LAWS = {"frozen": ("d", "G_ref"), "riccati": ("g", "G_exact")}


def ulp_perturb(rng):
    eps = np.finfo(float).eps

    def f(A, B):
        return A * (1.0 + eps * rng.choice([-1.0, 1.0], A.shape)), B * (1.0 + eps * rng.choice([-1.0, 1.0], B.shape))

    return f


def make_inputs(d, rng):
    X = np.concatenate([d["foh_X"].reshape(-1, d["foh_X"].shape[-1]), d["zoh_X"].reshape(-1, d["zoh_X"].shape[-1])])
    nx = X.shape[1]
    sd = np.minimum(0.02 * np.abs(X).max(axis=0), 5.0) + 0.01
    M = rng.standard_normal((nx, nx))
    C = M @ M.T / nx + np.eye(nx)
    s = 1.0 / np.sqrt(np.diag(C))
    S0 = (C * s[:, None] * s[None, :]) * sd[:, None] * sd[None, :]
    S0 = np.triu(S0) + np.triu(S0, 1).T  # symmetric to the bit
    assert (S0 == S0.T).all() and np.linalg.eigvalsh(S0).min() > 0.0
    return S0, 0.02 * sd * sd


def stationary_case(par, q, r, S0, w):
    import scipy.linalg

    import scpp_amd

    m = scpp_amd.Rocket2D().loadParameters()
    x_eq, u_eq = (np.asarray(v, dtype=np.float64) for v in m.getOperatingPoint())
    _, A, B = oracle_lib.flow(1, x_eq, u_eq, par)
    Pc = scipy.linalg.solve_continuous_are(A, B, np.diag(q), np.diag(r))
    Kc = (B.T @ Pc) / r[:, None]
    Acl = A - B @ Kc
    assert np.linalg.eigvals(Acl).real.max() < 0.0
    Sl = scipy.linalg.solve_continuous_lyapunov(Acl, -np.diag(w))
    X, U, G = np.tile(x_eq, (2, 1)), np.tile(u_eq, (2, 1)), np.tile(Kc, (2, 1, 1))
    for T in np.arange(5.0, 400.0, 5.0):
        steps = int(20 * T)
        St, _ = cr.twin(1, par, X, U, float(T), G, S0, w, steps=steps)
        gap = cr.rel_gap(St[1], Sl)
        print(f"   stationary case, horizon {T:5.1f} s, {steps} steps: twin S(T) vs Lyapunov {gap:.2e}")
        if gap <= 1e-8:
            break
    else:
        raise AssertionError("no horizon reaches 1e-8")
    return dict(stat_horizon=np.array(float(T)), stat_steps=np.array(steps), stat_gap=np.array(gap))


def cross_check(model, d, S0):
    """the sigma-point flights of the restatement's loop against the exact S(T)"""
    par, X, U, T, G = d["par"], d["foh_X"][0], d["foh_U"][0], float(d["foh_t"][0]), d["foh_G_ref"][0]
    Se, _ = cr.exact(model, par, X, U, T, G, S0)
    ts0 = float(d["time_step"])

    def gap(eps, ts):
        xs = cr.sigma_point_starts(X[0], S0, eps)
        xe = np.array([ref.track(model, par, X, U, G, T, x, X[-1], ts)["x"] for x in xs])
        return cr.rel_gap(cr.sigma_point_covariance(xe, eps), Se[-1])

    eps = 0.5
    ge = gap(eps, ts0)
    while True:
        gh = gap(eps / 2, ts0)
        print(f"   sigma points: eps {eps:.4g} gap {ge:.3e}, eps {eps / 2:.4g} gap {gh:.3e} (time step {ts0})")
        if abs(gh - ge) < 0.1 * ge:
            break
        eps, ge = eps / 2, gh
        assert eps > 1e-4
    g2, g2h = gap(eps, ts0 / 2), gap(eps / 2, ts0 / 2)
    print(f"   sigma points at time step {ts0 / 2}: eps {eps:.4g} gap {g2:.3e}, eps {eps / 2:.4g} gap {g2h:.3e}; chosen eps {eps:.4g}, stored gap {ge:.3e} "
          f"of max|S(T)| = {np.abs(Se[-1]).max():.3e}")
    return dict(xc_eps=np.array(eps), xc_gap=np.array(ge), xc_gap_half_eps=np.array(gh), xc_gap_half_step=np.array(g2), xc_S_exact=Se[-1])


def generate(name, seed):
    model = MODELS[name]
    src = dict(d=np.load(os.path.join(HERE, f"lqr_{name}.npz")), g=np.load(os.path.join(HERE, f"lqr_riccati_{name}.npz")))
    d = src["d"]
    par = d["par"]
    rng = np.random.default_rng(seed)
    S0, w = make_inputs(d, rng)
    nx = S0.shape[0]
    iu = np.triu_indices(nx)
    c, a, b = oracle_lib.rkf78_tableau()
    a_wrong = a.copy()
    assert a_wrong[9, 8] != 0.0
    a_wrong[9, 8] = -a_wrong[9, 8]
    out = dict(steps=np.array(STEPS), sigma0=S0, w=w)
    print(f"{name}: initial standard deviations {np.sqrt(np.diag(S0)).round(4)}, w {w}")
    for hold in ("foh", "zoh"):
        X, U, t = d[f"{hold}_X"], d[f"{hold}_U"], d[f"{hold}_t"]
        n, K = X.shape[0], X.shape[1]
        for law, (which, key) in LAWS.items():
            G = src[which][f"{hold}_{key}"]
            for wc, wv in (("w0", None), ("w1", w)):
                tag = f"{hold}_{law}_{wc}"
                Se, Ie = np.zeros((n, K, nx, nx)), np.zeros((n, K, U.shape[2], U.shape[2]))
                m = {k: np.zeros(n) for k in ("gap_scheme_S", "gap_scheme_I", "gap_round_S", "gap_round_I", "wrong_sign_gap")}
                for i in range(n):
                    T = float(t[i])
                    Se[i], Ie[i] = cr.exact(model, par, X[i], U[i], T, G[i], S0, wv)
                    St, It = cr.twin(model, par, X[i], U[i], T, G[i], S0, wv, steps=STEPS)
                    Sp, _ = cr.twin(model, par, X[i], U[i], T, G[i], S0, wv, steps=STEPS, perturb=ulp_perturb(rng))
                    Ip = cr.input_cov(G[i] * (1.0 + np.finfo(float).eps * rng.choice([-1.0, 1.0], G[i].shape)), Sp)
                    Sw, _ = cr.twin(model, par, X[i], U[i], T, G[i], S0, wv, steps=STEPS, tableau=(c, a_wrong, b))
                    m["gap_scheme_S"][i], m["gap_scheme_I"][i] = cr.scaled_gap(St, Se[i]), cr.scaled_gap(It, Ie[i])
                    m["gap_round_S"][i], m["gap_round_I"][i] = cr.scaled_gap(Sp, St), cr.scaled_gap(Ip, It)
                    m["wrong_sign_gap"][i] = cr.scaled_gap(Sw, Se[i])
                    ev = min(np.linalg.eigvalsh(Se[i, k]).min() for k in range(K))
                    print(f"{name} {tag} {i}: max|S| {np.abs(Se[i]).max():.3e}, max|GSG'| {np.abs(Ie[i]).max():.3e}, final position std "
                          f"{np.sqrt(np.diag(Se[i, -1]))[:3].round(4)}, smallest eigenvalue {ev:.2e}; " + ", ".join(f"{k} {v[i]:.2e}" for k, v in m.items()))
                    bar = m["gap_scheme_S"][i] + 10.0 * m["gap_round_S"][i]
                    assert ev >= -1e-12 * np.abs(Se[i]).max(), (name, tag, i, ev)
                    assert m["gap_round_S"][i] > 0.0 and m["gap_round_I"][i] > 0.0
                    assert m["wrong_sign_gap"][i] >= 100.0 * bar, (name, tag, i, m["wrong_sign_gap"][i], bar)
                out.update({f"{tag}_S_exact": Se[:, :, iu[0], iu[1]], f"{tag}_I_exact": Ie})
                out.update({f"{tag}_{k}": v for k, v in m.items()})
    out.update(cross_check(model, d, S0))
    if name == "rocket2d":
        out.update(stationary_case(par, d["q"], d["r"], S0, w))
    path = os.path.join(HERE, f"lqr_covariance_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    for which in sys.argv[1:] or ["rocket2d", "lander3dof", "rocketquat"]:
        generate(which, dict(rocket2d=21, lander3dof=22, rocketquat=23)[which])

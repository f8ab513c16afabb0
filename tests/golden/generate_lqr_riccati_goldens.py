"""Goldens of the finite-horizon LQR tests (tests/test_lqr_riccati.py):
    python tests/golden/generate_lqr_riccati_goldens.py  ->  tests/golden/lqr_riccati_<model>.npz

numpy / scipy / the oracle only (tests/lqr_riccati_reference.py, tests/lqr_reference.py); nothing here touches the kernels under test.
Inputs: the trajectories, weights and dispersed starts of tests/golden/lqr_<model>.npz, read only; Qf = Q; STEPS = 5 RKF78 steps per segment.

Measured and stored per model and hold (per trajectory):
    gap_scheme_P / _G   twin vs exact, relative to max|P| / max|K| of the trajectory: the truncation error of the scheme at STEPS
    gap_round_P / _G    twin vs a copy of itself whose Jacobians are perturbed by 1 ulp at every right-hand side: the rounding floor of the sweep
    P_exact, G_exact    the tight-tolerance answer (DOP853, rtol 1e-12, restarted at every node)
    err_exact           |x_end - x_final| of the eight dispersed flights of trajectory 0 under the exact gains (lqr_reference.track)
    wrong_row_gap       twin with the sign of ONE tableau entry flipped (a[9][8]) vs exact
    retime_gap          twin that re-derives the segment from t vs exact (zero-order hold: what the fixed segment index is for)
Asserted here, with the reference alone (the tests rely on each):
    * gap_scheme <= 1e-9 for every case: two orders below the best fixed-step RK4 figure at the same step count (3e-8, RocketQuat), and
      the wrong-row twin misses the tests' bar (gap_scheme + 10 gap_round) by a factor >= 100, so the bar resolves a wrong tableau row;
    * the exact P(t_k) is positive definite at every node;
    * every one of the eight flights under the exact gains ends closer to x_final than the stored open-loop error;
    * zero-order hold: the re-timed twin misses the exact answer by >= 1e4 x the tests' bar.
Rocket2D also stores the constant-system case: the horizon (a multiple of 5 s) at which the exact P(0) and gain of a two-node constant
trajectory at the operating point are within 1e-8 of scipy.linalg.solve_continuous_are's, and the step count (20 per second of horizon)
at which the twin is asserted to be within 1e-9 of the exact answer there.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lqr_reference as ref  # noqa: E402
import lqr_riccati_reference as rr  # noqa: E402
import oracle_lib  # noqa: E402

MODELS = {"rocketquat": 0, "rocket2d": 1, "lander3dof": 2}
STEPS = 5


def ulp_perturb(rng):
    eps = np.finfo(float).eps

    def f(A, B):
        return A * (1.0 + eps * rng.choice([-1.0, 1.0], A.shape)), B * (1.0 + eps * rng.choice([-1.0, 1.0], B.shape))

    return f


def constant_case(par, q, r):
    import scipy.linalg

    import scpp_amd

    m = scpp_amd.Rocket2D().loadParameters()
    x_eq, u_eq = (np.asarray(v, dtype=np.float64) for v in m.getOperatingPoint())
    _, A, B = oracle_lib.flow(1, x_eq, u_eq, par)
    Pc = scipy.linalg.solve_continuous_are(A, B, np.diag(q), np.diag(r))
    Kc = (B.T @ Pc) / r[:, None]
    X, U = np.tile(x_eq, (2, 1)), np.tile(u_eq, (2, 1))
    for T in np.arange(5.0, 400.0, 5.0):
        Pe, Ge = rr.exact(1, par, X, U, float(T), q, r)
        gp, gk = rr.rel_gap(Pe[0], Pc), rr.rel_gap(Ge[0], Kc)
        print(f"   constant system, horizon {T:5.1f} s: exact P(0) vs CARE {gp:.2e}, gain {gk:.2e}")
        if gp <= 1e-8 and gk <= 1e-8:
            break
    else:
        raise AssertionError("no horizon reaches 1e-8")
    steps = int(20 * T)
    Pt, Gt = rr.twin(1, par, X, U, float(T), q, r, steps=steps)
    sp, sk = rr.rel_gap(Pt[0], Pe[0]), rr.rel_gap(Gt[0], Ge[0])
    print(f"   twin at {steps} steps vs exact: P {sp:.2e}, gain {sk:.2e}")
    assert sp <= 1e-9 and sk <= 1e-9, (sp, sk)
    return dict(const_horizon=np.array(float(T)), const_steps=np.array(steps), const_gap_P=np.array(gp), const_gap_G=np.array(gk),
                const_scheme_P=np.array(sp), const_scheme_G=np.array(sk))


def generate(name, seed):
    model = MODELS[name]
    d = np.load(os.path.join(HERE, f"lqr_{name}.npz"))
    par, q, r = d["par"], d["q"], d["r"]
    rng = np.random.default_rng(seed)
    c, a, b = oracle_lib.rkf78_tableau()
    a_wrong = a.copy()
    assert a_wrong[9, 8] != 0.0
    a_wrong[9, 8] = -a_wrong[9, 8]
    out = dict(steps=np.array(STEPS))
    for hold in ("foh", "zoh"):
        X, U, t = d[f"{hold}_X"], d[f"{hold}_U"], d[f"{hold}_t"]
        n, K = X.shape[0], X.shape[1]
        Pe, Ge = np.zeros((n, K, X.shape[2], X.shape[2])), np.zeros((n, K, U.shape[2], X.shape[2]))
        g = {k: np.zeros(n) for k in ("gap_scheme_P", "gap_scheme_G", "gap_round_P", "gap_round_G", "wrong_row_gap", "retime_gap")}
        for i in range(n):
            T = float(t[i])
            Pe[i], Ge[i] = rr.exact(model, par, X[i], U[i], T, q, r)
            Pt, Gt = rr.twin(model, par, X[i], U[i], T, q, r, steps=STEPS)
            Pp, Gp = rr.twin(model, par, X[i], U[i], T, q, r, steps=STEPS, perturb=ulp_perturb(rng))
            Pw, _ = rr.twin(model, par, X[i], U[i], T, q, r, steps=STEPS, tableau=(c, a_wrong, b))
            Pr, _ = rr.twin(model, par, X[i], U[i], T, q, r, steps=STEPS, retime=True)
            g["gap_scheme_P"][i], g["gap_scheme_G"][i] = rr.rel_gap(Pt, Pe[i]), rr.rel_gap(Gt, Ge[i])
            g["gap_round_P"][i], g["gap_round_G"][i] = rr.rel_gap(Pp, Pt), rr.rel_gap(Gp, Gt)
            g["wrong_row_gap"][i], g["retime_gap"][i] = rr.rel_gap(Pw, Pe[i]), rr.rel_gap(Pr, Pe[i])
            ev = min(np.linalg.eigvalsh(Pe[i, k]).min() for k in range(K))
            print(f"{name} {hold} {i}: max|P| {np.abs(Pe[i]).max():.3e}, smallest eigenvalue over the nodes {ev:.3e}; " +
                  ", ".join(f"{k} {v[i]:.2e}" for k, v in g.items()))
            assert ev > 0.0, (name, hold, i, ev)
            bar = g["gap_scheme_P"][i] + 10.0 * g["gap_round_P"][i]
            assert g["gap_scheme_P"][i] <= 1e-9 and g["gap_scheme_G"][i] <= 1e-9, (name, hold, i)
            assert g["gap_round_P"][i] > 0.0 and g["gap_round_G"][i] > 0.0
            assert g["wrong_row_gap"][i] >= 100.0 * bar, (name, hold, i, g["wrong_row_gap"][i], bar)
            if hold == "zoh":
                assert g["retime_gap"][i] >= 1e4 * bar, (name, hold, i, g["retime_gap"][i], bar)
        xs, xf, e_open = d[f"{hold}_starts"], X[0, -1], d[f"{hold}_err_open"]
        e = np.array([ref.track(model, par, X[0], U[0], Ge[0], float(t[0]), x, xf, float(d["time_step"]))["err1"] for x in xs])
        print(f"   flights under the exact gains {np.round(e, 3)}\n   frozen-time (stored)          {np.round(d[f'{hold}_err_closed'], 3)}\n   open loop {np.round(e_open, 2)}")
        assert (e < e_open).all(), (name, hold, e, e_open)
        out.update({f"{hold}_P_exact": Pe, f"{hold}_G_exact": Ge, f"{hold}_err_exact": e})
        out.update({f"{hold}_{k}": v for k, v in g.items()})
    if name == "rocket2d":
        out.update(constant_case(par, q, r))
    path = os.path.join(HERE, f"lqr_riccati_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    for w in sys.argv[1:] or ["rocket2d", "lander3dof", "rocketquat"]:
        generate(w, dict(rocket2d=11, lander3dof=12, rocketquat=13)[w])

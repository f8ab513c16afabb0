"""Goldens of the sampled-data LQR tests (tests/test_lqr_discrete.py):
    python tests/golden/generate_lqr_discrete_goldens.py  ->  tests/golden/lqr_discrete_<model>.npz

numpy / scipy / the oracle only (tests/lqr_discrete_reference.py, tests/lqr_reference.py); nothing here touches the kernels under test.
Inputs: the trajectories, weights and dispersed starts of tests/golden/lqr_<model>.npz, read only; Qf = Q; STEPS = 5 RKF78 steps per segment.

Four matrix kinds, Phi, Gamma, P and G (the gains); every gap is relative to the largest entry of that kind along the trajectory
(lqr_discrete_reference.rel_gap).  Measured and stored per model and hold (per trajectory):
    Phi_exact, Gamma_exact, P_exact, G_exact   the tight-tolerance answer (DOP853, rtol 1e-12, restarted at every node), then the recursion
    gap_scheme_<kind>     twin vs exact: the truncation error of the scheme at STEPS
    gap_round_<kind>      the largest change of the twin's answer under N_PERTURB draws of a relative 1e-15 perturbation (random signs) of
                          every entry of A and B at every right-hand side: the rounding floor of the sweep, the conditioning of S included
                          (cond S is 1.8e10 for Rocket2D: R = diag(1e4, 1e-6))
    gap_one_step_<kind>   twin at ONE step per segment vs twin at STEPS
    wrong_row_gap_<kind>  twin with the sign of ONE tableau entry flipped (a[9][8]) vs exact
    retime_gap_<kind>     twin that re-derives the segment from t vs exact
Asserted here, with the reference alone (the tests rely on each):
    * the wrong-row twin misses the tests' bar (gap_scheme + 10 gap_round) by a factor >= 100, for every kind;
    * zero-order hold: the re-timed twin misses that bar for every kind (it reads the next segment's input at the stages with a = 1);
    * the exact P is positive definite at every node and the closed loop contracts: |prod (Phi_i - Gamma_i K_i)| < |prod Phi_i|.
The linear model against the flights (first-order hold, trajectory 0): the 2 nx + 1 starts X[0] and X[0] +- delta_j e_j flown by the numpy loop
with the latch (track_held) under the exact discrete gains; the final deviations from the centre flight against prod (Phi_i - Gamma_i K_i)
applied to the same starts.  Stored: sp_delta, sp_gap (relative to the largest predicted entry).  What the gap is made of: the latch falls up to
one plant step after the node, the flight ends up to one plant step after T, and the terms of second order in delta.
Rocket2D also stores the constant-system case: the operating point repeated over const_K nodes CONST_DT apart (the first of 51, 101, ... at
which the twin's gain at node 0 is within 1e-9 of the algebraic one).  [Phi | Gamma] of the
twin against scipy.linalg.expm of the augmented matrix, the twin's gain at node 0 against scipy.linalg.solve_discrete_are's (stage weights
Q dt, R dt), and the twin's rounding floor there, measured as above.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lqr_discrete_reference as dr  # noqa: E402
import oracle_lib  # noqa: E402

MODELS = {"rocketquat": 0, "rocket2d": 1, "lander3dof": 2}
KINDS = ("Phi", "Gamma", "P", "G")
STEPS = 5
N_PERTURB = 3
CONST_DT = 0.4


def rel_perturb(rng, size=1e-15):
    def f(A, B):
        return A * (1.0 + size * rng.choice([-1.0, 1.0], A.shape)), B * (1.0 + size * rng.choice([-1.0, 1.0], B.shape))

    return f


def kinds_of(PG, P, G, nx):
    return dict(Phi=PG[:, :, :nx], Gamma=PG[:, :, nx:], P=P, G=G)


def gaps(a, b):
    return {k: dr.rel_gap(a[k], b[k]) for k in KINDS}


def round_floor(model, par, X, U, T, q, r, steps, rng, base):
    """the largest change of the twin's answer under N_PERTURB perturbed copies"""
    nx = X.shape[1]
    worst = {k: 0.0 for k in KINDS}
    for _ in range(N_PERTURB):
        p = kinds_of(*dr.twin(model, par, X, U, T, q, r, steps=steps, perturb=rel_perturb(rng)), nx)
        for k, v in gaps(p, base).items():
            worst[k] = max(worst[k], v)
    return worst


def constant_case(par, q, r, rng):
    import scipy.linalg

    import scpp_amd

    m = scpp_amd.Rocket2D().loadParameters()
    x_eq, u_eq = (np.asarray(v, dtype=np.float64) for v in m.getOperatingPoint())
    _, A, B = oracle_lib.flow(1, x_eq, u_eq, par)
    nx, nu = B.shape
    aug = np.zeros((nx + nu, nx + nu))
    aug[:nx, :nx], aug[:nx, nx:] = A, B
    E = scipy.linalg.expm(aug * CONST_DT)
    Phi, Gam = E[:nx, :nx], E[:nx, nx:]
    Qd, Rd = np.diag(q * CONST_DT), np.diag(r * CONST_DT)
    Pd = scipy.linalg.solve_discrete_are(Phi, Gam, Qd, Rd)
    Kd = np.linalg.solve(Rd + Gam.T @ Pd @ Gam, Gam.T @ Pd @ Phi)
    for K in (51, 101, 151, 201, 301, 401):
        T = CONST_DT * (K - 1)
        X, U = np.tile(x_eq, (K, 1)), np.tile(u_eq, (K, 1))
        t = kinds_of(*dr.twin(1, par, X, U, T, q, r, steps=STEPS), nx)
        gk, gp = dr.rel_gap(t["G"][0], Kd), dr.rel_gap(t["P"][0], Pd)
        print(f"   constant system, {K} nodes {CONST_DT} s apart: twin gain at node 0 vs DARE {gk:.2e}, P {gp:.2e}")
        if gk <= 1e-9:
            break  # the horizon no longer shows; the floor, 1.6e-13 from 301 nodes on, is the conditioning of S and of the algebraic solver
    else:
        raise AssertionError("no horizon reaches 1e-9")
    fl = round_floor(1, par, X, U, T, q, r, STEPS, rng, t)
    ge_phi, ge_gam = dr.rel_gap(t["Phi"], np.tile(Phi, (K - 1, 1, 1))), dr.rel_gap(t["Gamma"], np.tile(Gam, (K - 1, 1, 1)))
    print(f"   twin vs expm: Phi {ge_phi:.2e}, Gamma {ge_gam:.2e}; rounding floor " + ", ".join(f"{k} {v:.2e}" for k, v in fl.items()))
    return dict(const_K=np.array(K), const_dt=np.array(CONST_DT), const_gap_expm_Phi=np.array(ge_phi), const_gap_expm_Gamma=np.array(ge_gam),
                const_gap_dare_G=np.array(gk), const_gap_dare_P=np.array(gp), **{f"const_round_{k}": np.array(v) for k, v in fl.items()})


def sigma_point_starts(X):
    """X[0] and X[0] +- delta_j e_j, delta_j = 1e-3 (min(0.02 max|x_j|, 5) + 0.01): small against the nominal, large against the flights' rounding"""
    nx = X.shape[1]
    delta = 1e-3 * (np.minimum(0.02 * np.abs(X).max(axis=0), 5.0) + 0.01)
    xs = np.tile(X[0], (2 * nx + 1, 1))
    for j in range(nx):
        xs[1 + 2 * j, j] += delta[j]
        xs[2 + 2 * j, j] -= delta[j]
    return xs, delta


def sigma_point_gap(x_end, xs, M):
    """(gap, largest predicted entry): final deviations from the centre flight against M applied to the starts' deviations"""
    pred = (xs[1:] - xs[0]) @ M.T
    got = x_end[1:] - x_end[0]
    return float(np.abs(got - pred).max() / np.abs(pred).max()), float(np.abs(pred).max())


def sigma_point_case(model, d, PG, G):
    par, X, U, T = d["par"], d["foh_X"][0], d["foh_U"][0], float(d["foh_t"][0])
    xs, delta = sigma_point_starts(X)
    xe = np.array([dr.track_held(model, par, X, U, G, T, x, X[-1], time_step=float(d["time_step"]))["x"] for x in xs])
    gap, scale = sigma_point_gap(xe, xs, dr.closed_loop_product(PG, G))
    print(f"   sigma points under hold = node: final deviations vs prod (Phi - Gamma K): {gap:.3e} of the largest predicted entry {scale:.3e}")
    return dict(sp_delta=delta, sp_starts=xs, sp_gap=np.array(gap))


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
        n, K, nx = X.shape
        ex = {k: [] for k in KINDS}
        g = {f"{w}_{k}": np.zeros(n) for w in ("gap_scheme", "gap_round", "gap_one_step", "wrong_row_gap", "retime_gap") for k in KINDS}
        for i in range(n):
            T = float(t[i])
            e = kinds_of(*dr.exact(model, par, X[i], U[i], T, q, r), nx)
            tw = kinds_of(*dr.twin(model, par, X[i], U[i], T, q, r, steps=STEPS), nx)
            t1 = kinds_of(*dr.twin(model, par, X[i], U[i], T, q, r, steps=1), nx)
            tx = kinds_of(*dr.twin(model, par, X[i], U[i], T, q, r, steps=STEPS, tableau=(c, a_wrong, b)), nx)
            tr = kinds_of(*dr.twin(model, par, X[i], U[i], T, q, r, steps=STEPS, retime=True), nx)
            fl = round_floor(model, par, X[i], U[i], T, q, r, STEPS, rng, tw)
            for w, v in (("gap_scheme", gaps(tw, e)), ("gap_round", fl), ("gap_one_step", gaps(t1, tw)), ("wrong_row_gap", gaps(tx, e)),
                         ("retime_gap", gaps(tr, e))):
                for k in KINDS:
                    g[f"{w}_{k}"][i] = v[k]
            for k in KINDS:
                ex[k].append(e[k])
            ev = min(np.linalg.eigvalsh(e["P"][k]).min() for k in range(K))
            PGe = np.concatenate([e["Phi"], e["Gamma"]], axis=2)
            ncl = np.linalg.norm(dr.closed_loop_product(PGe, e["G"]), 2)
            nol = np.linalg.norm(dr.closed_loop_product(PGe, np.zeros_like(e["G"])), 2)
            print(f"{name} {hold} {i}: smallest eigenvalue of P over the nodes {ev:.3e}, |prod (Phi - Gamma K)| {ncl:.3e} vs open loop {nol:.3e}")
            for w in ("gap_scheme", "gap_round", "gap_one_step", "wrong_row_gap", "retime_gap"):
                print(f"      {w:14s} " + ", ".join(f"{k} {g[f'{w}_{k}'][i]:.2e}" for k in KINDS))
            assert ev > 0.0 and ncl < nol, (name, hold, i, ev, ncl, nol)
            for k in KINDS:
                bar = g[f"gap_scheme_{k}"][i] + 10.0 * g[f"gap_round_{k}"][i]
                assert g[f"gap_round_{k}"][i] > 0.0
                assert g[f"wrong_row_gap_{k}"][i] >= 100.0 * bar, (name, hold, i, k, g[f"wrong_row_gap_{k}"][i], bar)
                if hold == "zoh":
                    assert g[f"retime_gap_{k}"][i] > bar, (name, hold, i, k, g[f"retime_gap_{k}"][i], bar)
            if hold == "foh" and i == 0:
                out.update(sigma_point_case(model, d, PGe, e["G"]))
        out.update({f"{hold}_{k}_exact": np.stack(ex[k]) for k in KINDS})
        out.update({f"{hold}_{k}": v for k, v in g.items()})
    if name == "rocket2d":
        out.update(constant_case(par, q, r, rng))
    path = os.path.join(HERE, f"lqr_discrete_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    for w in sys.argv[1:] or ["rocket2d", "lander3dof", "rocketquat"]:
        generate(w, dict(rocket2d=21, lander3dof=22, rocketquat=23)[w])

"""Goldens of the tests of the covariance sweep of the sampled-data loop (tests/test_lqr_covariance_discrete.py):
    python tests/golden/generate_lqr_covariance_discrete_goldens.py  ->  tests/golden/lqr_covariance_discrete_<model>.npz

numpy / scipy / mpmath / the oracle only (tests/lqr_covariance_discrete_reference.py and the references it builds on); nothing here touches
the kernels under test.  Inputs, all read only: the trajectories of tests/golden/lqr_<model>.npz, the exact discrete gains and transition
matrices of lqr_discrete_<model>.npz (G_exact, Phi_exact, Gamma_exact), and sigma0, w and the sigma-point step xc_eps of
lqr_covariance_<model>.npz.  (The shipped LQR.info files carry no initial_std / disturbance_std, and tests/test_lqr_covariance.py pins that;
so the covariance inputs are those the continuous sweep's tests already use.)  STEPS = 5 RKF78 steps per segment.

Three kinds, S, state_std and input_cov; every gap is relative to the largest entry of that kind along the trajectory (rel_gap).  Stored per
model and hold (per trajectory):
    S_exact (packed upper triangle), input_cov_exact    DOP853 (rtol 1e-12) for Wd, the stored exact [Phi | Gamma], then the recursion
    gap_scheme_<kind>     twin vs exact: the truncation error of the scheme at STEPS
    gap_round_<kind>      the largest change of the twin's answer under N_PERTURB draws of a relative 1e-15 perturbation (random signs) of every
                          entry of A and B at every right-hand side
    wrong_continuous_S, wrong_no_wd_S, wrong_next_gain_S    three WRONG twins vs exact, for S: the continuous-loop sweep under the same
                          gains (lqr_covariance_reference.twin), the recursion without Wd, and the recursion that closes segment i with G[i+1]
Asserted here, with the reference alone: each wrong twin misses the tests' second bar (gap_scheme + 10 gap_round) by a factor >= 100 for S.
The sigma-point flights (first-order hold, trajectory 0, W = 0): the 2 nx + 1 starts of lqr_covariance_reference.sigma_point_starts flown by
the numpy loop with the latch (lqr_discrete_reference.track_held) under the exact discrete gains; (1 / 2 eps^2) sum dx dx' of the final
deviations against the exact S_{K-1} of this sweep (sp_gap) and against the continuous sweep's exact S(T) under the same gains
(sp_gap_continuous), both relative to the largest entry of the latter matrix of the pair.
Rocket2D also stores the constant-system case: the operating point repeated over CONST_K nodes CONST_DT apart under the twin's own discrete
gains (const_G): the twin against lqr_covariance_discrete_reference.constant_system (matrix exponentials and the recursion in mpmath), and the
twin's rounding floor there.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lqr_covariance_discrete_reference as cd  # noqa: E402
import lqr_covariance_reference as cr  # noqa: E402
import lqr_discrete_reference as dr  # noqa: E402
import oracle_lib  # noqa: E402

MODELS = {"rocketquat": 0, "rocket2d": 1, "lander3dof": 2}
KINDS = ("S", "state_std", "input_cov")
STEPS = 5
N_PERTURB = 5
CONST_K, CONST_DT = 12, 0.4


def rel_perturb(rng, size=1e-15):
    def f(A, B):
        return A * (1.0 + size * rng.choice([-1.0, 1.0], A.shape)), B * (1.0 + size * rng.choice([-1.0, 1.0], B.shape))

    return f


def gaps(a, b):
    return {k: cd.rel_gap(a[k], b[k]) for k in KINDS}


def round_floor(model, par, X, U, T, G, S0, w, steps, rng, base):
    worst = {k: 0.0 for k in KINDS}
    for _ in range(N_PERTURB):
        p = cd.kinds(*cd.twin(model, par, X, U, T, G, S0, w, steps, perturb=rel_perturb(rng)))
        for k, v in gaps(p, base).items():
            worst[k] = max(worst[k], v)
    return worst


def sigma_point_case(model, d, G, S0, eps, S_end, S_end_continuous):
    par, X, U, T = d["par"], d["foh_X"][0], d["foh_U"][0], float(d["foh_t"][0])
    xs = cr.sigma_point_starts(X[0], S0, eps)
    xe = np.array([dr.track_held(model, par, X, U, G, T, x, X[-1], time_step=float(d["time_step"]))["x"] for x in xs])
    Smc = cr.sigma_point_covariance(xe, eps)
    gap, gap_c = cd.rel_gap(Smc, S_end), cd.rel_gap(Smc, S_end_continuous)
    print(f"   sigma-point flights under hold = node vs the exact S_(K-1): {gap:.3e}; vs the continuous sweep's S(T): {gap_c:.3e}")
    return dict(sp_gap=np.array(gap), sp_gap_continuous=np.array(gap_c), sp_S_exact=S_end)


def constant_case(par, q, r, S0, w, rng):
    import scpp_amd

    m = scpp_amd.Rocket2D().loadParameters()
    x_eq, u_eq = (np.asarray(v, dtype=np.float64) for v in m.getOperatingPoint())
    _, A, B = oracle_lib.flow(1, x_eq, u_eq, par)
    K, T = CONST_K, CONST_DT * (CONST_K - 1)
    X, U = np.tile(x_eq, (K, 1)), np.tile(u_eq, (K, 1))
    _, _, G = dr.twin(1, par, X, U, T, q, r, steps=STEPS)
    tw = cd.kinds(*cd.twin(1, par, X, U, T, G, S0, w, STEPS))
    ex = cd.kinds(*cd.constant_system(A, B, w, G, S0, CONST_DT, K))
    gs, fl = gaps(tw, ex), round_floor(1, par, X, U, T, G, S0, w, STEPS, rng, tw)
    print(f"   constant system, {K} nodes {CONST_DT} s apart: twin vs mpmath " + ", ".join(f"{k} {v:.2e}" for k, v in gs.items()) + "; rounding floor "
          + ", ".join(f"{k} {v:.2e}" for k, v in fl.items()))
    out = dict(const_K=np.array(K), const_dt=np.array(CONST_DT), const_G=G, const_S_exact=ex["S"], const_input_cov_exact=ex["input_cov"])
    out.update({f"const_gap_scheme_{k}": np.array(v) for k, v in gs.items()})
    out.update({f"const_gap_round_{k}": np.array(v) for k, v in fl.items()})
    return out


def generate(name, seed):
    model = MODELS[name]
    d, dg, cg = (np.load(os.path.join(HERE, f"lqr_{pre}{name}.npz")) for pre in ("", "discrete_", "covariance_"))
    par, S0, w = d["par"], cg["sigma0"], cg["w"]
    rng = np.random.default_rng(seed)
    out = dict(steps=np.array(STEPS))
    for hold in ("foh", "zoh"):
        X, U, t, Gd = d[f"{hold}_X"], d[f"{hold}_U"], d[f"{hold}_t"], dg[f"{hold}_G_exact"]
        n, K, nx = X.shape
        iu = np.triu_indices(nx)
        Se, Ie = [], []
        names = [f"gap_scheme_{k}" for k in KINDS] + [f"gap_round_{k}" for k in KINDS] + ["wrong_continuous_S", "wrong_no_wd_S", "wrong_next_gain_S"]
        g = {k: np.zeros(n) for k in names}
        for i in range(n):
            T = float(t[i])
            PGe = np.concatenate([dg[f"{hold}_Phi_exact"][i], dg[f"{hold}_Gamma_exact"][i]], axis=2)
            Wde = cd.exact_disturbances(model, par, X[i], U[i], T, w)
            e = cd.kinds(*cd.recursion(PGe, Wde, Gd[i], S0))
            tw = cd.kinds(*cd.twin(model, par, X[i], U[i], T, Gd[i], S0, w, STEPS))
            fl = round_floor(model, par, X[i], U[i], T, Gd[i], S0, w, STEPS, rng, tw)
            for k in KINDS:
                g[f"gap_scheme_{k}"][i], g[f"gap_round_{k}"][i] = cd.rel_gap(tw[k], e[k]), fl[k]
            PGt = dr.transitions(model, par, X[i], U[i], T, STEPS)
            Wdt = cd.disturbances(model, par, X[i], U[i], T, w, STEPS)
            g["wrong_continuous_S"][i] = cd.rel_gap(cr.twin(model, par, X[i], U[i], T, Gd[i], S0, w, steps=STEPS)[0], e["S"])
            g["wrong_no_wd_S"][i] = cd.rel_gap(cd.recursion(PGt, np.zeros_like(Wdt), Gd[i], S0)[0], e["S"])
            Gn = np.concatenate([Gd[i], Gd[i][-1:]])
            g["wrong_next_gain_S"][i] = cd.rel_gap(cd.recursion(PGt, Wdt, Gn, S0, gain_shift=1)[0][:K], e["S"])
            Se.append(e["S"][:, iu[0], iu[1]])
            Ie.append(e["input_cov"])
            ev = min(np.linalg.eigvalsh(e["S"][k]).min() for k in range(K))
            print(f"{name} {hold} {i}: smallest eigenvalue of S over the nodes {ev:.3e} (max |S| {np.abs(e['S']).max():.3e})")
            for k in names:
                print(f"      {k:22s} {g[k][i]:.2e}")
            bar = g["gap_scheme_S"][i] + 10.0 * g["gap_round_S"][i]
            assert all(g[f"gap_round_{k}"][i] > 0.0 for k in KINDS)
            for k in ("wrong_continuous_S", "wrong_no_wd_S", "wrong_next_gain_S"):
                assert g[k][i] >= 100.0 * bar, (name, hold, i, k, g[k][i], bar)
            if hold == "foh" and i == 0:
                e0 = cd.recursion(PGe, np.zeros_like(Wde), Gd[i], S0)[0][-1]
                c0 = cr.exact(model, par, X[i], U[i], T, Gd[i], S0, None)[0][-1]
                out.update(sigma_point_case(model, d, Gd[i], S0, float(cg["xc_eps"]), e0, c0))
        out[f"{hold}_S_exact"], out[f"{hold}_input_cov_exact"] = np.stack(Se), np.stack(Ie)
        out.update({f"{hold}_{k}": v for k, v in g.items()})
    if name == "rocket2d":
        out.update(constant_case(par, d["q"], d["r"], S0, w, rng))
    path = os.path.join(HERE, f"lqr_covariance_discrete_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    for m in sys.argv[1:] or ["rocket2d", "lander3dof", "rocketquat"]:
        generate(m, dict(rocket2d=31, lander3dof=32, rocketquat=33)[m])

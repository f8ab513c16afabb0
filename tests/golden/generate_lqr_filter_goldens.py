"""Goldens of the filter-sweep tests (tests/test_lqr_filter.py):
    python tests/golden/generate_lqr_filter_goldens.py  ->  tests/golden/lqr_filter_<model>.npz

numpy / scipy / the oracle only (tests/lqr_filter_reference.py); nothing here touches the kernels under test.  Inputs, read only: the
trajectories of tests/golden/lqr_<model>.npz with their frozen-time gains (G_ref), the finite-horizon gains of lqr_riccati_<model>.npz
(G_exact), and sigma0 and w of lqr_covariance_<model>.npz.  STEPS = 5 RKF78 steps per segment.

The measurement of the main cases is a selection (RocketQuat r, v, q: ny = 10; Rocket2D states 0, 1, 4; Lander3dof states 1..3) with
v_m = 8 h (H sigma0 H')_mm, h = the largest dt of the model's trajectories / STEPS: h rho = 1/8 at 5 steps, the front ends' step rule.
Stored per model: H, v.  Per case (hold, gain law, w1: W = diag(w); one w0 case, foh / riccati, W = 0) and trajectory:
    Sg_exact, Xh_exact, I_exact   the tight-tolerance answer (DOP853, rtol 1e-12, restarted at every node): packed upper triangles, G Xh G'
    gap_scheme_{Sg,Xh,L,I,sd}     twin vs exact.  Sg, Xh, I in units of the two states' (inputs') largest standard deviation along the
                                  trajectory (scaled_gap; Xh in the units of Sg + Xh); L[j][m] in units d_j dy_m / v_m, dy_m^2 = the largest
                                  (H Sg H')_mm; sd = sqrt diag (Sg + Xh) relative to each state's largest
    gap_round_{...}               twin vs a copy of itself whose Jacobians are perturbed by 1 ulp at every right-hand side; the copy's L and
                                  G Xh G' are formed with H and G perturbed by 1 ulp as well (as the covariance generator treats G S G')
    wrong_sign_gap                Sg of a twin with the sign of ONE tableau entry flipped (a[9][8]) vs exact
    joint_gap                     Cov(e) of the 2 nx x 2 nx joint system of (e, eps) (joint_exact) vs Sg + Xh of exact, relative to its largest entry
Asserted here, with the reference alone (the tests rely on each):
    * gap_scheme <= 1e-10 on every case and quantity;
    * the wrong-sign twin misses the tests' exact bar on Sg (gap_scheme + 10 gap_round) by a factor >= 100;
    * joint_gap <= 1e-9.
Further measurements (first-order hold, Riccati gains, W = diag(w)), gap_round only -- the tests hold these against the twin:
    lander3dof   dense: a fixed-seed random 5 x 7 H;   rocket2d   ny1 (state 1), nyI (H = I), ny16 (16 rows over 6 states, repeated rows
    with different v);  v by the same rule.
Rocket2D also stores the stationary case: a constant two-node system at the operating point, the main H and v, W = diag(w): the horizon
and step count (40 steps per second) at which the twin's Sg(T) is within 1e-8 of scipy.linalg.solve_continuous_are(A', H', W, V).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lqr_filter_reference as fr  # noqa: E402
import oracle_lib  # noqa: E402

MODELS = {"rocketquat": 0, "rocket2d": 1, "lander3dof": 2}
MEASURED = {"rocketquat": list(range(1, 11)), "rocket2d": [0, 1, 4], "lander3dof": [1, 2, 3]}
STEPS = 5
CASES, QUANTITIES = fr.CASES, fr.QUANTITIES


def noise_for(H, S0, h):
    """v_m = 8 h (H sigma0 H')_mm"""
    return 8.0 * h * np.einsum("mi,ij,mj->m", H, S0, H)


def stationary_case(par, S0, w, H, v):
    import scipy.linalg

    import scpp_amd

    m = scpp_amd.Rocket2D().loadParameters()
    x_eq, u_eq = (np.asarray(a, dtype=np.float64) for a in m.getOperatingPoint())
    _, A, _ = oracle_lib.flow(1, x_eq, u_eq, par)
    Sa = scipy.linalg.solve_continuous_are(A.T, H.T, np.diag(w), np.diag(v))
    X, U = np.tile(x_eq, (2, 1)), np.tile(u_eq, (2, 1))
    for T in (10.0, 20.0, 40.0, 80.0, 160.0, 320.0):
        steps = int(40 * T)
        t = fr.twin(1, par, X, U, T, None, S0, w, H, v, steps=steps)
        gap = fr.rel_gap(t["Sg"][1], Sa)
        print(f"   stationary case, horizon {T:5.1f} s, {steps} steps: twin Sg(T) vs the algebraic Riccati solution {gap:.2e}")
        if gap <= 1e-8:
            break
    else:
        raise AssertionError("no horizon reaches 1e-8")
    return dict(stat_horizon=np.array(T), stat_steps=np.array(steps), stat_gap=np.array(gap))


def extra_measurements(name, nx, rng):
    if name == "lander3dof":
        return {"dense": rng.standard_normal((5, 7))}
    if name == "rocket2d":
        H16 = np.concatenate([np.eye(6), np.eye(6), rng.standard_normal((4, 6))])
        return {"ny1": fr.selection(6, [1]), "nyI": np.eye(6), "ny16": H16}
    return {}


def generate(name, seed):
    model = MODELS[name]
    d, g, cg = (np.load(os.path.join(HERE, f"lqr_{pre}{name}.npz")) for pre in ("", "riccati_", "covariance_"))
    par, S0, w = d["par"], cg["sigma0"], cg["w"]
    rng = np.random.default_rng(seed)
    nx = S0.shape[0]
    iu = np.triu_indices(nx)
    c, a, b = oracle_lib.rkf78_tableau()
    a_wrong = a.copy()
    assert a_wrong[9, 8] != 0.0
    a_wrong[9, 8] = -a_wrong[9, 8]
    h = max(float(d[f"{hold}_t"].max()) / (d[f"{hold}_X"].shape[1] - 1) for hold in ("foh", "zoh")) / STEPS
    H = fr.selection(nx, MEASURED[name])
    v = noise_for(H, S0, h)
    assert fr.auto_steps(S0, H, v, h * STEPS)[0] == STEPS
    out = dict(steps=np.array(STEPS), H=H, v=v)
    print(f"{name}: measured states {MEASURED[name]}, v {v}, h {h:.4f}, rho {fr.auto_steps(S0, H, v, h * STEPS)[1]:.3f}")
    for hold, law, wc in CASES:
        X, U, t = d[f"{hold}_X"], d[f"{hold}_U"], d[f"{hold}_t"]
        G = d[f"{hold}_G_ref"] if law == "frozen" else g[f"{hold}_G_exact"]
        wv = w if wc == "w1" else None
        tag = f"{hold}_{law}_{wc}"
        n, K = X.shape[0], X.shape[1]
        ex = {k: [] for k in ("Sg", "Xh", "I")}
        m = {f"gap_{kind}_{q}": np.zeros(n) for kind in ("scheme", "round") for q in QUANTITIES}
        m.update(wrong_sign_gap=np.zeros(n), joint_gap=np.zeros(n))
        for i in range(n):
            args = (model, par, X[i], U[i], float(t[i]), G[i], S0, wv, H, v)
            e = fr.exact(*args)
            tw = fr.twin(*args, steps=STEPS)
            tp = fr.perturbed_twin(*args, STEPS, rng)
            tws = fr.twin(*args, steps=STEPS, tableau=(c, a_wrong, b))
            J = fr.joint_exact(*args)
            for q, val in fr.gaps(tw, e, H, v).items():
                m[f"gap_scheme_{q}"][i] = val
            for q, val in fr.gaps(tp, tw, H, v).items():
                m[f"gap_round_{q}"][i] = val
            m["wrong_sign_gap"][i] = fr.scaled_gap(tws["Sg"], e["Sg"])
            m["joint_gap"][i] = fr.rel_gap(J, e["Sg"] + e["Xh"])
            for k in ex:
                ex[k].append(e[k])
            print(f"{name} {tag} {i}: max|Sg| {np.abs(e['Sg']).max():.3e} max|Xh| {np.abs(e['Xh']).max():.3e} max|L| {np.abs(e['L']).max():.3e}; "
                  + ", ".join(f"{k} {val[i]:.2e}" for k, val in m.items()))
            assert all(m[f"gap_scheme_{q}"][i] <= 1e-10 for q in QUANTITIES), (name, tag, i)
            assert all(m[f"gap_round_{q}"][i] > 0.0 for q in QUANTITIES), (name, tag, i)
            assert m["wrong_sign_gap"][i] >= 100.0 * (m["gap_scheme_Sg"][i] + 10.0 * m["gap_round_Sg"][i]), (name, tag, i)
            assert m["joint_gap"][i] <= 1e-9, (name, tag, i)
        out.update({f"{tag}_Sg_exact": np.array(ex["Sg"])[:, :, iu[0], iu[1]], f"{tag}_Xh_exact": np.array(ex["Xh"])[:, :, iu[0], iu[1]],
                    f"{tag}_I_exact": np.array(ex["I"])})
        out.update({f"{tag}_{k}": val for k, val in m.items()})
    X, U, t, G = d["foh_X"], d["foh_U"], d["foh_t"], g["foh_G_exact"]
    for key, He in extra_measurements(name, nx, rng).items():
        ve = noise_for(He, S0, h)
        if key == "ny16":
            ve[6:12] *= 3.0  # the repeated rows carry a different v
        m = {f"{key}_gap_round_{q}": np.zeros(X.shape[0]) for q in QUANTITIES}
        for i in range(X.shape[0]):
            args = (model, par, X[i], U[i], float(t[i]), G[i], S0, w, He, ve)
            for q, val in fr.gaps(fr.perturbed_twin(*args, STEPS, rng), fr.twin(*args, steps=STEPS), He, ve).items():
                assert val > 0.0
                m[f"{key}_gap_round_{q}"][i] = val
            print(f"{name} {key} {i}: " + ", ".join(f"{k} {val[i]:.2e}" for k, val in m.items()))
        out.update(m)
        out.update({f"{key}_H": He, f"{key}_v": ve})
    if name == "rocket2d":
        out.update(stationary_case(par, S0, w, H, v))
    path = os.path.join(HERE, f"lqr_filter_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    for which in sys.argv[1:] or ["rocket2d", "lander3dof", "rocketquat"]:
        generate(which, dict(rocket2d=31, lander3dof=32, rocketquat=33)[which])

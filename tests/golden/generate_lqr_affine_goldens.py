"""Goldens of the affine finite-horizon LQR tests (tests/test_lqr_affine.py):
    python tests/golden/generate_lqr_affine_goldens.py  ->  tests/golden/lqr_affine_<model>.npz

numpy / scipy / the oracle only (tests/lqr_affine_reference.py); nothing here touches the kernels under test.  Inputs: the trajectories and
weights of tests/golden/lqr_<model>.npz, read only; Qf = Q; STEPS = 5 RKF78 steps per segment.

Two kinds of nominal per model and hold:
    plain   the dynamically exact nominals of lqr_<model>.npz.  Their defect c is what linear interpolation between the nodes leaves: small,
            and made of cancellation.
    bent    the same nodes moved by a smooth profile that is consistent in itself: positions by A sin^2(pi tau) d, velocities by its time
            derivative A (pi / T) sin(2 pi tau) d, tau = k / (K - 1), d = (1, -0.6, 0.3) cut to the model's position dimension; masses, angles,
            rates and the (unit) quaternions stay.  The bend vanishes with zero slope at both ends.  The plant cannot follow it without an
            acceleration the nominal inputs do not hold: integrated over a segment the bent nominal misses its own next node in velocity by up
            to 10 m/s (RocketQuat, Lander3dof: A = 300 m) and 2.8 m/s (Rocket2D, A = 50 m), the order README.md reports for solver output.

Measured and stored per kind, hold and trajectory, for each of P, K, p, k, s (relative to the largest magnitude of that array over the trajectory):
    gap_scheme_*   twin vs exact: the truncation error of the scheme at STEPS
    gap_round_*    twin vs a copy whose Jacobian AND flow-map values are perturbed by 1 ulp at every right-hand side: the rounding floor
    *_exact        the tight-tolerance answer (DOP853, rtol 1e-12, restarted at every node)
Bent only:
    wrong_row_gap_p   twin with the sign of ONE tableau entry flipped (a[9][8]) vs exact, for p
    J_ff, J_noff, s0  the cost (lqr_affine_reference.cost) of the twin loop flown from x_start = X[0] to the end under the twin's gains, with and
                      without the feedforward term, and the predicted cost-to-go s(t_0)
Asserted here, with the reference alone (the tests rely on each):
    * every gap_round is > 0; the wrong-row twin misses the tests' bar for p (gap_scheme_p + 10 gap_round_p) by a factor >= 100 on every bent input;
    * J_ff <= 0.5 J_noff for every bent case.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lqr_affine_reference as ar  # noqa: E402
import oracle_lib  # noqa: E402

MODELS = {"rocketquat": 0, "rocket2d": 1, "lander3dof": 2}
STEPS = 5
# (position columns, velocity columns, amplitude in metres)
BEND = {"rocket2d": ((0, 1), (2, 3), 50.0), "lander3dof": ((1, 2, 3), (4, 5, 6), 300.0), "rocketquat": ((1, 2, 3), (4, 5, 6), 300.0)}
FIELDS = ("P", "K", "p", "k", "s")


def bend(name, X, T):
    ri, vi, amp = BEND[name]
    K = X.shape[0]
    tau = np.arange(K) / (K - 1)
    d = np.array([1.0, -0.6, 0.3])[:len(ri)]
    Xb = X.copy()
    Xb[:, ri] += amp * (np.sin(np.pi * tau) ** 2)[:, None] * d
    Xb[:, vi] += amp * (np.pi / T) * np.sin(2.0 * np.pi * tau)[:, None] * d
    return Xb


def gap(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


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
        n = X.shape[0]
        Xb = np.stack([bend(name, X[i], float(t[i])) for i in range(n)])
        out[f"{hold}_Xbent"] = Xb
        for kind, Xk in (("plain", X), ("bent", Xb)):
            g = {f"gap_{w}_{f}": np.zeros(n) for w in ("scheme", "round") for f in FIELDS}
            ex = {f: [] for f in FIELDS}
            wrong, J_ff, J_noff, s0 = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
            for i in range(n):
                T = float(t[i])
                e = ar.exact(model, par, Xk[i], U[i], T, q, r)
                tw = ar.twin(model, par, Xk[i], U[i], T, q, r, steps=STEPS)
                tp = ar.twin(model, par, Xk[i], U[i], T, q, r, steps=STEPS, perturb=ar.ulp_perturb(rng))
                for f in FIELDS:
                    g[f"gap_scheme_{f}"][i], g[f"gap_round_{f}"][i] = gap(tw[f], e[f]), gap(tp[f], tw[f])
                    assert g[f"gap_round_{f}"][i] > 0.0, (name, hold, kind, i, f)
                    ex[f].append(e[f])
                line = f"{name} {hold} {kind} {i}: max|p| {np.abs(e['p']).max():.3e} max|k| {np.abs(e['k']).max():.3e} s0 {e['s'][0]:.3e}; " + ", ".join(
                    f"{f} scheme {g[f'gap_scheme_{f}'][i]:.1e} round {g[f'gap_round_{f}'][i]:.1e}" for f in FIELDS)
                if kind == "bent":
                    tww = ar.twin(model, par, Xk[i], U[i], T, q, r, steps=STEPS, tableau=(c, a_wrong, b))
                    wrong[i] = gap(tww["p"], e["p"])
                    bar = g["gap_scheme_p"][i] + 10.0 * g["gap_round_p"][i]
                    assert wrong[i] >= 100.0 * bar, (name, hold, i, wrong[i], bar)
                    fl = [ar.track(model, par, Xk[i], U[i], tw["K"], ff, T, Xk[i, 0], Xk[i, -1], time_step=float(d["time_step"])) for ff in (tw["k"], None)]
                    J_ff[i], J_noff[i] = (ar.cost(Xk[i], U[i], T, q, r, q, Xk[i, 0], f_["rec_x"], f_["rec_u"], float(d["time_step"])) for f_ in fl)
                    s0[i] = tw["s"][0]
                    line += f"; wrong row p {wrong[i]:.1e}; J_ff {J_ff[i]:.4e} J_noff {J_noff[i]:.4e} (ratio {J_ff[i] / J_noff[i]:.3f}) s0 {s0[i]:.4e}"
                    assert J_ff[i] <= 0.5 * J_noff[i], (name, hold, i, J_ff[i], J_noff[i])
                print(line, flush=True)
            out.update({f"{hold}_{kind}_{k}": v for k, v in g.items()})
            for f in FIELDS:
                out[f"{hold}_{kind}_{f}_exact"] = np.stack(ex[f])
            if kind == "bent":
                out.update({f"{hold}_wrong_row_gap_p": wrong, f"{hold}_J_ff": J_ff, f"{hold}_J_noff": J_noff, f"{hold}_s0": s0})
    path = os.path.join(HERE, f"lqr_affine_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    for w in sys.argv[1:] or ["rocket2d", "lander3dof", "rocketquat"]:
        generate(w, dict(rocket2d=21, lander3dof=22, rocketquat=23)[w])

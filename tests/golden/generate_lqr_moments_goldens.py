"""Goldens of the closed-loop mean tests (tests/test_lqr_moments.py):
    python tests/golden/generate_lqr_moments_goldens.py  ->  tests/golden/lqr_moments_<model>.npz

numpy / scipy / the oracle only (tests/lqr_moments_reference.py); nothing here touches the kernels under test.  Inputs, read only:
tests/golden/lqr_<model>.npz (nominals, inputs, parameters), lqr_affine_<model>.npz (the bent nominals; *_K_exact and *_k_exact are the gains
and feedforward terms of every sweep here, so the mean is tested without the affine kernel) and lqr_covariance_<model>.npz (sigma0, w, used by
the tests).  STEPS = the affine goldens' 5 RKF78 steps per segment; mean0 = 0.

Stored per kind (plain, bent), hold, trajectory and feedforward setting (ff0: d = c, ff1: d = c - B k_t):
    mean_exact     the tight-tolerance m (DOP853, rtol 1e-12, restarted at every node)
    gap_scheme_m   twin vs exact: the truncation error of the scheme at STEPS
    gap_round_m    twin vs a copy whose flow-map AND Jacobian values are perturbed by 1 ulp at every right-hand side: the rounding floor
    gap_scheme_u, gap_round_u   the same two for du_mean = -G m - [ff]
each relative to the largest magnitude of the array over the trajectory (on plain nominals m is made of cancellation, as p is).
Plain only, per hold and trajectory: outer_gap, the identity S_k = dm_k dm_k' (S(0) = v v', W = 0, dm = m(v) - m(0), v = probe_mean(sigma0)) as
the two TWINS meet it (lqr_covariance_reference.twin against lqr_moments_reference.twin), relative to max|S|: the rounding of the identity
itself, which the bar of the structure test adds to the covariance sweep's own.
Bent only: wrong_row_gap_m, the twin with the sign of ONE tableau entry flipped (a[9][8]) vs exact.
The flight test, per hold and feedforward setting, trajectory 0: the nominal is X0 + s (Xbent - X0), the gains and terms are blended in the same way,
s = flight_scale (1 % of the bend); flight_gap = max_k |(x(t_k) - X[k]) - m_k| / max|m| of the reference flight (lqr_moments_reference.flight, plant
step dt / ceil(dt / 0.01)) against the exact mean of that loop.
Asserted here, with the reference alone (the tests rely on each):
    * every gap_round is > 0; the wrong-row twin misses the tests' bar for m (gap_scheme_m + 10 gap_round_m) by a factor >= 100 on every bent input;
    * every flight_gap is <= 0.15 (the mean predicts the flight); a model that misses it gets a smaller flight_scale, never a larger cap.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lqr_covariance_reference as cr  # noqa: E402
import lqr_moments_reference as mr  # noqa: E402
import oracle_lib  # noqa: E402

MODELS = {"rocketquat": 0, "rocket2d": 1, "lander3dof": 2}
FLIGHT_SCALE = {"rocketquat": 0.01, "rocket2d": 0.01, "lander3dof": 0.01}
FLIGHT_CAP = 0.15


def generate(name, seed):
    model = MODELS[name]
    d = np.load(os.path.join(HERE, f"lqr_{name}.npz"))
    ag = np.load(os.path.join(HERE, f"lqr_affine_{name}.npz"))
    par = d["par"]
    steps = int(ag["steps"])
    rng = np.random.default_rng(seed)
    c, a, b = oracle_lib.rkf78_tableau()
    a_wrong = a.copy()
    assert a_wrong[9, 8] != 0.0
    a_wrong[9, 8] = -a_wrong[9, 8]
    out = dict(steps=np.array(steps), flight_scale=np.array(FLIGHT_SCALE[name]))
    for hold in ("foh", "zoh"):
        X0, U, t = d[f"{hold}_X"], d[f"{hold}_U"], d[f"{hold}_t"]
        n = X0.shape[0]
        for kind, Xk in (("plain", X0), ("bent", ag[f"{hold}_Xbent"])):
            G, kff = ag[f"{hold}_{kind}_K_exact"], ag[f"{hold}_{kind}_k_exact"]
            for fi in (0, 1):
                key = f"{hold}_{kind}_ff{fi}"
                g = {f"gap_{w}_{f}": np.zeros(n) for w in ("scheme", "round") for f in ("m", "u")}
                ex, wrong = [], np.zeros(n)
                for i in range(n):
                    T, ff = float(t[i]), (kff[i] if fi else None)
                    e = mr.exact(model, par, Xk[i], U[i], T, G[i], ff)
                    tw = mr.twin(model, par, Xk[i], U[i], T, G[i], ff, steps=steps)
                    tp = mr.twin(model, par, Xk[i], U[i], T, G[i], ff, steps=steps, perturb=mr.ulp_perturb(rng))
                    for q, f in enumerate(("m", "u")):
                        g[f"gap_scheme_{f}"][i], g[f"gap_round_{f}"][i] = mr.rel_gap(tw[q], e[q]), mr.rel_gap(tp[q], tw[q])
                        assert g[f"gap_round_{f}"][i] > 0.0, (name, key, i, f)
                    ex.append(e[0])
                    line = f"{name} {key} {i}: max|m| {np.abs(e[0]).max():.3e} |m(T)| {np.linalg.norm(e[0][-1]):.3e} max|du| {np.abs(e[1]).max():.3e}; " + ", ".join(
                        f"{f} scheme {g[f'gap_scheme_{f}'][i]:.1e} round {g[f'gap_round_{f}'][i]:.1e}" for f in ("m", "u"))
                    if kind == "bent":
                        tww = mr.twin(model, par, Xk[i], U[i], T, G[i], ff, steps=steps, tableau=(c, a_wrong, b))
                        wrong[i] = mr.rel_gap(tww[0], e[0])
                        bar = g["gap_scheme_m"][i] + 10.0 * g["gap_round_m"][i]
                        assert wrong[i] >= 100.0 * bar, (name, key, i, wrong[i], bar)
                        line += f"; wrong row m {wrong[i]:.1e}"
                    print(line, flush=True)
                out.update({f"{key}_{k}": v for k, v in g.items()})
                out[f"{key}_mean_exact"] = np.stack(ex)
                if kind == "bent":
                    out[f"{key}_wrong_row_gap_m"] = wrong
        v = mr.probe_mean(np.load(os.path.join(HERE, f"lqr_covariance_{name}.npz"))["sigma0"])
        og = np.zeros(n)
        for i in range(n):
            G, T = ag[f"{hold}_plain_K_exact"][i], float(t[i])
            S, _ = cr.twin(model, par, X0[i], U[i], T, G, np.outer(v, v), steps=steps)
            og[i] = mr.outer_gap(S, mr.twin(model, par, X0[i], U[i], T, G, None, v, steps=steps)[0], mr.twin(model, par, X0[i], U[i], T, G, steps=steps)[0])
            print(f"{name} {hold} plain {i}: outer-product identity between the twins {og[i]:.2e}", flush=True)
        out[f"{hold}_plain_outer_gap"] = og
        # the flight test: trajectory 0, the nominal, gains and terms at FLIGHT_SCALE of the way from plain to bent
        s, T = FLIGHT_SCALE[name], float(t[0])
        Xs = mr.blend(X0[0], ag[f"{hold}_Xbent"][0], s)
        Gs = mr.blend(ag[f"{hold}_plain_K_exact"][0], ag[f"{hold}_bent_K_exact"][0], s)
        ks = mr.blend(ag[f"{hold}_plain_k_exact"][0], ag[f"{hold}_bent_k_exact"][0], s)
        for fi in (0, 1):
            ff = ks if fi else None
            m, _ = mr.exact(model, par, Xs, U[0], T, Gs, ff)
            dev = mr.flight(model, par, Xs, U[0], T, Gs, ff)
            gap = float(np.abs(dev - m).max() / np.abs(m).max())
            print(f"{name} {hold} flight ff{fi}: scale {s}, max|m| {np.abs(m).max():.3e}, max|x - X| {np.abs(dev).max():.3e}, gap {gap:.3e}", flush=True)
            assert gap <= FLIGHT_CAP, (name, hold, fi, gap)
            out[f"{hold}_ff{fi}_flight_gap"] = np.array(gap)
    path = os.path.join(HERE, f"lqr_moments_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    for w in sys.argv[1:] or ["rocket2d", "lander3dof", "rocketquat"]:
        generate(w, dict(rocket2d=31, lander3dof=32, rocketquat=33)[w])

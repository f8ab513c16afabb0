"""Sampled-data LQR (scpp_hip_lqr_compute_gains_discrete, scpp_amd/csrc/lqr/lqr_discrete_kernel.h) and the node-rate feedback hold of the
tracking loop (scpp_hip_lqr_set_feedback_hold): every test runs the SAME assertions on the CPU emulation of the kernel sources (`emu`) and,
marked gpu, on the device library (`hip`).

Checkers (tests/lqr_discrete_reference.py, no code shared with the kernels): the exact answer (DOP853, rtol 1e-12, stored by
tests/golden/generate_lqr_discrete_goldens.py), the twin (numpy fixed-step RKF78 of the same definition on the oracle's Jacobians, then the
recursion as the header writes it; run here, once per case and shared) and track_held (the numpy tracking loop with the latch).
Inputs: tests/golden/lqr_<model>.npz (trajectories, weights, dispersed starts; read only) and tests/golden/lqr_discrete_<model>.npz.

Bars: device vs twin 10 x gap_round (the largest change of the twin under relative 1e-15 perturbations of every A and B; the factor 10 covers
fused multiply-add placement and the summation order of the tile products); device vs exact gap_scheme + that.  Per matrix kind (Phi, Gamma,
P, gains), relative to the largest entry of that kind along the trajectory, all measured by the generator with the reference alone."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import lqr_discrete_reference as dr
import lqr_saturation_reference as sr

MODELS = {"rocketquat": 0, "rocket2d": 1, "lander3dof": 2}
CASES = [("rocketquat", "foh"), ("rocketquat", "zoh"), ("rocket2d", "foh"), ("rocket2d", "zoh"), ("lander3dof", "foh"), ("lander3dof", "zoh")]
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
KINDS = ("Phi", "Gamma", "P", "G")


@pytest.fixture(scope="module", params=BACKENDS)
def backend(request):
    """(name, LQR library, solver library builder) of the emulation build or of the device build"""
    import __graft_entry__ as g

    g.build_oracle()
    if request.param == "emu":
        return "emu", g.build_lqr_emu(), g.build_emu

    def solver():
        alt = os.environ.get("SCPP_HIP_LIBRARY")
        return alt if alt else (g.HIP_LIB if os.path.exists(g.HIP_LIB) else g.build_hip())

    lib = os.environ.get("SCPP_LQR_LIBRARY") or g.LQR_LIB
    if not os.path.exists(lib):
        g.build_lqr()
    return "hip", lib, solver


@pytest.fixture(scope="module")
def lqr_lib(backend):
    return backend[1]


def golden(name):
    return np.load(os.path.join(GOLDEN, f"lqr_{name}.npz"))


def dgolden(name):
    return np.load(os.path.join(GOLDEN, f"lqr_discrete_{name}.npz"))


def context(lib, name, d, hold, B=None):
    from scpp_amd import _lib

    X, U, t = d[f"{hold}_X"], d[f"{hold}_U"], d[f"{hold}_t"]
    c = _lib.LqrContext(MODELS[name], X.shape[1], X.shape[0] if B is None else B, hold == "foh", 0, lib)
    c.set_weights(d["q"], d["r"])
    c.set_flow_params(d["par"])
    if B is None:
        c.set_trajectories(X, U, t)
    return c


def sweep(lib, name, d, hold, steps, qf=None):
    """n_ok and the four kinds (+ status, iters) of the device's sweep over the golden batch"""
    c = context(lib, name, d, hold)
    if qf is not None:
        c.set_terminal_weights(qf)
    n_ok = c.compute_gains_discrete(steps, True)
    o = c.download_gains()
    o.update(c.download_discrete())
    o["G"] = o["gains"]
    c.close()
    return n_ok, o


@functools.lru_cache(maxsize=None)
def twin_of(name, hold, b, steps=5):
    """the twin of trajectory b, computed once and shared (read only)"""
    import __graft_entry__ as g

    g.build_oracle()
    d = golden(name)
    X, U, t = d[f"{hold}_X"], d[f"{hold}_U"], d[f"{hold}_t"]
    PG, P, G = dr.twin(MODELS[name], d["par"], X[b], U[b], float(t[b]), d["q"], d["r"], steps=steps)
    nx = X.shape[2]
    out = dict(Phi=PG[:, :, :nx], Gamma=PG[:, :, nx:], P=P, G=G)
    for v in out.values():
        v.setflags(write=False)
    return out


def same(a, b):
    return a.shape == b.shape and (a == b).all()


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hold", CASES)
def test_transitions_p_and_gains_against_twin_and_exact(lqr_lib, name, hold):
    """Phi, Gamma of every segment and P, K of every node vs the twin (bar 10 x gap_round) and vs the exact answer (bar gap_scheme + that);
    status 0 everywhere, n_ok = B K, the count of node k is (K-1-k) steps.  The generator asserts that a twin with ONE tableau entry's sign
    flipped misses the second bar by a factor >= 100 for every kind, and that a twin that re-derives the segment from the time misses it
    under zero-order hold."""
    d, g = golden(name), dgolden(name)
    steps = int(g["steps"])
    B, K = d[f"{hold}_X"].shape[:2]
    n_ok, o = sweep(lqr_lib, name, d, hold, steps)
    assert all(np.isfinite(o[k]).all() for k in KINDS)
    for b in range(B):
        tw = twin_of(name, hold, b)
        for k in KINDS:
            bar_t = 10.0 * float(g[f"{hold}_gap_round_{k}"][b])
            bar_e = float(g[f"{hold}_gap_scheme_{k}"][b]) + bar_t
            gt, ge = dr.rel_gap(o[k][b], tw[k]), dr.rel_gap(o[k][b], g[f"{hold}_{k}_exact"][b])
            print(f"{name} {hold} {b} {k:5s}: vs twin {gt:.2e} (bar {bar_t:.2e}), vs exact {ge:.2e} (bar {bar_e:.2e}); wrong-row twin "
                  f"{float(g[f'{hold}_wrong_row_gap_{k}'][b]):.2e}, re-timed twin {float(g[f'{hold}_retime_gap_{k}'][b]):.2e}")
            assert gt <= bar_t, (k, gt, bar_t)
            assert ge <= bar_e, (k, ge, bar_e)
            assert float(g[f"{hold}_wrong_row_gap_{k}"][b]) >= 100.0 * bar_e
            if hold == "zoh":
                assert float(g[f"{hold}_retime_gap_{k}"][b]) > bar_e
    assert (o["status"] == 0).all() and n_ok == B * K
    assert (o["iters"] == (K - 1 - np.arange(K)) * steps).all()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hold", CASES)
def test_structure(lqr_lib, name, hold):
    """P symmetric TO THE BIT and positive definite at every node; P[K-1] == diag(Qf) and G[K-1] == G[K-2] bitwise; a Qf that is not Q changes
    P and the gains at every node (and leaves Phi and Gamma bitwise alone); one step per segment agrees with five within gap_one_step, the
    twin's own gap between the two, plus 20 x gap_round: each of the two device results is within 10 x gap_round of its twin (case 1's bar)."""
    d, g = golden(name), dgolden(name)
    steps = int(g["steps"])
    X, U, t = d[f"{hold}_X"], d[f"{hold}_U"], d[f"{hold}_t"]
    B, K = X.shape[:2]
    _, o = sweep(lqr_lib, name, d, hold, steps)
    P = o["P"]
    for b in range(B):
        ev = min(np.linalg.eigvalsh(P[b, k]).min() for k in range(K))
        print(f"{name} {hold} {b}: smallest eigenvalue of P over the nodes {ev:.3e}")
        assert same(P[b], P[b].transpose(0, 2, 1))
        assert ev > 0.0
        assert same(P[b, K - 1], np.diag(d["q"]))
        assert same(o["G"][b, K - 1], o["G"][b, K - 2]) and np.abs(o["G"][b, K - 1]).max() > 0
    qf = d["q"] * (2.0 + np.arange(d["q"].size))
    _, o2 = sweep(lqr_lib, name, d, hold, steps, qf=qf)
    for b in range(B):
        assert same(o2["P"][b, K - 1], np.diag(qf)) and same(o2["P"][b], o2["P"][b].transpose(0, 2, 1))
        assert same(o2["Phi"][b], o["Phi"][b]) and same(o2["Gamma"][b], o["Gamma"][b])  # the transitions do not know the weights
        ch = [dr.rel_gap(o2[k][b][:K - 1], o[k][b][:K - 1]) for k in ("P", "G")]
        print(f"{name} {hold} {b}: another Qf moves P by {ch[0]:.2e} of its largest entry, the gains by {ch[1]:.2e}")
        assert all((o2["P"][b, k] != P[b, k]).any() and (o2["G"][b, k] != o["G"][b, k]).any() for k in range(K - 1))
    n1, o1 = sweep(lqr_lib, name, d, hold, 1)
    assert n1 == B * K and (o1["iters"] == (K - 1 - np.arange(K))).all()
    for b in range(B):
        for k in KINDS:
            gap = dr.rel_gap(o1[k][b], o[k][b])
            bar = float(g[f"{hold}_gap_one_step_{k}"][b]) + 20.0 * float(g[f"{hold}_gap_round_{k}"][b])
            print(f"{name} {hold} {b} {k:5s}: one step vs {steps} steps per segment {gap:.2e} (bar {bar:.2e}, twin {float(g[f'{hold}_gap_one_step_{k}'][b]):.2e})")
            assert gap <= bar, (k, gap, bar)


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------
def test_constant_system_against_expm_and_the_algebraic_solution(lqr_lib):
    """Rocket2D's operating point repeated over const_K nodes const_dt apart (from the generator: the first horizon at which the twin's gain
    at node 0 is within 1e-9 of the algebraic one).  Every Phi_i, Gamma_i vs scipy.linalg.expm of the augmented matrix [[A, B], [0, 0]] dt:
    bar = the twin's gap to expm + 10 x the twin's rounding floor there.  The gain at node 0 vs scipy.linalg.solve_discrete_are's (stage
    weights Q dt, R dt): bar = the twin's gap + 10 x its floor; cond S = 1.8e10 here (R = diag(1e4, 1e-6)) and is inside both figures."""
    import scipy.linalg

    import oracle_lib
    import scpp_amd
    from scpp_amd import _lib

    d, g = golden("rocket2d"), dgolden("rocket2d")
    K, dt, steps = int(g["const_K"]), float(g["const_dt"]), int(g["steps"])
    m = scpp_amd.Rocket2D().loadParameters()
    x_eq, u_eq = (np.asarray(v, dtype=np.float64) for v in m.getOperatingPoint())
    c = _lib.LqrContext(1, K, 1, True, 0, lqr_lib)
    c.set_weights(d["q"], d["r"])
    c.set_flow_params(d["par"])
    c.set_trajectories(np.tile(x_eq, (1, K, 1)), np.tile(u_eq, (1, K, 1)), [dt * (K - 1)])
    assert c.compute_gains_discrete(steps, True) == K
    o, D = c.download_gains(), c.download_discrete()
    c.close()
    _, A, Bm = oracle_lib.flow(1, x_eq, u_eq, d["par"])
    nx, nu = Bm.shape
    aug = np.zeros((nx + nu, nx + nu))
    aug[:nx, :nx], aug[:nx, nx:] = A, Bm
    E = scipy.linalg.expm(aug * dt)
    Phi, Gam = E[:nx, :nx], E[:nx, nx:]
    Rd = np.diag(d["r"] * dt)
    Pd = scipy.linalg.solve_discrete_are(Phi, Gam, np.diag(d["q"] * dt), Rd)
    Kd = np.linalg.solve(Rd + Gam.T @ Pd @ Gam, Gam.T @ Pd @ Phi)
    gphi, ggam = dr.rel_gap(D["Phi"][0], np.tile(Phi, (K - 1, 1, 1))), dr.rel_gap(D["Gamma"][0], np.tile(Gam, (K - 1, 1, 1)))
    bphi = float(g["const_gap_expm_Phi"]) + 10.0 * float(g["const_round_Phi"])
    bgam = float(g["const_gap_expm_Gamma"]) + 10.0 * float(g["const_round_Gamma"])
    gk = dr.rel_gap(o["gains"][0, 0], Kd)
    bk = float(g["const_gap_dare_G"]) + 10.0 * float(g["const_round_G"])
    print(f"constant system, {K} nodes {dt} s apart: Phi vs expm {gphi:.2e} (bar {bphi:.2e}), Gamma {ggam:.2e} (bar {bgam:.2e}); gain at node 0 vs "
          f"the algebraic solution {gk:.2e} (bar {bk:.2e})")
    assert gphi <= bphi and ggam <= bgam
    assert float(g["const_gap_dare_G"]) <= 1e-9 and gk <= bk
    assert same(D["Phi"][0], np.tile(D["Phi"][0, 0], (K - 1, 1, 1)))  # one system, one transition: bitwise the same in every segment


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------
def held_flights(lqr_lib, name, hold, n_record=2, write_steps=30):
    """the 8 dispersed starts of trajectory 0 under the discrete gains, hold = node: device results, the gains flown and the inputs"""
    d, g = golden(name), dgolden(name)
    X, U, t = d[f"{hold}_X"][0], d[f"{hold}_U"][0], float(d[f"{hold}_t"][0])
    xs = d[f"{hold}_starts"]
    B = xs.shape[0]
    c = context(lqr_lib, name, d, hold, B=B)
    c.set_trajectories(np.tile(X, (B, 1, 1)), np.tile(U, (B, 1, 1)), np.full(B, t))
    assert c.compute_gains_discrete(int(g["steps"]), False) == B * X.shape[0]
    G = c.download_gains()["gains"]
    c.set_feedback_hold(1)
    assert c.track(xs, X[-1], float(d["time_step"]), 20, 2000, n_record, write_steps) == B
    r = c.track_download()
    r["record"] = c.track_record()
    c.set_feedback_hold(0)
    assert c.track(xs, X[-1], float(d["time_step"]), 20, 2000) == B
    r["step_mode"] = c.track_download()
    c.close()
    assert (G == G[0]).all()  # eight copies of one trajectory: eight bitwise equal sweeps
    return d, X, U, t, xs, G[0], r


@pytest.mark.parametrize("name,hold", CASES)
def test_held_flights_against_the_twin(lqr_lib, name, hold):
    """hold = node under the discrete gains (the gains the sweep left in the buffer): final x, last u, steps, status and max_dev of the 8 dispersed
    starts, and the record of the first two (every 30th step), vs track_held under the same, downloaded, gains: to the bar of the existing
    flight tests (1e-9 of the largest entry; test_lqr.py::test_tracking_kernel_alone).  The latch was taken once per segment.  hold = step with
    the same gains on the same context afterwards is bitwise the flight of a context that never heard of the mode."""
    d, X, U, t, xs, G, r = held_flights(lqr_lib, name, hold)
    B, K = xs.shape[0], X.shape[0]
    worst = 0.0
    for i in range(B):
        e = dr.track_held(MODELS[name], d["par"], X, U, G, t, xs[i], X[-1], time_step=float(d["time_step"]), write_steps=30)
        assert e["n_latch"] == K - 1
        assert r["status"][i] == 0 == e["status"] and r["steps"][i] == e["steps"]
        dx = np.abs(r["x"][i] - e["x"]).max() / np.abs(e["x"]).max()
        du = np.abs(r["u"][i] - e["u"]).max() / np.abs(e["u"]).max()
        dm = abs(r["max_dev"][i] - e["max_dev"]) / e["max_dev"]
        worst = max(worst, dx, du, dm)
        assert dx <= 1e-9 and du <= 1e-9 and dm <= 1e-9, (i, dx, du, dm)
        if i < 2:
            n = int(r["record"]["n"][i])
            assert n == len(e["rec_t"]) and n > 10
            rx = np.abs(r["record"]["X"][i, :n] - np.array(e["rec_x"])).max() / np.abs(np.array(e["rec_x"])).max()
            ru = np.abs(r["record"]["U"][i, :n] - np.array(e["rec_u"])).max() / np.abs(np.array(e["rec_u"])).max()
            worst = max(worst, rx, ru)
            assert rx <= 1e-9 and ru <= 1e-9 and np.abs(r["record"]["t"][i, :n] - np.array(e["rec_t"])).max() <= 1e-12, (i, rx, ru)
    print(f"{name} {hold}: device loop with the latch vs track_held {worst:.2e} (bar 1e-9); final errors {np.round(r['err1'], 3)}, "
          f"open loop {np.round(d[f'{hold}_err_open'], 2)}")
    assert (r["err1"] < d[f"{hold}_err_open"]).all()
    # hold = step after hold = node: the loop as it was
    c = context(lqr_lib, name, d, hold, B=B)
    c.set_trajectories(np.tile(X, (B, 1, 1)), np.tile(U, (B, 1, 1)), np.full(B, t))
    c.set_gains(np.tile(G, (B, 1, 1, 1)))
    assert c.track(xs, X[-1], float(d["time_step"]), 20, 2000) == B
    plain = c.track_download()
    c.close()
    for key in ("x", "u", "t", "steps", "status", "err0", "err1", "max_dev"):
        assert same(plain[key], r["step_mode"][key]), key
    assert not same(plain["x"], r["x"])


def test_held_flights_with_input_limits_and_a_sample_fan(lqr_lib):
    """Rocket2D, both first-order-hold trajectories, 3 flights each, hold = node, limits that bite (thrust capped inside the range the nominal
    itself commands, the gimbal inside the range the unlimited loop commands): n_sat equal to the twin's and > 0, max_clip, final x and last
    u to 1e-9, steps and status equal.  The clip acts on u_ref(t) + du, flight f follows trajectory f // 3."""
    name, S = "rocket2d", 3
    d, g = golden(name), dgolden(name)
    X, U, t = d["foh_X"], d["foh_U"], d["foh_t"]
    B = X.shape[0]
    xs = np.concatenate([X[b, 0] + (d["foh_starts"][:S] - X[0, 0]) for b in range(B)])
    lim = np.array([[0.5 * U[b][:, 1].min(), 0.97 * U[b][:, 1].max(), 0.8 * np.abs(U[b][:, 0]).max()] for b in range(B)])
    c = context(lqr_lib, name, d, "foh")
    assert c.compute_gains_discrete(int(g["steps"]), False) == B * X.shape[1]
    G = c.download_gains()["gains"]
    c.set_input_limits(lim)
    c.set_feedback_hold(1)
    assert c.track_samples(xs, X[0, -1], S, float(d["time_step"]), 20, 2000) == B * S
    r = c.track_download()
    r.update(c.track_download_saturation())
    c.close()
    worst = 0.0
    for f in range(B * S):
        b = f // S
        e = dr.track_held(MODELS[name], d["par"], X[b], U[b], G[b], float(t[b]), xs[f], X[0, -1], lim=lim[b], time_step=float(d["time_step"]),
                          saturate=sr.saturate)
        assert e["n_sat"] > 0 and r["n_sat"][f] == e["n_sat"] and r["steps"][f] == e["steps"] and r["status"][f] == e["status"] == 0
        dx = np.abs(r["x"][f] - e["x"]).max() / np.abs(e["x"]).max()
        du = np.abs(r["u"][f] - e["u"]).max() / np.abs(e["u"]).max()
        dc = abs(r["max_clip"][f] - e["max_clip"]) / e["max_clip"]
        worst = max(worst, dx, du, dc)
        assert dx <= 1e-9 and du <= 1e-9 and dc <= 1e-9, (f, dx, du, dc)
    print(f"rocket2d foh, limits and {S} flights per trajectory under hold = node: device vs track_held {worst:.2e} (bar 1e-9), n_sat {r['n_sat'].tolist()}")


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rocketquat", "rocket2d", "lander3dof"])
def test_the_linear_model_is_the_flights_model(lqr_lib, name):
    """2 nx + 1 sigma-point flights under hold = node along the dynamically exact golden nominal (first-order hold, trajectory 0; the starts are
    the generator's): their final deviations from the centre flight vs prod (Phi_i - Gamma_i K_i), from the device's own Phi, Gamma and gains,
    applied to the same starts.  The generator measures this gap with track_held and the exact matrices alone (sp_gap); the device's bar is
    2 x that: what the gap is made of -- the latch falling up to one plant step after the node, the flight ending up to one plant step after
    T, second-order terms -- both sides share."""
    d, g = golden(name), dgolden(name)
    X, U, t = d["foh_X"][:1], d["foh_U"][:1], d["foh_t"][:1]
    xs = g["sp_starts"]
    F = xs.shape[0]
    assert F == 2 * X.shape[2] + 1
    c = context(lqr_lib, name, d, "foh", B=1)
    c.set_trajectories(X, U, t)
    assert c.compute_gains_discrete(int(g["steps"]), True) == X.shape[1]
    G, D = c.download_gains()["gains"][0], c.download_discrete()
    c.set_feedback_hold(1)
    assert c.track_samples(xs, X[0, -1], F, float(d["time_step"]), 20, 2000) == F
    r = c.track_download()
    c.close()
    assert (r["status"] == 0).all()
    M = dr.closed_loop_product(np.concatenate([D["Phi"][0], D["Gamma"][0]], axis=2), G)
    pred = (xs[1:] - xs[0]) @ M.T
    gap = float(np.abs((r["x"][1:] - r["x"][0]) - pred).max() / np.abs(pred).max())
    print(f"{name}: sigma-point flights under hold = node vs the device's prod (Phi - Gamma K): {gap:.3e}; track_held vs the exact matrices "
          f"(generator) {float(g['sp_gap']):.3e}; bar {2.0 * float(g['sp_gap']):.3e}")
    assert gap <= 2.0 * float(g["sp_gap"])


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------------
def test_nonfinite_trajectory_gets_status_and_zeros(lqr_lib):
    """a NaN node, a NaN input or a non-finite flight time: SCPP_LQR_NONFINITE and zero gains on EVERY node of that trajectory, zero P, Phi and
    Gamma, nothing non-finite leaves the device, and the other trajectory of the batch is bitwise what it is without it"""
    d = golden("rocket2d")
    _, clean = sweep(lqr_lib, "rocket2d", d, "foh", 5)
    X, U, t = d["foh_X"].copy(), d["foh_U"].copy(), d["foh_t"].copy()
    K = X.shape[1]
    for what in ("node", "time", "input"):
        Xb, Ub, tb = X.copy(), U.copy(), t.copy()
        if what == "node":
            Xb[1, 5, 4] = np.nan
        elif what == "time":
            tb[1] = np.inf
        else:
            Ub[1, K - 1, 0] = np.nan
        c = context(lqr_lib, "rocket2d", d, "foh", B=2)
        c.set_trajectories(Xb, Ub, tb)
        assert c.compute_gains_discrete(5, True) == K
        o, D = c.download_gains(), c.download_discrete()
        c.close()
        assert (o["status"][1] == -2).all() and (o["gains"][1] == 0).all() and (o["iters"][1] == 0).all()
        assert all((D[k][1] == 0).all() and np.isfinite(D[k]).all() for k in ("P", "Phi", "Gamma")) and np.isfinite(o["gains"]).all()
        assert (o["status"][0] == 0).all() and same(o["gains"][0], clean["gains"][0])
        assert all(same(D[k][0], clean[k][0]) for k in ("P", "Phi", "Gamma"))


def test_p_overflowing_fails_that_node_and_every_earlier_one(lqr_lib):
    """State weights of 1e308 (Qf = Q): P_{K-1} = Qf is finite, Phi'Qf Phi is not, in the first segment the recursion takes, K-2.  That segment
    defines the gain of node K-1 as well, so every node gets SCPP_LQR_NONFINITE and zeros.  With Qf = 1 and Q = 1e306 the first steps are finite
    and P overflows further down: nodes 0..k carry the status and zeros, nodes k+1.. are finite and carry 0, k as the numpy recursion on the
    device's own Phi and Gamma finds it.  No non-finite value is written in either case."""
    from scpp_amd import _lib

    d = golden("rocket2d")
    X, U, t = d["foh_X"], d["foh_U"], d["foh_t"]
    B, K = X.shape[:2]

    def run(q, qf):
        c = _lib.LqrContext(1, K, B, True, 0, lqr_lib)
        c.set_weights(q, d["r"])
        c.set_terminal_weights(qf)
        c.set_flow_params(d["par"])
        c.set_trajectories(X, U, t)
        n = c.compute_gains_discrete(5, True)
        o = c.download_gains()
        o.update(c.download_discrete())
        c.close()
        assert all(np.isfinite(o[k]).all() for k in ("gains", "P", "Phi", "Gamma"))
        assert n == int((o["status"] == 0).sum())
        return o

    o = run(np.full(6, 1e308), None)
    assert (o["status"] == -2).all() and (o["iters"] == 0).all()
    assert all((o[k] == 0).all() for k in ("gains", "P", "Phi", "Gamma"))
    q = np.full(6, 1e306)
    o = run(q, np.ones(6))
    _, ok = sweep(lqr_lib, "rocket2d", d, "foh", 5)
    for b in range(B):
        with np.errstate(all="ignore"):
            try:
                Pn, Gn = dr.recursion(np.concatenate([ok["Phi"][b], ok["Gamma"][b]], axis=2), q, d["r"], np.ones(6), float(t[b]) / (K - 1))
            except (np.linalg.LinAlgError, ValueError):  # numpy / scipy refuse the non-finite matrix outright
                Pn = None
        st = o["status"][b]
        kf = int(np.flatnonzero(st == -2).max())
        print(f"trajectory {b}: nodes 0..{kf} failed, {K - 1 - kf} kept")
        assert 0 <= kf < K - 2 and (st[:kf + 1] == -2).all() and (st[kf + 1:] == 0).all()
        assert (o["gains"][b, :kf + 1] == 0).all() and (o["P"][b, :kf + 1] == 0).all() and (o["iters"][b, :kf + 1] == 0).all()
        assert (o["Phi"][b, :kf + 1] == 0).all() and (o["Gamma"][b, :kf + 1] == 0).all()
        assert np.abs(o["gains"][b, kf + 1:]).min(axis=(1, 2)).max() > 0 and same(o["Phi"][b, kf + 1:], ok["Phi"][b, kf + 1:])
        assert (o["iters"][b, kf + 1:] == (K - 1 - np.arange(kf + 1, K)) * 5).all()
        if Pn is not None:  # numpy's recursion, run through the overflow, turns non-finite at the same node
            bad = np.flatnonzero(~np.isfinite(Pn).all(axis=(1, 2)))
            assert bad.size and int(bad.max()) == kf


def test_abi_errors(lqr_lib):
    from scpp_amd import _lib

    L = _lib.load_lqr_library(lqr_lib)
    E_ARG, E_STATE = -1, -4
    d = golden("rocket2d")
    X, U, t = d["foh_X"], d["foh_U"], d["foh_t"]
    p = _lib._p
    n = ctypes.c_int()
    assert b"scpp_hip_lqr 2" in L.scpp_hip_lqr_version()
    c = _lib.LqrContext(1, 30, 2, True, 0, lqr_lib)
    c.set_weights(d["q"], d["r"])
    assert L.scpp_hip_lqr_compute_gains_discrete(c.h, 5, 0, ctypes.byref(n)) == E_STATE  # nothing set yet
    c.set_flow_params(d["par"])
    assert L.scpp_hip_lqr_compute_gains_discrete(c.h, 5, 0, ctypes.byref(n)) == E_STATE  # no trajectories
    c.set_trajectories(X, U, t)
    for steps in (0, -3):
        assert L.scpp_hip_lqr_compute_gains_discrete(c.h, steps, 0, ctypes.byref(n)) == E_ARG
    assert L.scpp_hip_lqr_compute_gains_discrete(None, 5, 0, None) == E_ARG
    Pb, Fb, Cb = np.zeros((2, 30, 6, 6)), np.zeros((2, 29, 6, 6)), np.zeros((2, 29, 6, 2))
    assert L.scpp_hip_lqr_download_discrete(None, p(Pb), p(Fb), p(Cb)) == E_ARG
    assert L.scpp_hip_lqr_download_discrete(c.h, p(Pb), p(Fb), p(Cb)) == E_STATE  # nothing computed
    assert L.scpp_hip_lqr_compute_gains_discrete(c.h, 5, 0, ctypes.byref(n)) == 0 and n.value == 60
    assert L.scpp_hip_lqr_download_discrete(c.h, p(Pb), p(Fb), p(Cb)) == E_STATE  # computed without keep
    assert L.scpp_hip_lqr_compute_gains_discrete(c.h, 5, 1, None) == 0
    assert L.scpp_hip_lqr_download_riccati(c.h, p(Pb)) == E_STATE  # the discrete P is not the Riccati sweep's
    assert L.scpp_hip_lqr_download_discrete(c.h, None, None, None) == 0  # any pointer may be NULL
    assert L.scpp_hip_lqr_download_discrete(c.h, None, p(Fb), None) == 0 and np.abs(Fb).max() > 0 and np.abs(Pb).max() == 0
    assert L.scpp_hip_lqr_download_discrete(c.h, p(Pb), p(Fb), p(Cb)) == 0 and np.abs(Pb).max() > 0 and np.abs(Cb).max() > 0
    for other in (lambda: c.compute_gains(), lambda: c.compute_gains_riccati(5, True), lambda: c.set_gains(np.zeros((2, 30, 2, 6))),
                  lambda: c.set_weights(d["q"], d["r"]), lambda: c.set_trajectories(X, U, t)):
        assert L.scpp_hip_lqr_compute_gains_discrete(c.h, 5, 1, None) == 0
        other()
        assert L.scpp_hip_lqr_download_discrete(c.h, p(Pb), p(Fb), p(Cb)) == E_STATE  # the last gain computation was another one
    # the feedback hold: 0 or 1, nothing else; it invalidates neither gains nor a covariance sweep
    assert L.scpp_hip_lqr_set_feedback_hold(None, 0) == E_ARG
    for mode in (2, -1, 7):
        assert L.scpp_hip_lqr_set_feedback_hold(c.h, mode) == E_ARG
    assert L.scpp_hip_lqr_compute_gains_discrete(c.h, 5, 1, None) == 0
    c.set_covariance_inputs(np.eye(6))
    assert c.propagate_covariance(2) == 2
    cov = c.download_covariance()
    gains = c.download_gains()
    assert L.scpp_hip_lqr_set_feedback_hold(c.h, 1) == 0
    assert L.scpp_hip_lqr_download_discrete(c.h, p(Pb), p(Fb), p(Cb)) == 0
    again = c.download_gains()
    assert all(same(again[k], gains[k]) for k in gains) and all(same(c.download_covariance()[k], cov[k]) for k in cov)
    # the mode stays until it is set again, across new trajectories and new gains
    xs = d["foh_starts"][:2]
    c.track(xs, X[0, -1], 0.01, 20, 300)
    held = c.track_download()
    c.set_trajectories(X, U, t)
    c.compute_gains_discrete(5)
    c.track(xs, X[0, -1], 0.01, 20, 300)
    assert same(c.track_download()["x"], held["x"])
    assert L.scpp_hip_lqr_set_feedback_hold(c.h, 0) == 0
    c.track(xs, X[0, -1], 0.01, 20, 300)
    assert not same(c.track_download()["x"], held["x"])
    c3 = _lib.LqrContext(1, 30, 3, True, 0, lqr_lib)  # parameter rows for 2 instances, 3 trajectories: refused as by compute_gains
    c3.set_weights(d["q"], d["r"])
    c3.set_flow_params(np.tile(d["par"], (2, 1)))
    c3.set_trajectories(np.tile(X[:1], (3, 1, 1)), np.tile(U[:1], (3, 1, 1)), np.tile(t[:1], 3))
    assert L.scpp_hip_lqr_compute_gains_discrete(c3.h, 5, 0, None) == E_STATE
    c3.close()
    c.close()


@pytest.mark.parametrize("name", ["rocketquat", "rocket2d"])
def test_batch_independence(lqr_lib, name):
    """a permuted, shorter batch on the SAME context (batch_max 2, then one trajectory: the other one): bitwise the rows of the full batch"""
    d = golden(name)
    X, U, t = d["foh_X"], d["foh_U"], d["foh_t"]
    c = context(lqr_lib, name, d, "foh")
    c.compute_gains_discrete(3, True)
    full = c.download_gains()
    full.update(c.download_discrete())
    for order in ([1, 0], [1]):
        c.set_trajectories(X[order], U[order], t[order])
        assert c.compute_gains_discrete(3, True) == len(order) * X.shape[1]
        o = c.download_gains()
        o.update(c.download_discrete())
        for j, b in enumerate(order):
            for key in ("gains", "status", "iters", "P", "Phi", "Gamma"):
                assert same(o[key][j], full[key][b]), (order, key)
    c.close()


def test_each_gain_law_leaves_exactly_its_own_gains(lqr_lib):
    """the discrete law before and after each of the other two on one context: gains, status and counts are bitwise those of a fresh context
    that ran that law alone"""
    d = golden("rocket2d")
    laws = dict(frozen=lambda c: c.compute_gains(), riccati=lambda c: c.compute_gains_riccati(5), discrete=lambda c: c.compute_gains_discrete(5))

    def fresh(law):
        c = context(lqr_lib, "rocket2d", d, "foh")
        laws[law](c)
        o = c.download_gains()
        c.close()
        return o

    alone = {law: fresh(law) for law in laws}
    c = context(lqr_lib, "rocket2d", d, "foh")
    for law in ("discrete", "frozen", "discrete", "riccati", "discrete"):
        laws[law](c)
        o = c.download_gains()
        for key in ("gains", "status", "iters"):
            assert same(o[key], alone[law][key]), (law, key)
    c.close()
    assert not same(alone["discrete"]["gains"], alone["riccati"]["gains"]) and not same(alone["discrete"]["gains"], alone["frozen"]["gains"])
    # the other law, for the record (the issue's sanity range is 3 .. 10 % of the largest entry)
    print(f"discrete vs Riccati-ODE gains: {dr.rel_gap(alone['discrete']['gains'], alone['riccati']['gains']):.3e} of the largest entry")


# ---- 7 -------------------------------------------------------------------------------------------------------------------------------------
def test_front_end_tracker(lqr_lib):
    """scpp_amd.LQRTracker(horizon="discrete") == the C ABI's gains and matrices; track(hold="node") == the C ABI's held flights, and
    track() afterwards is the default loop again"""
    import scpp_amd

    d = golden("rocket2d")
    X, U, t = d["foh_X"], d["foh_U"], d["foh_t"]
    m = scpp_amd.Rocket2D().loadParameters()
    _, abi = sweep(lqr_lib, "rocket2d", d, "foh", 5)
    trk = scpp_amd.LQRTracker(m, X, U, t, library=lqr_lib, horizon="discrete", keep_discrete=True)
    assert trk.n_ok == X.shape[0] * X.shape[1] and (trk.status == 0).all()
    assert same(trk.gains, abi["gains"]) and same(trk.iterations, abi["iters"]) and (trk.Qf == trk.Q).all()
    D = trk.discrete()
    assert all(same(D[k], abi[k]) for k in ("P", "Phi", "Gamma"))
    with pytest.raises(RuntimeError):
        trk.riccati
    xs = d["foh_starts"][:2]
    node = trk.track(xs, X[0, -1], hold="node")
    step = trk.track(xs, X[0, -1])
    with pytest.raises(ValueError):
        trk.track(xs, X[0, -1], hold="segment")
    c = context(lqr_lib, "rocket2d", d, "foh")
    c.set_gains(abi["gains"])
    c.track(xs, X[0, -1], 0.01, 20, 1202)
    plain = c.track_download()
    c.set_feedback_hold(1)
    c.track(xs, X[0, -1], 0.01, 20, 1202)
    held = c.track_download()
    c.close()
    assert (node["status"] == 0).all() and same(node["x"], held["x"]) and same(step["x"], plain["x"]) and not same(node["x"], step["x"])
    assert trk.computeGainsDiscrete(steps=1, keep=False) == trk.n_ok
    with pytest.raises(RuntimeError):
        trk.discrete()
    assert trk.computeGainsDiscrete(steps=1, keep=True) == trk.n_ok and trk.discrete()["Phi"].shape == abi["Phi"].shape
    trk.close()
    qf = np.array([10.0, 10.0, 20.0, 20.0, 5.0, 5.0])
    _, abi2 = sweep(lqr_lib, "rocket2d", d, "foh", 5, qf=qf)
    trk = scpp_amd.LQRTracker(m, X, U, t, library=lqr_lib, horizon="discrete", terminal_weights=qf, discrete_steps=5)
    assert same(trk.gains, abi2["gains"]) and not same(trk.gains, abi["gains"])
    with pytest.raises(RuntimeError):
        trk.discrete()
    trk.close()
    with pytest.raises(ValueError):
        scpp_amd.LQRTracker(m, X, U, t, library=lqr_lib, horizon="sampled")


@pytest.mark.xdist_group("host_cpp")  # shares the build directory scpp_amd/host with tests/test_host_cpp.py
def test_sc_tracking_names_the_gain_law_and_the_hold(backend, tmp_path):
    """host/sc_tracking --gains discrete --hold node: solves, sweeps, flies, and names both choices in its summary (K = 10 nodes, as the emulation
    build runs in test_lqr.py); another --hold is refused before anything is solved"""
    import __graft_entry__ as g

    name, _, solver = backend
    host = os.path.join(ROOT, "scpp_amd", "host")
    solver()
    if name == "emu":
        subprocess.check_call(["make", "-s", "-C", host, "sc_tracking_emu"])
        cmd = [os.path.join(host, "sc_tracking_emu")]
    else:
        g.build_host()
        cmd = [os.path.join(host, "sc_tracking")]
    cmd += ["--K", "10", "--batch", "2", "--config", os.path.join(ROOT, "scpp_amd", "config"), "--out", str(tmp_path)]
    r = subprocess.run(cmd + ["--gains", "discrete", "--discrete-steps", "4", "--hold", "node"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "Gains: discrete" in r.stdout and "4 RKF78 steps per segment" in r.stdout and "Hold: node" in r.stdout and "Final error:" in r.stdout
    assert "(20 converged)" in r.stdout
    assert subprocess.run(cmd + ["--hold", "other"], capture_output=True, text=True).returncode == 2

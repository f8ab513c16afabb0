"""Finite-horizon LQR gains (scpp_hip_lqr_compute_gains_riccati, scpp_amd/csrc/lqr/lqr_riccati_kernel.h): every test runs the SAME assertions
on the CPU emulation of the kernel sources (`emu`) and, marked gpu, on the device library (`hip`).

Checkers (tests/lqr_riccati_reference.py, no code shared with the kernels): the exact answer (DOP853, rtol 1e-12, stored by
tests/golden/generate_lqr_riccati_goldens.py) and the twin (numpy fixed-step RKF78 of the same definition on the oracle's Jacobians, run here).
Inputs: tests/golden/lqr_<model>.npz (trajectories, weights, dispersed starts; read only) and tests/golden/lqr_riccati_<model>.npz.

Bars: device vs twin 10 x gap_round (the twin against a copy of itself with Jacobians perturbed by 1 ulp; the factor 10 covers fused
multiply-add placement and the summation order of the tile product); device vs exact gap_scheme + that.  Both relative to max|P| and
max|K| of the trajectory, both measured by the generator with the reference alone."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import lqr_reference as ref
import lqr_riccati_reference as rr

MODELS = {"rocketquat": 0, "rocket2d": 1, "lander3dof": 2}
CASES = [("rocketquat", "foh"), ("rocketquat", "zoh"), ("rocket2d", "foh"), ("rocket2d", "zoh"), ("lander3dof", "foh"), ("lander3dof", "zoh")]
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
EPS = float(np.finfo(float).eps)


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


def rgolden(name):
    return np.load(os.path.join(GOLDEN, f"lqr_riccati_{name}.npz"))


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
    c = context(lib, name, d, hold)
    if qf is not None:
        c.set_terminal_weights(qf)
    n_ok = c.compute_gains_riccati(steps, True)
    o = c.download_gains()
    o["P"] = c.download_riccati()
    c.close()
    return n_ok, o


def bars(g, hold, b):
    """(P vs twin, K vs twin, P vs exact, K vs exact) of trajectory b"""
    rp, rk = 10.0 * float(g[f"{hold}_gap_round_P"][b]), 10.0 * float(g[f"{hold}_gap_round_G"][b])
    return rp, rk, float(g[f"{hold}_gap_scheme_P"][b]) + rp, float(g[f"{hold}_gap_scheme_G"][b]) + rk


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hold", CASES)
def test_gains_and_p_against_twin_and_exact(lqr_lib, name, hold):
    """P(t_k) and K_k of every node vs the twin (bar 10 x gap_round) and vs the exact answer (bar gap_scheme + that); status 0 everywhere,
    n_ok = B K, the count of node k is (K-1-k) steps.  The generator asserts that a twin with ONE tableau entry's sign flipped misses the
    second bar by a factor >= 100."""
    d, g = golden(name), rgolden(name)
    steps = int(g["steps"])
    X, U, t = d[f"{hold}_X"], d[f"{hold}_U"], d[f"{hold}_t"]
    B, K = X.shape[0], X.shape[1]
    n_ok, o = sweep(lqr_lib, name, d, hold, steps)
    assert np.isfinite(o["gains"]).all() and np.isfinite(o["P"]).all()
    for b in range(B):
        Pt, Gt = rr.twin(MODELS[name], d["par"], X[b], U[b], float(t[b]), d["q"], d["r"], steps=steps)
        bp, bk, ep, ek = bars(g, hold, b)
        gp, gk = rr.rel_gap(o["P"][b], Pt), rr.rel_gap(o["gains"][b], Gt)
        xp, xk = rr.rel_gap(o["P"][b], g[f"{hold}_P_exact"][b]), rr.rel_gap(o["gains"][b], g[f"{hold}_G_exact"][b])
        print(f"{name} {hold} {b}: vs twin P {gp:.2e} (bar {bp:.2e}) K {gk:.2e} (bar {bk:.2e}); vs exact P {xp:.2e} (bar {ep:.2e}) K {xk:.2e} (bar {ek:.2e})")
        assert gp <= bp and gk <= bk, (gp, bp, gk, bk)
        assert xp <= ep and xk <= ek, (xp, ep, xk, ek)
    assert (o["status"] == 0).all() and n_ok == B * K
    assert (o["iters"] == (K - 1 - np.arange(K)) * steps).all()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hold", CASES)
def test_structure(lqr_lib, name, hold):
    """P symmetric to the rounding bar, positive definite at every node, P[K-1] == Qf exactly, gains[K-1] == R^-1 B'Qf to rounding (one
    product and one scaling per entry, B from two implementations of the same Jacobian: 8 ulp of max|K[K-1]|); another terminal weight
    (Qf = 10 Q) changes P near the end, and changes node 0 by less than node K-2.  "Changes" is |dP(t_k)|_F / |P(t_k)|_F, the change
    relative to the node's own P: at node K-2, P is Qf plus one segment of running cost, so it moves by nearly the factor 9; at node 0 it
    is dominated by 12 s of running cost.  (In ABSOLUTE terms the change does not decay along these trajectories -- the mass is not
    controllable, a terminal weight on it is carried back unchanged and grows with the open-loop modes: Lander3dof moves by 0.8 of max|P| at
    node 0 and by 0.02 at node K-2 -- so an absolute measure would test the plant, not the sweep.)  The twin, run here with the same Qf, must
    show the same ordering and agree with the device to 10 x the twin's own rounding floor at THIS Qf (measured here as the generator does:
    against a copy with Jacobians perturbed by 1 ulp)."""
    import oracle_lib

    d, g = golden(name), rgolden(name)
    steps = int(g["steps"])
    X, U = d[f"{hold}_X"], d[f"{hold}_U"]
    B, K = X.shape[0], X.shape[1]
    _, o = sweep(lqr_lib, name, d, hold, steps)
    P = o["P"]
    for b in range(B):
        asym = np.abs(P[b] - P[b].transpose(0, 2, 1)).max() / np.abs(P[b]).max()
        ev = min(np.linalg.eigvalsh(0.5 * (P[b, k] + P[b, k].T)).min() for k in range(K))
        print(f"{name} {hold} {b}: asymmetry {asym:.2e} of max|P|, smallest eigenvalue over the nodes {ev:.3e}")
        assert asym <= bars(g, hold, b)[0]
        assert ev > 0.0
        assert (P[b, K - 1] == np.diag(d["q"])).all()
        _, _, Bm = oracle_lib.flow(MODELS[name], X[b, K - 1], U[b, min(K - 1, U.shape[1] - 1)], d["par"])
        Kl = (Bm.T * d["q"][None, :]) / d["r"][:, None]
        assert np.abs(o["gains"][b, K - 1] - Kl).max() <= 8 * EPS * np.abs(Kl).max()
    qf = 10.0 * d["q"]
    _, o2 = sweep(lqr_lib, name, d, hold, steps, qf=qf)
    t = d[f"{hold}_t"]
    for b in range(B):
        assert (o2["P"][b, K - 1] == np.diag(qf)).all()
        Pt0, _ = rr.twin(MODELS[name], d["par"], X[b], U[b], float(t[b]), d["q"], d["r"], steps=steps)
        Pt, _ = rr.twin(MODELS[name], d["par"], X[b], U[b], float(t[b]), d["q"], d["r"], qf=qf, steps=steps)
        ch = np.linalg.norm(o2["P"][b] - P[b], axis=(1, 2)) / np.linalg.norm(P[b], axis=(1, 2))
        cht = np.linalg.norm(Pt - Pt0, axis=(1, 2)) / np.linalg.norm(Pt0, axis=(1, 2))
        rng = np.random.default_rng(100 + b)
        Pp, _ = rr.twin(MODELS[name], d["par"], X[b], U[b], float(t[b]), d["q"], d["r"], qf=qf, steps=steps, perturb=lambda A, Bm: (
            A * (1.0 + EPS * rng.choice([-1.0, 1.0], A.shape)), Bm * (1.0 + EPS * rng.choice([-1.0, 1.0], Bm.shape))))
        gp, floor = rr.rel_gap(o2["P"][b], Pt), rr.rel_gap(Pp, Pt)
        print(f"{name} {hold} {b}: Qf = 10 Q moves P(t_k) by {ch[K - 2]:.2e} of itself at node K-2, {ch[0]:.2e} at node 0 (twin: {cht[K - 2]:.2e}, {cht[0]:.2e}); "
              f"device vs twin {gp:.2e} (bar {10 * floor:.2e})")
        assert cht[K - 2] > 0.0 and cht[0] < cht[K - 2]
        assert ch[K - 2] > 0.0 and ch[0] < ch[K - 2]
        assert gp <= 10.0 * floor


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rocketquat", "rocket2d", "lander3dof"])
def test_zero_order_hold_keeps_the_segment_index(lqr_lib, name):
    """Zero-order hold: a stage at a = 0 or a = 1 stays in the segment being integrated.  The device meets the same bar against the exact answer
    as under first-order hold, while a twin that re-derives the segment from t (and so reads the neighbouring segment's constant input at
    a node-aligned stage) misses it by >= 1e4 x the bar (stored by the generator)."""
    d, g = golden(name), rgolden(name)
    _, o = sweep(lqr_lib, name, d, "zoh", int(g["steps"]))
    for b in range(d["zoh_X"].shape[0]):
        _, _, ep, ek = bars(g, "zoh", b)
        xp, xk = rr.rel_gap(o["P"][b], g["zoh_P_exact"][b]), rr.rel_gap(o["gains"][b], g["zoh_G_exact"][b])
        print(f"{name} zoh {b}: device vs exact P {xp:.2e} (bar {ep:.2e}), K {xk:.2e} (bar {ek:.2e}); re-timed twin vs exact {float(g['zoh_retime_gap'][b]):.2e}")
        assert float(g["zoh_retime_gap"][b]) >= 1e4 * ep
        assert xp <= ep and xk <= ek


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------
def test_constant_system_converges_to_the_algebraic_solution(lqr_lib):
    """Two-node constant trajectory at Rocket2D's operating point, horizon and step count from the generator: there the exact P(0) and gain are
    within 1e-8 of solve_continuous_are's and the twin within 1e-9 of the exact answer (both asserted by the generator).  Device P(0) vs the
    algebraic P: 2e-8 of max|P| (1e-8 horizon + 1e-9 scheme, the rest, 9e-9, for rounding over 1400 steps).  Device gain vs the frozen-time
    kernel's gain at the same point: 3e-8 of max|K| (the same 2e-8 plus the 1e-8 the sign iteration stops at)."""
    import scipy.linalg

    import oracle_lib
    import scpp_amd
    from scpp_amd import _lib

    d, g = golden("rocket2d"), rgolden("rocket2d")
    T, steps = float(g["const_horizon"]), int(g["const_steps"])
    m = scpp_amd.Rocket2D().loadParameters()
    x_eq, u_eq = (np.asarray(v, dtype=np.float64) for v in m.getOperatingPoint())
    c = _lib.LqrContext(1, 2, 1, True, 0, lqr_lib)
    c.set_weights(d["q"], d["r"])
    c.set_flow_params(d["par"])
    c.set_trajectories(np.tile(x_eq, (1, 2, 1)), np.tile(u_eq, (1, 2, 1)), [T])
    assert c.compute_gains_riccati(steps, True) == 2
    o, P = c.download_gains(), c.download_riccati()
    assert c.compute_gains() == 2
    frozen = c.download_gains()
    c.close()
    _, A, Bm = oracle_lib.flow(1, x_eq, u_eq, d["par"])
    Pc = scipy.linalg.solve_continuous_are(A, Bm, np.diag(d["q"]), np.diag(d["r"]))
    gp, gk = rr.rel_gap(P[0, 0], Pc), rr.rel_gap(o["gains"][0, 0], frozen["gains"][0, 0])
    print(f"constant system, horizon {T} s, {steps} steps: P(0) vs CARE {gp:.2e} (bar 2e-8), gain vs the frozen-time kernel {gk:.2e} (bar 3e-8)")
    assert float(g["const_gap_P"]) <= 1e-8 and float(g["const_gap_G"]) <= 1e-8 and float(g["const_scheme_P"]) <= 1e-9 and float(g["const_scheme_G"]) <= 1e-9
    assert gp <= 2e-8 and gk <= 3e-8
    assert o["iters"].tolist() == [[steps, 0]]


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hold", CASES)
def test_flights_under_riccati_gains(lqr_lib, name, hold):
    """scpp_hip_lqr_track flies the gains the sweep left in the gain buffer (no set_gains in between): final x, u, t, steps of the 8 dispersed
    starts vs the restatement's loop under the same, downloaded, gains, to the bar of test_lqr.py::test_tracking_kernel_alone (1e-9 max|x|;
    the tracking kernel is unchanged).  Every flight ends below the stored open-loop error (the generator asserts it of the exact gains)."""
    d, g = golden(name), rgolden(name)
    X, U, t = d[f"{hold}_X"][0], d[f"{hold}_U"][0], float(d[f"{hold}_t"][0])
    xs = d[f"{hold}_starts"]
    B = xs.shape[0]
    c = context(lqr_lib, name, d, hold, B=B)
    c.set_trajectories(np.tile(X, (B, 1, 1)), np.tile(U, (B, 1, 1)), np.full(B, t))
    assert c.compute_gains_riccati(int(g["steps"]), False) == B * X.shape[0]
    G = c.download_gains()["gains"]
    assert c.track(xs, X[-1], float(d["time_step"]), 20, 2000) == B
    r = c.track_download()
    c.close()
    assert (G == G[0]).all()  # eight copies of one trajectory: eight bitwise equal sweeps
    worst = 0.0
    for i in range(B):
        e = ref.track(MODELS[name], d["par"], X, U, G[0], t, xs[i], X[-1], float(d["time_step"]))
        assert r["status"][i] == 0 and r["steps"][i] == e["steps"]
        dx = np.abs(r["x"][i] - e["x"]).max() / np.abs(e["x"]).max()
        du = np.abs(r["u"][i] - e["u"]).max() / np.abs(e["u"]).max()
        worst = max(worst, dx, du)
        assert dx <= 1e-9 and du <= 1e-9, (i, dx, du)
    print(f"{name} {hold}: device loop vs restatement {worst:.2e} (bar 1e-9); final errors {np.round(r['err1'], 3)}, exact gains "
          f"{np.round(g[f'{hold}_err_exact'], 3)}, frozen-time {np.round(d[f'{hold}_err_closed'], 3)}, open loop {np.round(d[f'{hold}_err_open'], 2)}")
    assert (g[f"{hold}_err_exact"] < d[f"{hold}_err_open"]).all()
    assert (r["err1"] < d[f"{hold}_err_open"]).all()


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------------
def test_nonfinite_trajectory_gets_status_and_zero_gains(lqr_lib):
    """a NaN node (or a non-finite flight time): SCPP_LQR_NONFINITE and zero gains on EVERY node of that trajectory, zero P, nothing non-finite
    leaves the device, and the other trajectory of the batch is bitwise what it is without it"""
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
        assert c.compute_gains_riccati(5, True) == K
        o, P = c.download_gains(), c.download_riccati()
        c.close()
        assert (o["status"][1] == -2).all() and (o["gains"][1] == 0).all() and (P[1] == 0).all() and (o["iters"][1] == 0).all()
        assert np.isfinite(o["gains"]).all() and np.isfinite(P).all()
        assert (o["status"][0] == 0).all() and (o["gains"][0] == clean["gains"][0]).all() and (P[0] == clean["P"][0]).all()


def test_p_turning_nonfinite_fails_that_node_and_every_earlier_one(lqr_lib):
    """weights of 1e200: P(T) = Qf and the last node's gain are finite, the quadratic term overflows in the first stage of segment K-2.
    Nodes 0..K-2 get SCPP_LQR_NONFINITE and zeros, node K-1 keeps status 0; no non-finite value is written."""
    from scpp_amd import _lib

    d = golden("rocket2d")
    X, U, t = d["foh_X"], d["foh_U"], d["foh_t"]
    K = X.shape[1]
    c = _lib.LqrContext(1, K, 2, True, 0, lqr_lib)
    c.set_weights(np.full(6, 1e200), d["r"])
    c.set_flow_params(d["par"])
    c.set_trajectories(X, U, t)
    assert c.compute_gains_riccati(5, True) == 2
    o, P = c.download_gains(), c.download_riccati()
    c.close()
    assert np.isfinite(o["gains"]).all() and np.isfinite(P).all()
    assert (o["status"][:, K - 1] == 0).all() and (o["status"][:, :K - 1] == -2).all()
    assert (o["gains"][:, :K - 1] == 0).all() and (P[:, :K - 1] == 0).all() and np.abs(o["gains"][:, K - 1]).max() > 0
    assert (o["iters"] == 0).all()


def test_abi_errors(lqr_lib):
    from scpp_amd import _lib

    L = _lib.load_lqr_library(lqr_lib)
    E_ARG, E_STATE = -1, -4
    d = golden("rocket2d")
    X, U, t = d["foh_X"], d["foh_U"], d["foh_t"]
    p = _lib._p
    n = ctypes.c_int()
    c = _lib.LqrContext(1, 30, 2, True, 0, lqr_lib)
    c.set_weights(d["q"], d["r"])
    assert L.scpp_hip_lqr_compute_gains_riccati(c.h, 5, 0, ctypes.byref(n)) == E_STATE  # nothing set yet
    c.set_flow_params(d["par"])
    assert L.scpp_hip_lqr_compute_gains_riccati(c.h, 5, 0, ctypes.byref(n)) == E_STATE  # no trajectories
    c.set_trajectories(X, U, t)
    for steps in (0, -3):
        assert L.scpp_hip_lqr_compute_gains_riccati(c.h, steps, 0, ctypes.byref(n)) == E_ARG
    assert L.scpp_hip_lqr_compute_gains_riccati(None, 5, 0, None) == E_ARG
    for qf in (np.array([1, 1, 1, 0, 1, 1.0]), np.array([1, 1, -2.0, 1, 1, 1]), np.array([1, np.nan, 1, 1, 1, 1.0]), np.array([1, np.inf, 1, 1, 1, 1.0])):
        assert L.scpp_hip_lqr_set_terminal_weights(c.h, p(qf)) == E_ARG  # refused, not clamped
    assert L.scpp_hip_lqr_set_terminal_weights(None, None) == E_ARG
    assert L.scpp_hip_lqr_set_terminal_weights(c.h, None) == 0  # Qf = Q
    Pbuf = np.zeros((2, 30, 6, 6))
    assert L.scpp_hip_lqr_download_riccati(c.h, p(Pbuf)) == E_STATE  # nothing computed
    assert L.scpp_hip_lqr_compute_gains_riccati(c.h, 5, 0, ctypes.byref(n)) == 0 and n.value == 60
    assert L.scpp_hip_lqr_download_riccati(c.h, p(Pbuf)) == E_STATE  # computed without keep_p
    assert L.scpp_hip_lqr_compute_gains_riccati(c.h, 5, 1, None) == 0
    assert L.scpp_hip_lqr_download_riccati(c.h, None) == E_ARG
    assert L.scpp_hip_lqr_download_riccati(c.h, p(Pbuf)) == 0 and np.abs(Pbuf).max() > 0
    c.compute_gains()
    assert L.scpp_hip_lqr_download_riccati(c.h, p(Pbuf)) == E_STATE  # the last computation was the frozen-time one
    c3 = _lib.LqrContext(1, 30, 3, True, 0, lqr_lib)  # parameter rows for 2 instances, 3 trajectories: refused as by compute_gains
    c3.set_weights(d["q"], d["r"])
    c3.set_flow_params(np.tile(d["par"], (2, 1)))
    c3.set_trajectories(np.tile(X[:1], (3, 1, 1)), np.tile(U[:1], (3, 1, 1)), np.tile(t[:1], 3))
    assert L.scpp_hip_lqr_compute_gains_riccati(c3.h, 5, 0, None) == E_STATE
    c3.close()
    c.close()


@pytest.mark.parametrize("name", ["rocketquat", "rocket2d"])
def test_batch_independence(lqr_lib, name):
    """trajectory b alone == trajectory b in a batch, bitwise: gains, P and counts (the pattern of test_lqr.py::test_batch_independence)"""
    d = golden(name)
    X, U, t = d["foh_X"], d["foh_U"], d["foh_t"]
    _, batch = sweep(lqr_lib, name, d, "foh", 3)
    for b in range(X.shape[0]):
        c1 = context(lqr_lib, name, d, "foh", B=1)
        c1.set_trajectories(X[b:b + 1], U[b:b + 1], t[b:b + 1])
        c1.compute_gains_riccati(3, True)
        one, P1 = c1.download_gains(), c1.download_riccati()
        c1.close()
        assert (one["gains"][0] == batch["gains"][b]).all() and (P1[0] == batch["P"][b]).all()
        assert one["iters"][0].tolist() == batch["iters"][b].tolist() and one["status"][0].tolist() == batch["status"][b].tolist()


def test_each_gain_law_leaves_exactly_its_own_gains(lqr_lib):
    """compute_gains after compute_gains_riccati, and the reverse: gains, status and counts are bitwise those of a fresh context"""
    d = golden("rocketquat")

    def fresh(riccati):
        c = context(lqr_lib, "rocketquat", d, "foh")
        c.compute_gains_riccati(5) if riccati else c.compute_gains()
        o = c.download_gains()
        c.close()
        return o

    f_frozen, f_ric = fresh(False), fresh(True)
    c = context(lqr_lib, "rocketquat", d, "foh")
    c.compute_gains_riccati(5)
    c.compute_gains()
    a = c.download_gains()
    c.compute_gains_riccati(5)
    b = c.download_gains()
    c.close()
    for key in ("gains", "status", "iters"):
        assert (a[key] == f_frozen[key]).all(), key
        assert (b[key] == f_ric[key]).all(), key
    assert not (f_frozen["gains"] == f_ric["gains"]).all()


# ---- 7 -------------------------------------------------------------------------------------------------------------------------------------
def test_front_end_tracker(lqr_lib, tmp_path):
    """scpp_amd.LQRTracker(horizon="finite") == the C ABI's gains; the default constructor is bitwise the frozen-time path; LQR.info's optional
    terminal_weights is read when the argument is left out"""
    import scpp_amd

    d = golden("rocket2d")
    X, U, t = d["foh_X"], d["foh_U"], d["foh_t"]
    m = scpp_amd.Rocket2D().loadParameters()
    assert scpp_amd.load_lqr_terminal_weights(m) is None  # absent from the shipped file: Qf = Q
    _, abi = sweep(lqr_lib, "rocket2d", d, "foh", 5)
    trk = scpp_amd.LQRTracker(m, X, U, t, library=lqr_lib, horizon="finite", keep_riccati=True)
    assert trk.n_ok == X.shape[0] * X.shape[1] and (trk.status == 0).all()
    assert (trk.gains == abi["gains"]).all() and (trk.riccati == abi["P"]).all() and (trk.iterations == abi["iters"]).all()
    assert (trk.Qf == trk.Q).all()
    out = trk.track(d["foh_starts"][:2], X[0, -1])
    assert (out["status"] == 0).all()
    assert trk.computeGainsRiccati(steps=3) == trk.n_ok and not (trk.gains == abi["gains"]).all()
    trk.close()
    c = context(lqr_lib, "rocket2d", d, "foh")
    c.compute_gains()
    frozen = c.download_gains()
    c.close()
    trk = scpp_amd.LQRTracker(m, X, U, t, library=lqr_lib)
    assert trk.horizon == "infinite" and (trk.gains == frozen["gains"]).all() and (trk.iterations == frozen["iters"]).all()
    with pytest.raises(RuntimeError):
        trk.riccati
    trk.close()
    with pytest.raises(ValueError):
        scpp_amd.LQRTracker(m, X, U, t, library=lqr_lib, horizon="receding")
    # terminal_weights in LQR.info
    cfg = tmp_path / "config"
    shutil.copytree(os.path.join(ROOT, "scpp_amd", "config"), cfg)
    with open(cfg / "Rocket2D" / "LQR.info", "a") as f:
        f.write("\nterminal_weights\n{\n" + "".join(f"    ({i}) {v}\n" for i, v in enumerate([10, 10, 20, 20, 5, 5])) + "}\n")
    m2 = scpp_amd.Rocket2D(str(cfg)).loadParameters()
    qf = scpp_amd.load_lqr_terminal_weights(m2)
    assert qf.tolist() == [10.0, 10.0, 20.0, 20.0, 5.0, 5.0]
    _, abi2 = sweep(lqr_lib, "rocket2d", d, "foh", 5, qf=qf)
    trk = scpp_amd.LQRTracker(m2, X, U, t, library=lqr_lib, horizon="finite")
    assert (trk.gains == abi2["gains"]).all() and not (trk.gains == abi["gains"]).all()
    trk.close()


@pytest.mark.xdist_group("host_cpp")  # shares the build directory scpp_amd/host with tests/test_host_cpp.py
def test_sc_tracking_names_the_gain_law(backend, tmp_path):
    """host/sc_tracking --gains riccati: solves, sweeps, flies, and names the choice in its summary; the default names `frozen`.  (The emulation
    build runs K = 10 nodes, as in test_lqr.py.)"""
    import __graft_entry__ as g

    name, _, solver = backend
    host = os.path.join(ROOT, "scpp_amd", "host")
    solver()
    if name == "emu":
        subprocess.check_call(["make", "-s", "-C", host, "sc_tracking_emu"])
        cmd = [os.path.join(host, "sc_tracking_emu"), "--K", "10"]
    else:
        g.build_host()
        cmd = [os.path.join(host, "sc_tracking")]
    cmd += ["--batch", "4", "--config", os.path.join(ROOT, "scpp_amd", "config"), "--out", str(tmp_path)]
    r = subprocess.run(cmd + ["--gains", "riccati", "--riccati-steps", "4"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "Gains: riccati" in r.stdout and "4 RKF78 steps per segment" in r.stdout and "Final error:" in r.stdout
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and "Gains: frozen" in r.stdout
    assert subprocess.run(cmd + ["--gains", "other"], capture_output=True, text=True).returncode == 2

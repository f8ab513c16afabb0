"""The LQR tracker (include/scpp_hip_lqr.h, scpp_amd/csrc/lqr/, scpp_amd/lqr.py): every test runs the SAME assertions on the CPU emulation of the
kernel sources (`emu`) and, marked gpu, on the device library (`hip`).

Checkers (none shares code with the kernels): tests/lqr_reference.py, a numpy restatement of LQR.cpp / LQRTracker.cpp / the SC_tracking loop on
the oracle's Jacobians and plant step, and scipy.linalg.solve_continuous_are.  Inputs: tests/golden/lqr_<model>.npz (generate_lqr_goldens.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import lqr_reference as ref

MODELS = {"rocketquat": 0, "rocket2d": 1, "lander3dof": 2}
CASES = [("rocketquat", "foh"), ("rocketquat", "zoh"), ("rocket2d", "foh"), ("rocket2d", "zoh"), ("lander3dof", "foh"), ("lander3dof", "zoh")]
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]


@pytest.fixture(scope="module", params=BACKENDS)
def backend(request):
    """(name, LQR library, solver library) of the emulation build or of the device build"""
    import __graft_entry__ as g

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


def context(lib, name, d, hold, B=None, weights=True):
    from scpp_amd import _lib

    X, U, t = d[f"{hold}_X"], d[f"{hold}_U"], d[f"{hold}_t"]
    c = _lib.LqrContext(MODELS[name], X.shape[1], X.shape[0] if B is None else B, hold == "foh", 0, lib)
    if weights:
        c.set_weights(d["q"], d["r"])
    c.set_flow_params(d["par"])
    if B is None:
        c.set_trajectories(X, U, t)
    return c


def device_gains(lib, name, d, hold):
    c = context(lib, name, d, hold)
    n_ok = c.compute_gains()
    out = c.download_gains()
    c.close()
    return n_ok, out


# ---- T1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hold", CASES)
def test_gains_agree_with_scipy(lqr_lib, name, hold):
    """Device gain vs scipy's solve_continuous_are gain, relative to max|K_scipy| of the node.  The bar is 10 x the largest gap the numpy
    restatement shows against scipy over the same nodes (stored by the generator: 1e-12 .. 4e-11 for these trajectories); the factor 10
    covers different rounding in the 7 - 13 Newton steps, which stop on a 1e-8 relative test.  Status 0 everywhere; the iteration count equals
    the restatement's on >= 95 % of the nodes and is within +-1 elsewhere (a cap the restatement meets against a copy of itself whose
    Jacobians are perturbed by 1 ulp: asserted in the generator)."""
    d = golden(name)
    n_ok, o = device_gains(lqr_lib, name, d, hold)
    Gs, it_ref = d[f"{hold}_G_scipy"], d[f"{hold}_it_ref"]
    bar = 10.0 * float(d[f"{hold}_gap"].max())
    gap = np.abs(o["gains"] - Gs).max(axis=(2, 3)) / np.abs(Gs).max(axis=(2, 3))
    same = float((o["iters"] == it_ref).mean())
    print(f"{name} {hold}: device vs scipy {gap.max():.3e} (bar {bar:.3e}), iterations {o['iters'].min()}..{o['iters'].max()}, equal to the restatement's on {same:.3f}")
    assert (o["status"] == 0).all() and n_ok == it_ref.size
    assert np.isfinite(o["gains"]).all()
    assert gap.max() <= bar, (gap.max(), bar)
    assert same >= 0.95 and (np.abs(o["iters"] - it_ref) <= 1).all()


# ---- T2 ------------------------------------------------------------------------------------------------------------------------------------
def test_rocketquat_at_zero_body_rate(lqr_lib):
    """At w_B = 0 (node 0 of both golden trajectories; every node of trajectory 0) the device gain is finite, the closed loop of the tangent
    system A_r - B_r K_r is Hurwitz and K q = 0 on the quaternion columns -- while the reference's literal 14-state path, run by the
    restatement on the same node, does not give the Riccati gain: its Hamiltonian is singular (p = (0,..,q,..,0): p'A = 0, p'B = 0), the sign
    iteration either fails or 'converges' to something else.  This is why the engine deviates."""
    import oracle_lib

    d = golden("rocketquat")
    _, o = device_gains(lqr_lib, "rocketquat", d, "foh")
    X, U, par, q, r = d["foh_X"], d["foh_U"], d["par"], d["q"], d["r"]
    for b, k in ((0, 0), (0, 25), (0, 49), (1, 0)):
        x, u = X[b, k], U[b, k]
        assert np.abs(x[11:14]).max() == 0.0
        K = o["gains"][b, k]
        assert o["status"][b, k] == 0 and np.isfinite(K).all()
        _, A, Bm = oracle_lib.flow(0, x, u, par)
        N = ref.tangent_basis(0, x)
        Ar, Br, Kr = N.T @ A @ N, N.T @ Bm, K @ N
        ev = np.linalg.eigvals(Ar - Br @ Kr)
        assert ev.real.max() < 0.0, ev.real.max()
        assert np.abs(K[:, 7:11] @ x[7:11]).max() <= 1e-9 * np.abs(K).max()
        # the singular direction of the 14-state system
        p = np.zeros(14)
        p[7:11] = x[7:11]
        assert np.abs(p @ A).max() <= 1e-12 and np.abs(p @ Bm).max() <= 1e-12
        K14, it14, st14 = ref.node_gain(0, x, u, par, q, r, tangent=False)
        Ks = d["foh_G_scipy"][b, k]
        off = np.abs(K14 - Ks).max() / np.abs(Ks).max()
        print(f"node ({b},{k}): 14-state path status {st14} after {it14} iterations, gain off scipy's by {off:.2e}; tangent path (device) "
              f"{np.abs(K - Ks).max() / np.abs(Ks).max():.2e}, closed-loop abscissa {ev.real.max():.3e}")
        assert st14 != 0 or off > 1e-3


# ---- T3 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hold", CASES)
def test_tracking_kernel_alone(lqr_lib, name, hold):
    """The tracking kernel on its own: the gains downloaded from the device are handed to both sides (scpp_hip_lqr_set_gains), so only
    rounding in the loop is left.  Final x, u, t and steps of 8 dispersed starts vs the restatement's loop on oracle_simulate; bar
    1e-9 max|x| (the MPC closed-loop parity bar, tests/test_mpc.py).  The restatement's own result moves by 8e-15 .. 1.4e-13 of max|x| when
    every plant step is taken as two oracle_simulate calls of half the time step (generate_lqr_goldens.py measures it per case and stores it
    as <hold>_half_step_shift; asserted below the bar here), so the bar stands.  One more start holds a NaN: it retires at once with status -2, writes no non-finite output, and the other loops of the
    batch are bitwise what they are without it."""
    d = golden(name)
    assert float(d[f"{hold}_half_step_shift"]) < 1e-9
    _, o = device_gains(lqr_lib, name, d, hold)
    X, U, t = d[f"{hold}_X"][0], d[f"{hold}_U"][0], float(d[f"{hold}_t"][0])
    G = o["gains"][0]
    xs = d[f"{hold}_starts"]
    B = xs.shape[0] + 1
    bad = 3
    xs_nan = np.insert(xs, bad, xs[0], axis=0)
    xs_nan[bad, 1] = np.nan
    xs_ok = np.insert(xs, bad, xs[0], axis=0)
    res = []
    for starts in (xs_nan, xs_ok):
        c = context(lqr_lib, name, d, hold, B=B)
        c.set_trajectories(np.tile(X, (B, 1, 1)), np.tile(U, (B, 1, 1)), np.full(B, t))
        c.set_gains(np.tile(G, (B, 1, 1, 1)))
        n_finite = c.track(starts, X[-1], float(d["time_step"]), 20, 2000)
        res.append((n_finite, c.track_download()))
        c.close()
    (nf, r), (nf_ok, r_ok) = res
    assert nf == B - 1 and nf_ok == B
    assert r["status"][bad] == -2 and r["steps"][bad] == 0
    for key in r:
        assert np.isfinite(r[key]).all(), key
        keep = np.arange(B) != bad
        assert (r[key][keep] == r_ok[key][keep]).all(), key  # bitwise
    worst = 0.0
    for i in range(xs.shape[0]):
        j = i if i < bad else i + 1
        e = ref.track(MODELS[name], d["par"], X, U, G, t, xs[i], X[-1], float(d["time_step"]))
        assert r["status"][j] == 0 and r["steps"][j] == e["steps"]
        assert abs(r["t"][j] - e["t"]) <= 1e-12
        dx = np.abs(r["x"][j] - e["x"]).max() / np.abs(e["x"]).max()
        du = np.abs(r["u"][j] - e["u"]).max() / np.abs(e["u"]).max()
        worst = max(worst, dx, du)
        assert dx <= 1e-9 and du <= 1e-9, (i, dx, du)
        assert abs(r["err1"][j] - e["err1"]) <= 1e-9 * np.abs(e["x"]).max() and abs(r["err0"][j] - e["err0"]) <= 1e-12 * np.abs(e["x"]).max()
        assert abs(r["max_dev"][j] - e["max_dev"]) <= 1e-9 * np.abs(e["x"]).max()
    print(f"{name} {hold}: device loop vs restatement, worst relative difference {worst:.2e} (bar 1e-9)")


def test_nonfinite_reference_node_retires_without_nonfinite_output(lqr_lib):
    """a trajectory with a NaN node (a failed solver instance): its gain node is status -2 with zeros, its flight retires with status -2 when
    it reaches the node, keeps its last finite state AND input, and the other flight of the batch is bitwise unaffected"""
    d = golden("rocket2d")
    X, U, t = d["foh_X"].copy(), d["foh_U"].copy(), d["foh_t"]
    ok = context(lqr_lib, "rocket2d", d, "foh")
    ok.compute_gains()
    xs = X[:, 0].copy()
    ok.track(xs, X[0, -1], 0.01, 20, 2000)
    r_ok = ok.track_download()
    ok.close()
    X[1, 5, 4] = np.nan  # the tilt angle: enters the Jacobian
    c = context(lqr_lib, "rocket2d", d, "foh", B=2)
    c.set_trajectories(X, U, t)
    assert c.compute_gains() == 2 * X.shape[1] - 1
    g = c.download_gains()
    assert g["status"][1, 5] == -2 and (g["gains"][1, 5] == 0).all() and np.isfinite(g["gains"]).all()
    assert c.track(xs, X[0, -1], 0.01, 20, 2000) == 1
    r = c.track_download()
    c.close()
    assert r["status"].tolist() == [0, -2] and 0 < r["steps"][1] < r["steps"][0]
    for key in r:
        assert np.isfinite(r[key]).all(), key
        assert (r[key][0] == r_ok[key][0]).all(), key
    assert np.abs(r["u"][1]).max() > 0  # the last input that was applied, not a placeholder


# ---- T4 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hold", CASES)
def test_it_tracks(lqr_lib, name, hold):
    """Property test with the generator's margins: for the stored weights (set through scpp_hip_lqr_set_weights) and dispersed starts the
    RESTATEMENT ends within 1/4 of the open-loop (G = 0) final error for every start; the device, with its own gains, must end within 1/2
    of the stored open-loop error.  From the undisturbed start the largest |x - x_ref| stays within 2 x the restatement's."""
    d = golden(name)
    X, U, t = d[f"{hold}_X"][0], d[f"{hold}_U"][0], float(d[f"{hold}_t"][0])
    xs = np.vstack([d[f"{hold}_starts"], X[:1]])
    B = xs.shape[0]
    c = context(lqr_lib, name, d, hold, B=B)
    c.set_trajectories(np.tile(X, (B, 1, 1)), np.tile(U, (B, 1, 1)), np.full(B, t))
    assert c.compute_gains() == B * X.shape[0]
    assert c.track(xs, X[-1], float(d["time_step"]), 20, 2000) == B
    r = c.track_download()
    c.close()
    print(f"{name} {hold}: tracked {np.round(r['err1'][:-1], 3)} open loop {np.round(d[f'{hold}_err_open'], 2)}; undisturbed excursion "
          f"{r['max_dev'][-1]:.3e} (restatement {float(d[f'{hold}_undisturbed_max_dev']):.3e})")
    assert (d[f"{hold}_err_closed"] <= 0.25 * d[f"{hold}_err_open"]).all()
    assert (r["status"] == 0).all()
    assert (r["err1"][:-1] <= 0.5 * d[f"{hold}_err_open"]).all()
    assert r["max_dev"][-1] <= 2.0 * float(d[f"{hold}_undisturbed_max_dev"])


# ---- T5 ------------------------------------------------------------------------------------------------------------------------------------
def declared_lqr_symbols():
    text = open(os.path.join(ROOT, "include", "scpp_hip_lqr.h")).read()
    return sorted(set(re.findall(r"\b(scpp_hip_lqr_[a-z0-9_]+)\s*\(", text)))


def test_binding_covers_header():
    from scpp_amd import _lib

    assert sorted(_lib.LQR_SYMBOLS) == declared_lqr_symbols()
    assert len(_lib.LQR_SYMBOLS) >= 16


def test_header_symbols_exported(backend):
    name, lib, _ = backend
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    exported = sorted(set(re.findall(r"\b(scpp_hip_lqr_[a-z0-9_]+)\b", out)))
    assert exported == declared_lqr_symbols()
    h = ctypes.CDLL(lib)
    h.scpp_hip_lqr_version.restype = ctypes.c_char_p
    assert (b"gfx950" if name == "hip" else b"emulation") in h.scpp_hip_lqr_version()
    if name == "hip":
        blob = open(lib, "rb").read()
        assert b"gfx950" in blob and b"lqr_gain_kernel" in blob and b"lqr_track_kernel" in blob


def test_solver_library_identity_is_untouched():
    """the LQR component lives outside what tools/csrc_hash.py hashes: the committed PMC / parity summaries stay those of the solver sources"""
    import glob
    import json
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import csrc_hash

    newest = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_hbm_v*.json")))[-1]
    assert json.load(open(newest))["csrc_sha"] == csrc_hash.csrc_sha()


def test_abi_errors(lqr_lib):
    from scpp_amd import _lib

    L = _lib.load_lqr_library(lqr_lib)
    h = ctypes.c_void_p()
    E_ARG, E_STATE = -1, -4
    assert L.scpp_hip_lqr_create(ctypes.byref(h), 0, 7, 10, 1, 1) == E_ARG  # unknown model
    assert L.scpp_hip_lqr_create(ctypes.byref(h), 0, 1, 1, 1, 1) == E_ARG  # K < 2
    assert L.scpp_hip_lqr_create(ctypes.byref(h), 0, 1, 10, 0, 1) == E_ARG
    assert L.scpp_hip_lqr_create(None, 0, 1, 10, 1, 1) == E_ARG
    assert L.scpp_hip_lqr_destroy(None) == E_ARG
    d = golden("rocket2d")
    c = _lib.LqrContext(1, 30, 2, True, 0, lqr_lib)
    one6, one2 = np.ones(6), np.ones(2)
    p = _lib._p
    for q, r in ((np.array([1, 1, 1, 0, 1, 1.0]), one2), (one6, np.array([1.0, -2.0])), (one6, np.array([np.nan, 1.0]))):
        assert L.scpp_hip_lqr_set_weights(c.h, p(q), p(r)) == E_ARG  # a non-positive weight is refused, not clamped
    assert L.scpp_hip_lqr_compute_gains(c.h, None) == E_STATE  # nothing set yet
    c.set_flow_params(d["par"])
    assert L.scpp_hip_lqr_compute_gains(c.h, None) == E_STATE
    X, U, t = d["foh_X"], d["foh_U"], d["foh_t"]
    assert L.scpp_hip_lqr_set_trajectories(c.h, p(X), p(U), p(t), 3) == E_ARG  # B > batch_max
    c.set_trajectories(X, U, t)
    G = np.zeros((2, 30, 2, 6))
    assert L.scpp_hip_lqr_download_gains(c.h, p(G), None, None) == E_STATE
    xs = X[:, 0].copy()
    n = ctypes.c_int()
    args = lambda B, ts, sub, ms, nr, ws: (c.h, p(xs), p(X[0, -1].copy()), B, ts, sub, ms, nr, ws, ctypes.byref(n))  # noqa: E731
    assert L.scpp_hip_lqr_track(*args(2, 0.01, 20, 10, 0, 30)) == E_STATE  # no gains
    G[0, 0, 0, 0] = np.inf
    assert L.scpp_hip_lqr_set_gains(c.h, p(G)) == E_ARG
    c.set_gains(np.zeros_like(G))
    st = np.zeros((2, 30), dtype=np.int32)
    assert L.scpp_hip_lqr_download_gains(c.h, p(G), p(st), None) == E_STATE  # user-supplied gains carry no status
    for bad in (args(1, 0.01, 20, 10, 0, 30), args(2, 0.0, 20, 10, 0, 30), args(2, 0.01, 0, 10, 0, 30), args(2, 0.01, 20, 0, 0, 30),
                args(2, 0.01, 20, 10, 3, 30), args(2, 0.01, 20, 10, 1, 0)):
        assert L.scpp_hip_lqr_track(*bad) == E_ARG
    assert L.scpp_hip_lqr_track_download(c.h, *([None] * 8)) == E_STATE
    assert L.scpp_hip_lqr_set_stop_tolerance(c.h, ctypes.c_double(-1.0)) == E_ARG
    c3 = _lib.LqrContext(1, 30, 3, True, 0, lqr_lib)  # parameter rows for 2 instances, then 3 trajectories: refused, not read past the rows given
    c3.set_flow_params(np.tile(d["par"], (2, 1)))
    c3.set_trajectories(np.tile(X[:1], (3, 1, 1)), np.tile(U[:1], (3, 1, 1)), np.tile(t[:1], 3))
    assert L.scpp_hip_lqr_compute_gains(c3.h, None) == E_STATE
    c3.set_flow_params(np.tile(d["par"], (3, 1)))
    assert c3.compute_gains() == 90
    c3.close()
    assert L.scpp_hip_lqr_track(*args(2, 0.01, 20, 10, 0, 30)) == 0 and n.value == 2
    assert L.scpp_hip_lqr_track_record(c.h, None, None, None, None) == E_STATE  # nothing was recorded
    c.close()


@pytest.mark.parametrize("hold", ["foh", "zoh"])
def test_device_trajectories_of_a_solved_context_equal_the_upload_path(backend, hold, tmp_path):
    """A small SC batch is SOLVED on the solver library (device: K = 50, emulator: K = 8), then the tracker takes the buffers the solve left
    behind through scpp_hip_device_ptrs (redimensionalised on the device, U in the solver's own layout of K rows per trajectory) without a
    copy: gains, status and iteration counts are bitwise those computed from the downloaded X / U / sigma of the same context, and so is a
    short tracked flight.  zoh: SC.info with interpolate_input false, the tracker has K - 1 inputs and strides the solver's K rows."""
    import shutil

    import scpp_amd
    from scpp_amd import _lib

    name, lib, build_solver = backend
    cfg = tmp_path / "config"
    shutil.copytree(os.path.join(ROOT, "scpp_amd", "config"), cfg)
    if hold == "zoh":
        f = cfg / "RocketQuat" / "SC.info"
        txt = f.read_text()
        assert re.search(r"interpolate_input\s+true", txt)
        f.write_text(re.sub(r"interpolate_input\s+true", "interpolate_input false", txt))
    model = scpp_amd.RocketQuat(str(cfg)).loadParameters()
    B, K = 3, (50 if name == "hip" else 8)
    x0 = model.randomized_initial_states(B)
    alg = scpp_amd.SCAlgorithm(model, K=K, batch_max=B, device=0, library=build_solver()).initialize()
    assert bool(alg.opts.interpolate_input) == (hold == "foh")
    alg.solve(x0)
    sol = alg.getSolution()
    assert (sol["status"] == 0).all() and (sol["sc_iters"] > 0).all()
    assert np.abs(sol["X"][:, 0] - x0).max() <= 1e-9 * np.abs(x0).max()  # dimensional: the trajectory starts at the SI initial state
    U = sol["U"] if hold == "foh" else sol["U"][:, :-1]
    par = model.flow_params(nondimensionalize=False)
    q, r = scpp_amd.load_lqr_weights(model)

    def run(setter):
        c = _lib.LqrContext(0, K, B, hold == "foh", 0, lib)
        c.set_weights(q, r)
        c.set_flow_params(par)
        setter(c)
        n_ok = c.compute_gains()
        o = c.download_gains()
        c.track(x0, model.p.x_final, 0.01, 20, 40)
        return n_ok, o, c.track_download(), c

    n_up, up, fl_up, c_up = run(lambda c: c.set_trajectories(sol["X"], U, sol["sigma"]))
    c_up.close()
    dX, dU, dt = alg.ctx.device_ptrs()
    alg.ctx.synchronize()
    n_dev, dev, fl_dev, c_dev = run(lambda c: c.set_trajectories_device(dX, dU, dt, B, K))
    assert c_dev.lib.scpp_hip_lqr_set_trajectories_device(c_dev.h, dX, dU, dt, B, K - 2) == -1  # fewer rows than the tracker has inputs
    c_dev.close()
    alg.ctx.close()
    print(f"{name} {hold}: {n_dev} of {B * K} nodes converged, iterations {dev['iters'].min()}..{dev['iters'].max()}")
    assert n_dev == n_up and n_dev > 0
    for key in ("gains", "status", "iters"):
        assert (dev[key] == up[key]).all(), key
    for key in fl_up:
        assert (fl_dev[key] == fl_up[key]).all(), key


@pytest.mark.parametrize("name", ["rocketquat", "rocket2d"])
def test_batch_independence(lqr_lib, name):
    """instance b alone == instance b in a batch, bitwise: gains and the tracked flight"""
    d = golden(name)
    X, U, t = d["foh_X"], d["foh_U"], d["foh_t"]
    xs = np.stack([d["foh_starts"][0], d["foh_starts"][1]])
    c = context(lqr_lib, name, d, "foh")
    c.compute_gains()
    batch = c.download_gains()
    c.track(xs, X[0, -1], 0.01, 20, 300)
    tb = c.track_download()
    c.close()
    for b in range(2):
        c1 = context(lqr_lib, name, d, "foh", B=1)
        c1.set_trajectories(X[b:b + 1], U[b:b + 1], t[b:b + 1])
        c1.compute_gains()
        one = c1.download_gains()
        c1.track(xs[b:b + 1], X[0, -1], 0.01, 20, 300)
        t1 = c1.track_download()
        c1.close()
        assert (one["gains"][0] == batch["gains"][b]).all() and one["iters"][0].tolist() == batch["iters"][b].tolist()
        for key in t1:
            assert (t1[key][0] == tb[key][b]).all(), key
        assert t1["status"][0] == 1 and t1["steps"][0] == 300  # stopped by max_steps


def test_record_is_sized_by_n_record(lqr_lib):
    d = golden("rocket2d")
    X, U, t = d["foh_X"], d["foh_U"], d["foh_t"]
    c = context(lqr_lib, "rocket2d", d, "foh")
    c.compute_gains()
    xs = X[:, 0].copy()
    c.track(xs, X[0, -1], 0.01, 20, 2000, n_record=1, write_steps=30)
    r = c.track_download()
    rec = c.track_record()
    assert rec["X"].shape == (1, 67, 6) and rec["U"].shape == (1, 67, 2) and rec["t"].shape == (1, 67)
    n = int(rec["n"][0])
    assert n == (int(r["steps"][0]) + 29) // 30
    assert np.allclose(rec["t"][0, :n], 0.01 * (1 + 30 * np.arange(n)))
    # a second call with more instances and fewer rows
    c.track(xs, X[0, -1], 0.01, 20, 100, n_record=2, write_steps=50)
    rec = c.track_record()
    assert rec["X"].shape == (2, 2, 6) and rec["n"].tolist() == [2, 2]
    c.close()


def test_front_end_tracker(lqr_lib):
    """scpp_amd.LQRTracker: weights from LQR.info, gains at construction, getInput on the host == the input the device loop applied first"""
    import scpp_amd

    d = golden("rocket2d")
    m = scpp_amd.Rocket2D().loadParameters()
    q, r = scpp_amd.load_lqr_weights(m)
    assert q.tolist() == [1.0] * 6 and r.tolist() == [1e4, 1e-6]
    X, U, t = d["foh_X"], d["foh_U"], d["foh_t"]
    trk = scpp_amd.LQRTracker(m, X, U, t, library=lqr_lib)
    assert trk.n_ok == X.shape[0] * X.shape[1] and (trk.status == 0).all()
    xs = d["foh_starts"][:2]
    out = trk.track(xs, X[0, -1], max_steps=1)
    for b in range(2):
        u = trk.getInput(0.0, xs[b], b)
        assert np.abs(out["u"][b] - u).max() <= 1e-12 * np.abs(u).max()
    trk.close()


# ---- T6 ------------------------------------------------------------------------------------------------------------------------------------
def test_regulator_mode(lqr_lib):
    """LQRAlgorithm / LQRSim (Rocket2D): the gain at the operating point vs scipy under T1's rule, a short closed loop vs the restatement under
    T3's rule (u = -K (x - x_final) + u_eq on a constant two-node trajectory, stop at |x - x_final| < stop_tol)."""
    import scpp_amd

    m = scpp_amd.Rocket2D().loadParameters()
    alg = scpp_amd.LQRAlgorithm(m, library=lqr_lib).initialize()
    x_eq, u_eq = m.getOperatingPoint()
    par = m.flow_params()
    Ks = ref.scipy_gain(1, x_eq, u_eq, par, alg.Q, alg.R)
    Kr, it, st = ref.node_gain(1, x_eq, u_eq, par, alg.Q, alg.R)
    bar = 10.0 * max(np.abs(Kr - Ks).max() / np.abs(Ks).max(), np.finfo(float).eps)
    gap = np.abs(alg.K - Ks).max() / np.abs(Ks).max()
    print(f"operating point: device vs scipy {gap:.3e} (bar {bar:.3e}), {alg.iterations} iterations (restatement {it})")
    assert st == 0 and gap <= bar and abs(alg.iterations - it) <= 1
    x_final = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    xs = np.array([[3.0, 5.0, -0.5, -1.0, 0.02, 0.0], [-4.0, 2.0, 1.0, 0.5, -0.03, 0.01], [0.01, 0.0, 0.0, 0.0, 0.0, 0.0]])
    alg.setInitialState(xs)
    alg.setFinalState(x_final)
    alg.solve()
    assert np.allclose(alg.getSolution(), -(xs - x_final) @ alg.K.T + u_eq, rtol=0, atol=0)
    sim_time = 1.5
    out = scpp_amd.LQRSim(alg, sim_time=sim_time, stop_tol=0.02).run(xs, x_final)
    Xc, Uc = np.tile(x_final, (2, 1)), np.tile(u_eq, (2, 1))
    G = np.tile(alg.K, (2, 1, 1))
    for b in range(3):
        x, t, steps = xs[b].copy(), 0.0, 0
        while t < sim_time:  # LQR_sim.cpp:43-82 without the clipping
            u, _ = ref.get_input(Xc, Uc, G, sim_time, t, x)
            x = ref.oracle_lib.simulate(1, par, 0.01, u, u, x)
            t += 0.01
            steps += 1
            if np.linalg.norm(x - x_final) < 0.02:
                break
        assert out["steps"][b] == steps and out["status"][b] == 0
        assert np.abs(out["x"][b] - x).max() <= 1e-9 * max(np.abs(x).max(), 1.0)
        assert np.abs(out["u"][b] - u).max() <= 1e-9 * np.abs(u).max()
    assert out["steps"][2] == 1  # starts inside the tolerance: one step, like the reference's loop
    with pytest.raises(RuntimeError):
        scpp_amd.LQRAlgorithm(scpp_amd.RocketQuat().loadParameters(), library=lqr_lib)


# ---- T7 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.xdist_group("host_cpp")  # shares the build directory scpp_amd/host with tests/test_host_cpp.py
def test_sc_tracking_executable(backend, tmp_path):
    """host/sc_tracking --batch 4: SCAlgorithm trajectories, gains, four tracked flights; writes X.txt / U.txt / t.txt of instance 0 in the
    reference's output tree and exits 0.  (The emulation build runs K = 10 nodes: an emulated K = 50 solve takes minutes.)"""
    import glob

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
    r = subprocess.run(cmd + ["--batch", "4", "--config", os.path.join(ROOT, "scpp_amd", "config"), "--out", str(tmp_path)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "SC batch 4:" in r.stdout and "gains/s" in r.stdout and "steps/s" in r.stdout and "Final error:" in r.stdout
    run = glob.glob(str(tmp_path / "output" / "RocketQuat" / "SC_tracking" / "*" / "0"))[0]
    X = np.loadtxt(os.path.join(run, "X.txt"), delimiter=",", ndmin=2)
    U = np.loadtxt(os.path.join(run, "U.txt"), delimiter=",", ndmin=2)
    t = np.loadtxt(os.path.join(run, "t.txt"), ndmin=1)
    assert X.shape[1] == 14 and U.shape[1] == 4 and X.shape[0] == U.shape[0] == t.shape[0] > 10
    assert np.isfinite(X).all() and np.isfinite(U).all() and (np.diff(t) > 0).all()


def test_lqr_algorithm_header_compiles_for_rocket2d(tmp_path):
    """host/lqr_algorithm.hpp is for models with an operating point (Rocket2d); no shipped executable includes it, so it is compiled here"""
    src = tmp_path / "check.cpp"
    src.write_text('#include "lqr_algorithm.hpp"\nint main() { auto m = std::make_shared<Model>(); scpp::LQRAlgorithm a(m); a.initialize(); a.setInitialState({}); '
                   'a.setFinalState({}); a.solve(); Model::input_vector_t u; a.getSolution(u); return 0; }\n')
    host = os.path.join(ROOT, "scpp_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-DSCPP_ACTIVE_MODEL_ROCKET2D", "-I" + os.path.join(ROOT, "include"), "-I" + host, str(src)])

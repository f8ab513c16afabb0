"""Affine finite-horizon LQR (scpp_hip_lqr_compute_gains_affine, scpp_amd/csrc/lqr/lqr_affine_kernel.h; the FF loop of lqr_track_kernel): every
kernel test runs the SAME assertions on the CPU emulation of the kernel sources (`emu`) and, marked gpu, on the device library (`hip`).

Checkers (tests/lqr_affine_reference.py, no code shared with the kernels, and NOT the augmented matrix: the three equations for P, p and s as
written): the exact answer (DOP853, rtol 1e-12, stored by tests/golden/generate_lqr_affine_goldens.py) and the twin (numpy fixed-step RKF78 on
the oracle's Jacobians and flow map, run here, once per case for the whole module).
Inputs: the nominals of tests/golden/lqr_<model>.npz (`plain`: the defect is what linear interpolation leaves) and the generator's `bent` copies.

Bars: device vs twin 10 x gap_round (the twin against a copy with Jacobian and flow-map values perturbed by 1 ulp); device vs exact gap_scheme +
that; each relative to the largest magnitude of P, K, p, k, s over the trajectory, all measured by the generator with the reference alone.
Flights: 1e-9 of the largest entry, the bar of the tracker-vs-twin tests (test_lqr.py, test_lqr_saturation.py)."""
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN

import lqr_affine_reference as ar

MODELS = {"rocketquat": 0, "rocket2d": 1, "lander3dof": 2}
CASES = [("rocketquat", "foh"), ("rocketquat", "zoh"), ("rocket2d", "foh"), ("rocket2d", "zoh"), ("lander3dof", "foh"), ("lander3dof", "zoh")]
KINDS = ["plain", "bent"]
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
FIELDS = ("P", "K", "p", "k", "s")
E_ARG, E_UNSUPPORTED, E_STATE = -1, -3, -4


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


@functools.lru_cache(maxsize=None)
def golden(name):
    return dict(np.load(os.path.join(GOLDEN, f"lqr_{name}.npz")))


@functools.lru_cache(maxsize=None)
def agolden(name):
    return dict(np.load(os.path.join(GOLDEN, f"lqr_affine_{name}.npz")))


def nominal(name, hold, kind):
    d = golden(name)
    X = d[f"{hold}_X"] if kind == "plain" else agolden(name)[f"{hold}_Xbent"]
    return X, d[f"{hold}_U"], d[f"{hold}_t"]


@functools.lru_cache(maxsize=None)
def twin(name, hold, kind, b):
    """the twin of one trajectory: computed once, shared by every test and both backends, never modified"""
    import __graft_entry__ as g

    g.build_oracle()
    d = golden(name)
    X, U, t = nominal(name, hold, kind)
    return ar.twin(MODELS[name], d["par"], X[b], U[b], float(t[b]), d["q"], d["r"], steps=int(agolden(name)["steps"]))


def context(lib, name, hold, B):
    from scpp_amd import _lib

    d = golden(name)
    c = _lib.LqrContext(MODELS[name], d[f"{hold}_X"].shape[1], B, hold == "foh", 0, lib)
    c.set_weights(d["q"], d["r"])
    c.set_flow_params(d["par"])
    return c


def sweep(lib, name, hold, kind, steps=None, keep=True):
    X, U, t = nominal(name, hold, kind)
    c = context(lib, name, hold, X.shape[0])
    c.set_trajectories(X, U, t)
    n_ok = c.compute_gains_affine(int(agolden(name)["steps"]) if steps is None else steps, keep)
    o = c.download_gains()
    o.update(c.download_affine(keep))
    o["K"], o["k"] = o["gains"], o["ff"]
    return n_ok, o, c


def fly(c, xs, x_final, time_step, samples=1, n_record=0):
    n = c.track_samples(xs, x_final, samples, time_step, 20, 4000, n_record, 1) if samples > 1 else c.track(xs, x_final, time_step, 20, 4000, n_record, 1)
    out = c.track_download()
    out.update(c.track_download_saturation())
    out["n_finite"] = n
    if n_record:
        out["record"] = c.track_record()
    return out


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,hold", CASES)
def test_against_twin_and_exact(lqr_lib, name, hold, kind):
    """p, k, s, P and K of every node vs the twin (bar 10 x gap_round) and vs the exact answer (bar gap_scheme + that); status 0 everywhere,
    n_ok = B K, the count of node k is (K-1-k) steps.  The generator asserts that a twin with ONE tableau entry's sign flipped misses the bar
    for p by a factor >= 100 on the bent inputs."""
    g = agolden(name)
    steps = int(g["steps"])
    X, _, _ = nominal(name, hold, kind)
    B, K = X.shape[0], X.shape[1]
    n_ok, o, c = sweep(lqr_lib, name, hold, kind)
    c.close()
    assert all(np.isfinite(o[f]).all() for f in FIELDS)
    for b in range(B):
        tw = twin(name, hold, kind, b)
        for f in FIELDS:
            ex = g[f"{hold}_{kind}_{f}_exact"][b]
            rb = 10.0 * float(g[f"{hold}_{kind}_gap_round_{f}"][b])
            eb = float(g[f"{hold}_{kind}_gap_scheme_{f}"][b]) + rb
            gt, ge = ar.rel_gap(o[f][b], tw[f]), ar.rel_gap(o[f][b], ex)
            print(f"{name} {hold} {kind} {b} {f}: vs twin {gt:.2e} (bar {rb:.2e}), vs exact {ge:.2e} (bar {eb:.2e})")
            assert gt <= rb, (f, gt, rb)
            assert ge <= eb, (f, ge, eb)
    assert (o["status"] == 0).all() and n_ok == B * K
    assert (o["iters"] == (K - 1 - np.arange(K)) * steps).all()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,hold", CASES)
def test_p_and_k_are_the_riccati_sweeps(lqr_lib, name, hold, kind):
    """P and K are np.array_equal to those of compute_gains_riccati at the same steps: the augmentation adds only the products p 0 and 0 p to
    them.  Status and counts are equal too."""
    _, o, c = sweep(lqr_lib, name, hold, kind)
    c.compute_gains_riccati(int(agolden(name)["steps"]), True)
    r, P = c.download_gains(), c.download_riccati()
    c.close()
    assert np.array_equal(o["P"], P) and np.array_equal(o["K"], r["gains"])
    assert np.array_equal(o["status"], r["status"]) and np.array_equal(o["iters"], r["iters"])


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,hold", CASES)
def test_structure(lqr_lib, name, hold, kind):
    """p[K-1], s[K-1] and ff[K-1] are exactly zero.  [[P, p], [p', s]] is symmetric: P to the bit; of p the library hands out ONE copy, row nx
    of the tile, while k_k = R^-1 B_k'p is formed from the other, column nx, so the two copies are compared through it: k against
    R^-1 B_k'p(row) with the oracle's B_k, to the rounding of that product, (nx + 2) eps R^-1 |B_k|'|p|.  V >= 0: s >= 0 and
    s - p'P^-1 p >= 0 up to the rounding bar of s (10 x gap_round_s of max|s|)."""
    import oracle_lib

    d = golden(name)
    X, U, _ = nominal(name, hold, kind)
    g = agolden(name)
    _, o, c = sweep(lqr_lib, name, hold, kind)
    c.close()
    B, K = o["P"].shape[:2]
    for b in range(B):
        assert (o["p"][b, K - 1] == 0).all() and o["s"][b, K - 1] == 0 and (o["ff"][b, K - 1] == 0).all()
        assert np.array_equal(o["P"][b], o["P"][b].transpose(0, 2, 1))
        for k in range(K):
            _, _, Bk = oracle_lib.flow(MODELS[name], X[b, k], U[b, min(k, U.shape[1] - 1)], d["par"])
            want, bound = (Bk.T @ o["p"][b, k]) / d["r"], (X.shape[2] + 2) * np.finfo(float).eps * (np.abs(Bk).T @ np.abs(o["p"][b, k])) / d["r"]
            assert (np.abs(o["ff"][b, k] - want) <= bound).all(), (b, k, o["ff"][b, k], want, bound)
        bar = 10.0 * float(g[f"{hold}_{kind}_gap_round_s"][b]) * np.abs(o["s"][b]).max()
        vmin = np.array([o["s"][b, k] - o["p"][b, k] @ np.linalg.solve(o["P"][b, k], o["p"][b, k]) for k in range(K)])
        print(f"{name} {hold} {kind} {b}: min s {o['s'][b].min():.3e}, min (s - p'P^-1 p) {vmin.min():.3e}, bar {bar:.2e}")
        assert (o["s"][b] >= -bar).all()
        assert (vmin >= -bar).all()


# ---- 4, 6 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hold", CASES)
def test_flights_and_cost(lqr_lib, name, hold):
    """On the bent nominal 0, three flights per trajectory (samples = 3: from X[0], and from two dispersed starts) under the device's own gains
    and terms, without and with input limits, against the numpy twin of the loop fed the same downloaded arrays: final x, last u, steps, n_sat
    to the flight bar.  Then the point of the feature: the flight from x_start = X[0], recorded at every step, costs what the twin loop under
    the twin's gains costs (J_ff, J_noff of the generator) to within what a record moved by the flight bar can move the cost
    (lqr_affine_reference.cost(moved=...)), and J_ff <= 0.5 J_noff holds for the device as the generator asserts it of the reference.  The gap
    between J_ff and s0 is printed; it measures the plant's nonlinearity and has no bar."""
    d, g = golden(name), agolden(name)
    m = MODELS[name]
    Xa, Ua, ta = nominal(name, hold, "bent")
    X, U, T = Xa[0], Ua[0], float(ta[0])
    dtp = float(d["time_step"])
    n_ok, o, c = sweep(lqr_lib, name, hold, "bent", keep=False)
    G, ff = o["K"], o["ff"]
    starts = np.stack([[Xa[b, 0], Xa[b, 0] + 0.25 * (d[f"{hold}_starts"][0] - d[f"{hold}_X"][0, 0]), Xa[b, 0] + 0.25 * (d[f"{hold}_starts"][1] - d[f"{hold}_X"][0, 0])]
                       for b in range(Xa.shape[0])]).reshape(-1, Xa.shape[2])
    import scpp_amd

    model = {"rocketquat": scpp_amd.RocketQuat, "rocket2d": scpp_amd.Rocket2D, "lander3dof": scpp_amd.Lander3dof}[name]().loadParameters()
    # the model's limits with T_max drawn in to 97 % of the largest nominal thrust, so that the clip acts on these flights (T_min follows where
    # the thrust-vector rule needs T_min <= T_max cos(angle_max))
    lim = scpp_amd.lqr.model_input_limits(model)
    thrust = np.abs(U[:, 1]).max() if name == "rocket2d" else np.linalg.norm(U[:, :3], axis=1).max()
    lim[1] = min(lim[1], 0.97 * thrust)
    lim[0] = min(lim[0], 0.5 * lim[1] * np.cos(lim[2]))
    worst, sat_seen = 0.0, False
    for limits in (None, lim):
        c.set_input_limits(limits)
        c.set_feedforward(1)
        r = fly(c, starts[:3 * Xa.shape[0]], X[-1], dtp, samples=3)
        assert r["n_finite"] == starts.shape[0]
        for f in range(3):  # the fan of trajectory 0
            e = ar.track(m, d["par"], X, U, G[0], ff[0], T, starts[f], X[-1], lim=limits, time_step=dtp)
            assert r["status"][f] == 0 and r["steps"][f] == e["steps"]
            dx = np.abs(r["x"][f] - e["x"]).max() / np.abs(e["x"]).max()
            du = np.abs(r["u"][f] - e["u"]).max() / np.abs(e["u"]).max()
            worst = max(worst, dx, du)
            assert dx <= 1e-9 and du <= 1e-9, (f, limits, dx, du)
            assert r["n_sat"][f] == e["n_sat"], (f, r["n_sat"][f], e["n_sat"])
            sat_seen = sat_seen or e["n_sat"] > 0
    assert sat_seen  # the limits did clip: the FF loop's SAT instantiation was exercised
    c.set_input_limits(None)
    J = {}
    for mode in (1, 0):
        c.set_feedforward(mode)
        r = fly(c, Xa[:, 0], X[-1], dtp, n_record=1)
        n = int(r["record"]["n"][0])
        rx, ru = r["record"]["X"][0, :n], r["record"]["U"][0, :n]
        J[mode] = ar.cost(X, U, T, d["q"], d["r"], d["q"], X[0], rx, ru, dtp)
        Jt = float(g[f"{hold}_J_ff" if mode else f"{hold}_J_noff"][0])
        bar = ar.cost(X, U, T, d["q"], d["r"], d["q"], X[0], rx, ru, dtp, moved=(1e-9 * np.abs(rx).max(), 1e-9 * np.abs(ru).max()))
        print(f"{name} {hold}: feedforward {mode}: device cost {J[mode]:.6e}, twin {Jt:.6e}, apart {abs(J[mode] - Jt):.2e} (bar {bar:.2e})")
        assert abs(J[mode] - Jt) <= bar
    c.close()
    s0 = float(g[f"{hold}_s0"][0])
    print(f"{name} {hold}: flights vs twin {worst:.2e} (bar 1e-9); J_ff {J[1]:.4e} = {J[1] / J[0]:.3f} J_noff; predicted s0 {s0:.4e}, J_ff / s0 = {J[1] / s0:.3f}")
    assert float(g[f"{hold}_J_ff"][0]) <= 0.5 * float(g[f"{hold}_J_noff"][0])
    assert J[1] <= 0.5 * J[0]


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hold", [("rocketquat", "foh"), ("rocket2d", "zoh"), ("lander3dof", "foh")])
def test_off_means_off(lqr_lib, name, hold):
    """After the affine sweep with mode 0 the flights are array_equal to those under the Riccati gains; in mode 1 with
    set_feedforward_terms(zeros) they are equal (==) too; with the sweep's own terms they differ."""
    d = golden(name)
    Xa, Ua, ta = nominal(name, hold, "bent")
    xs = Xa[:, 0] + 0.25 * (d[f"{hold}_starts"][0] - d[f"{hold}_X"][0, 0])
    dtp = float(d["time_step"])
    _, o, c = sweep(lqr_lib, name, hold, "bent", keep=False)
    keys = ("x", "u", "t", "steps", "status", "err1", "max_dev")
    c.set_feedforward(1)
    on = fly(c, xs, Xa[0, -1], dtp)
    c.set_feedforward(0)
    off = fly(c, xs, Xa[0, -1], dtp)
    c.set_feedforward(1)
    c.set_feedforward_terms(np.zeros_like(o["ff"]))
    zero = fly(c, xs, Xa[0, -1], dtp)
    c.compute_gains_riccati(int(agolden(name)["steps"]))
    c.set_feedforward(0)
    ric = fly(c, xs, Xa[0, -1], dtp)
    c.close()
    for k in keys:
        assert np.array_equal(off[k], ric[k]), k
        assert (zero[k] == ric[k]).all(), k
    assert not np.array_equal(on["x"], ric["x"])


# ---- 7 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,steps", [(2, 1), (2, 3), (3, 1), (3, 2)])
def test_smallest_shapes(lqr_lib, K, steps):
    """K = 2 (one segment) and K = 3, steps = 1, B = 1: the first K nodes of the bent Rocket2D nominal against the twin run here on the same
    nodes, to 10 x the twin's own rounding floor measured here as the generator measures it (against a copy perturbed by 1 ulp), and never
    below 10 ulp of the array's largest entry: with one or two segments the perturbation, which acts on the right-hand sides only, can leave
    an array untouched (k of a two-node trajectory) or nearly so (K, whose largest entry is node K-1's R^-1 B'Qf), while the device and the
    twin still round the node's own product B'[P | p], nx terms and one scaling, in different orders."""
    from scpp_amd import _lib

    d = golden("rocket2d")
    Xa, Ua, ta = nominal("rocket2d", "foh", "bent")
    X, U = Xa[0, :K].copy(), Ua[0, :K].copy()
    T = float(ta[0]) * (K - 1) / (Xa.shape[1] - 1)
    c = _lib.LqrContext(1, K, 1, True, 0, lqr_lib)
    c.set_weights(d["q"], d["r"])
    c.set_flow_params(d["par"])
    c.set_trajectories(X[None], U[None], [T])
    assert c.compute_gains_affine(steps, True) == K
    o = c.download_gains()
    o.update(c.download_affine(True))
    c.close()
    o["K"], o["k"] = o["gains"], o["ff"]
    tw = ar.twin(1, d["par"], X, U, T, d["q"], d["r"], steps=steps)
    tp = ar.twin(1, d["par"], X, U, T, d["q"], d["r"], steps=steps, perturb=ar.ulp_perturb(np.random.default_rng(K * 10 + steps)))
    for f in FIELDS:
        gap, floor = ar.rel_gap(o[f][0], tw[f]), ar.rel_gap(tp[f], tw[f])
        floor = max(floor, float(np.finfo(float).eps))
        print(f"K = {K}, steps = {steps}, {f}: device vs twin {gap:.2e} (bar {10 * floor:.2e})")
        assert gap <= 10.0 * floor, (f, gap, floor)
    assert o["iters"].tolist() == [[(K - 1 - k) * steps for k in range(K)]] and (o["status"] == 0).all()


@pytest.mark.parametrize("name", ["rocket2d", "rocketquat"])
def test_nan_node_in_the_middle_trajectory(lqr_lib, name):
    """a batch of 3 with a NaN node in the middle trajectory: its outputs are zeros with status -2, nothing non-finite is downloaded, and its
    neighbours are bitwise what they are alone"""
    Xa, Ua, ta = nominal(name, "foh", "bent")
    K = Xa.shape[1]
    X = np.stack([Xa[0], Xa[1], Xa[1]])
    U = np.stack([Ua[0], Ua[1], Ua[1]])
    t = np.array([ta[0], ta[1], ta[1]])
    X[1, K // 2, 2] = np.nan

    def run(Xs, Us, ts):
        c = context(lqr_lib, name, "foh", Xs.shape[0])
        c.set_trajectories(Xs, Us, ts)
        n = c.compute_gains_affine(3, True)
        o = c.download_gains()
        o.update(c.download_affine(True))
        c.close()
        return n, o

    n, o = run(X, U, t)
    assert n == 2 * K
    keys = ("gains", "ff", "P", "p", "s", "iters")
    assert all(np.isfinite(o[k]).all() for k in keys)
    assert (o["status"][1] == -2).all() and all((o[k][1] == 0).all() for k in keys)
    for b in (0, 2):
        _, one = run(X[b:b + 1], U[b:b + 1], t[b:b + 1])
        assert (one["status"] == 0).all()
        for k in keys + ("status",):
            assert np.array_equal(one[k][0], o[k][b]), (b, k)


def test_nonfinite_flow_map_of_a_finite_node(lqr_lib):
    """Rocket2D with every node finite and a non-finite defect: a position of -1e308 at node 11 makes the slope (X[12] - X[11]) / dt of
    segment 11 overflow, so c = f - dX/dt is -inf there while the reference itself is finite.  Nodes 0..11 get status -2 and zeros, nodes
    12.. keep status 0; nothing non-finite is written."""
    name = "rocket2d"
    Xa, Ua, ta = nominal(name, "foh", "bent")
    K = Xa.shape[1]
    X = Xa[:1].copy()
    X[0, 11, 0] = -1e308
    c = context(lqr_lib, name, "foh", 1)
    c.set_trajectories(X, Ua[:1], ta[:1])
    n = c.compute_gains_affine(2, True)
    o = c.download_gains()
    o.update(c.download_affine(True))
    c.close()
    assert all(np.isfinite(o[k]).all() for k in ("gains", "ff", "P", "p", "s"))
    assert (o["status"][0, :12] == -2).all() and (o["status"][0, 12:] == 0).all() and n == K - 12
    assert all((o[k][0, :12] == 0).all() for k in ("gains", "ff", "P", "p", "s", "iters"))


def device_copies(backend_name, lib, arrays):
    """(pointers, free) of copies of `arrays` the library can read as device memory: on the emulator the arrays themselves, on the device
    hipMalloc + hipMemcpy of the HIP runtime the LQR library is linked against, reached through the library's own handle"""
    from scpp_amd import _lib

    if backend_name == "emu":
        return [a.ctypes.data for a in arrays], lambda: None
    C = ctypes
    rt = _lib.load_lqr_library(lib)
    rt.hipMalloc.argtypes, rt.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
    rt.hipMemcpy.argtypes, rt.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    rt.hipFree.argtypes, rt.hipFree.restype = [C.c_void_p], C.c_int
    ptrs = []
    for a in arrays:
        q = C.c_void_p()
        assert rt.hipMalloc(C.byref(q), a.nbytes) == 0 and q.value
        assert rt.hipMemcpy(q, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice
        ptrs.append(q.value)
    return ptrs, lambda: [rt.hipFree(q) for q in ptrs]


def test_device_pointer_path_zero_order_hold_u_rows_k(backend):
    """the device-pointer path with a zero-order-hold context and u_rows = K (a solver context's layout: K input rows per trajectory, the last
    one unused, NaN here): bitwise the result of the copying path"""
    bname, lib, _ = backend
    name = "lander3dof"
    Xa, Ua, ta = nominal(name, "zoh", "bent")
    K = Xa.shape[1]
    _, want, c0 = sweep(lib, name, "zoh", "bent")
    c0.close()
    Upad = np.concatenate([Ua, np.full((Ua.shape[0], 1, Ua.shape[2]), np.nan)], axis=1)
    host = [np.array(v, dtype=np.float64, order="C") for v in (Xa, Upad, ta)]
    ptrs, free = device_copies(bname, lib, host)
    c = context(lib, name, "zoh", Xa.shape[0])
    c.set_trajectories_device(*ptrs, Xa.shape[0], K)
    assert c.compute_gains_affine(int(agolden(name)["steps"]), True) == Xa.shape[0] * K
    o = c.download_gains()
    o.update(c.download_affine(True))
    c.close()
    free()
    for k in ("gains", "status", "iters", "ff", "P", "p", "s"):
        assert np.array_equal(o[k], want[k]), k


# ---- 8 -------------------------------------------------------------------------------------------------------------------------------------
def test_abi(lqr_lib):
    """every SCPP_E_* answer and every invalidation of the four entry points, mode 1 with hold 1 and mode 1 without terms included"""
    from scpp_amd import _lib

    L = _lib.load_lqr_library(lqr_lib)
    d = golden("rocket2d")
    X, U, t = nominal("rocket2d", "foh", "bent")
    p = _lib._p
    n = ctypes.c_int()
    B, K = X.shape[0], X.shape[1]
    ffb, Pb, pb, sb = np.zeros((B, K, 2)), np.zeros((B, K, 6, 6)), np.zeros((B, K, 6)), np.zeros((B, K))
    c = _lib.LqrContext(1, K, B, True, 0, lqr_lib)
    c.set_weights(d["q"], d["r"])
    aff = L.scpp_hip_lqr_compute_gains_affine
    dl = L.scpp_hip_lqr_download_affine
    terms = L.scpp_hip_lqr_set_feedforward_terms
    xs, xf = np.ascontiguousarray(X[:, 0]), np.ascontiguousarray(X[0, -1])

    def track():
        return L.scpp_hip_lqr_track(c.h, p(xs), p(xf), B, 0.01, 20, 10, 0, 1, None)

    assert aff(c.h, 5, 0, ctypes.byref(n)) == E_STATE  # nothing set yet
    c.set_flow_params(d["par"])
    assert aff(c.h, 5, 0, ctypes.byref(n)) == E_STATE  # no trajectories
    c.set_trajectories(X, U, t)
    for steps in (0, -3):
        assert aff(c.h, steps, 0, ctypes.byref(n)) == E_ARG
    assert aff(None, 5, 0, None) == E_ARG
    assert dl(None, None, None, None, None) == E_ARG
    assert dl(c.h, p(ffb), None, None, None) == E_STATE  # nothing computed
    assert terms(c.h, p(ffb)) == E_STATE  # no gains
    assert terms(None, p(ffb)) == E_ARG and terms(c.h, None) == E_ARG
    for mode in (2, -1):
        assert L.scpp_hip_lqr_set_feedforward(c.h, mode) == E_ARG
    assert L.scpp_hip_lqr_set_feedforward(None, 1) == E_ARG
    # a sweep without keep: ff yes, P / p / s no
    assert aff(c.h, 5, 0, ctypes.byref(n)) == 0 and n.value == B * K
    assert dl(c.h, p(ffb), None, None, None) == 0 and np.abs(ffb).max() > 0
    assert dl(c.h, None, None, None, None) == 0
    for args in ((p(Pb), None, None), (None, p(pb), None), (None, None, p(sb))):
        assert dl(c.h, None, *args) == E_STATE
    assert L.scpp_hip_lqr_download_riccati(c.h, p(Pb)) == E_STATE  # not a Riccati sweep
    assert aff(c.h, 5, 1, None) == 0
    assert dl(c.h, p(ffb), p(Pb), p(pb), p(sb)) == 0 and np.abs(pb).max() > 0 and np.abs(sb).max() > 0 and np.abs(Pb).max() > 0
    # mode 1: flies with terms, refuses the held loop, and goes back
    assert L.scpp_hip_lqr_set_feedforward(c.h, 1) == 0
    assert track() == 0
    c.set_feedback_hold(1)
    assert track() == E_UNSUPPORTED
    c.set_feedback_hold(0)
    assert track() == 0
    # every other gain computation, set_gains, new flow parameters and new trajectories drop the terms
    G = c.download_gains()["gains"]
    for drop in ("frozen", "riccati", "discrete", "set_gains", "par", "traj"):
        assert aff(c.h, 5, 1, None) == 0 and track() == 0
        if drop == "frozen":
            c.compute_gains()
        elif drop == "riccati":
            c.compute_gains_riccati(5)
        elif drop == "discrete":
            c.compute_gains_discrete(5)
        elif drop == "set_gains":
            c.set_gains(G)
        elif drop == "par":
            c.set_flow_params(d["par"])
            c.set_gains(G)  # computed gains went with the parameters: the loop has gains again, and still no terms
        else:
            c.set_trajectories(X, U, t)
            c.set_gains(G)
        assert dl(c.h, p(ffb), None, None, None) == E_STATE, drop
        assert track() == E_STATE, drop  # mode 1 without terms
        c.set_feedforward(0)
        assert track() == 0, drop
        c.set_feedforward(1)
    # user-supplied terms for user-supplied gains
    c.set_gains(G)
    bad = np.zeros((B, K, 2))
    bad[1, 3, 1] = np.inf
    assert terms(c.h, p(bad)) == E_ARG
    bad[1, 3, 1] = np.nan
    assert terms(c.h, p(bad)) == E_ARG
    assert track() == E_STATE
    assert terms(c.h, p(np.zeros((B, K, 2)))) == 0
    assert track() == 0
    assert dl(c.h, p(ffb), None, None, None) == E_STATE  # the terms are the caller's, no affine sweep is held
    # user-supplied terms stay with user gains when new parameters arrive?  No: parameters define the defect
    c.set_flow_params(d["par"])
    assert track() == E_STATE
    c.close()


# ---- 9 -------------------------------------------------------------------------------------------------------------------------------------
def test_front_end_tracker(lqr_lib):
    """scpp_amd.LQRTracker(horizon="affine") == the C ABI's arrays; track() applies the term by default and feedforward=False flies the Riccati
    loop; getInput includes the term when it is on; the refused horizons stay refused"""
    import scpp_amd

    d = golden("rocket2d")
    X, U, t = nominal("rocket2d", "foh", "bent")
    m = scpp_amd.Rocket2D().loadParameters()
    _, abi, c = sweep(lqr_lib, "rocket2d", "foh", "bent")
    c.close()
    trk = scpp_amd.LQRTracker(m, X, U, t, library=lqr_lib, horizon="affine", keep_affine=True)
    a = trk.affine()
    assert trk.n_ok == X.shape[0] * X.shape[1] and (trk.status == 0).all()
    assert np.array_equal(trk.gains, abi["gains"]) and np.array_equal(trk.iterations, abi["iters"])
    for k in ("ff", "P", "p", "s"):
        assert np.array_equal(a[k], abi[k]), k
    on = trk.track(X[:, 0], X[0, -1])
    off = trk.track(X[:, 0], X[0, -1], feedforward=False)
    assert (on["status"] == 0).all() and (on["max_dev"] < off["max_dev"]).all()
    x = X[0, 3] + 0.1
    tq = 0.37 * float(t[0])
    u1, u0 = trk.getInput(tq, x), trk.getInput(tq, x, feedforward=False)
    import lqr_reference

    want = lqr_reference.get_input(X[0], U[0], trk.gains[0], float(t[0]), tq, x)[0]
    kt = ar.feedforward_at(a["ff"][0], X.shape[1], U.shape[1], float(t[0]), tq)
    assert np.abs(u0 - want).max() <= 1e-12 * np.abs(want).max() and np.abs(u1 - (want - kt)).max() <= 1e-12 * np.abs(want).max()
    with pytest.raises(Exception):
        trk.track(X[:, 0], X[0, -1], hold="node")  # feedforward with the held loop: unsupported
    trk.close()
    fin = scpp_amd.LQRTracker(m, X, U, t, library=lqr_lib, horizon="finite")
    ric = fin.track(X[:, 0], X[0, -1])
    with pytest.raises(RuntimeError):
        fin.affine()
    with pytest.raises(RuntimeError):
        fin.track(X[:, 0], X[0, -1], feedforward=True)
    fin.close()
    for k in ("x", "u", "steps", "max_dev"):
        assert np.array_equal(off[k], ric[k]), k
    trk2 = scpp_amd.LQRTracker(m, X, U, t, library=lqr_lib, horizon="affine")
    assert set(trk2.affine()) == {"ff"}
    trk2.close()
    for h in ("receding", "sampled"):
        with pytest.raises(ValueError):
            scpp_amd.LQRTracker(m, X, U, t, library=lqr_lib, horizon=h)

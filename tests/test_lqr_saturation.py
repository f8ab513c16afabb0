"""Input limits inside the tracking loop (scpp_hip_lqr_set_input_limits) and sample fans (scpp_hip_lqr_track_samples): every test runs the
SAME assertions on the CPU emulation of the kernel sources (`emu`) and, marked gpu, on the device library (`hip`).

Checker: tests/lqr_saturation_reference.py (the rule on Python floats, lqr_reference's loop with sat after get_input, flight f along
trajectory f // samples); it shares no code with the kernels.  Inputs: tests/golden/lqr_<model>.npz, cut to K = 5 nodes by
test_lqr_batch_layout.hetero (three trajectories that differ in nodes, flight time and parameter row), and for the property test the
covariance golden.  Bars: bitwise wherever two device computations must agree; the projection 4 ulp (the rule is a dozen correctly rounded
operations, written so that none is fused); flights 1e-9 relative (the bar of test_lqr_batch_layout.py and test_lqr.py); n_sat exact, which
is fair because the cases assert, on the twin alone, that no commanded input comes within 1e-6 T_max of a limit."""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN

import lqr_covariance_reference as cr
import lqr_saturation_reference as sr
from test_lqr_batch_layout import MODELS, hetero, new_context, same

NAMES = ["rocketquat", "rocket2d", "lander3dof"]
HOLDS = ["foh", "zoh"]
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
E_ARG, E_STATE = -1, -4
FLIGHT_KEYS = ("x", "u", "t", "steps", "status", "err0", "err1", "max_dev")


@pytest.fixture(scope="module", params=BACKENDS)
def lqr_lib(request):
    """the LQR library of the emulation build or of the device build"""
    import __graft_entry__ as g

    g.build_oracle()
    if request.param == "emu":
        return g.build_lqr_emu()
    lib = os.environ.get("SCPP_LQR_LIBRARY") or g.LQR_LIB
    if not os.path.exists(lib):
        g.build_lqr()
    return lib


def fly(c, xs, x_final, samples=1, max_steps=200, n_record=0, write_steps=1):
    """one fan on context c: the flight outputs, the two saturation outputs and, with n_record, the record"""
    n = c.track_samples(xs, x_final, samples, 0.01, 20, max_steps, n_record, write_steps)
    o = c.track_download()
    o.update(c.track_download_saturation())
    o["n_finite"] = n
    if n_record:
        o["record"] = c.track_record()
    return o


def ulps(a, b):
    """|a - b| in units of the spacing of b, entry by entry (0 where both are equal)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.where(a == b, 0.0, np.abs(a - b) / np.spacing(np.maximum(np.abs(b), np.finfo(float).tiny)))


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------
def probes(name, lim, n=200):
    """a fixed-seed cloud of n inputs around the input set of lim: directions inside and outside the cone at magnitudes from below T_min
    to above T_max, points computed to lie on each face, and u = 0, u_xy = 0"""
    t_min, t_max, ang = lim
    rng = np.random.default_rng(20261018)
    if name == "rocket2d":
        P = np.stack([ang * rng.choice([0.0, 0.3, 0.9, 1.0, 1.1, 3.0], n) * rng.choice([-1.0, 1.0], n) * rng.uniform(0.9, 1.1, n),
                      t_max * rng.choice([-0.5, 0.0, 0.2, 0.6, 1.0, 1.7], n) * rng.uniform(0.9, 1.1, n)], axis=1)
        P[:6] = [[0.0, 0.0], [ang, t_max], [-ang, t_min], [0.0, t_min], [ang, 0.5 * (t_min + t_max)], [0.5 * ang, t_max]]
        return P
    nu = 4 if name == "rocketquat" else 3
    tilt = ang * rng.choice([0.0, 0.2, 0.8, 1.0, 1.3, 2.5, 4.0], n) * rng.uniform(0.95, 1.05, n)
    az = rng.uniform(0.0, 2.0 * math.pi, n)
    mag = t_max * rng.choice([0.05, 0.3, 0.7, 1.0, 1.4, 5.0], n) * rng.uniform(0.9, 1.1, n)
    P = np.zeros((n, nu))
    P[:, 0], P[:, 1], P[:, 2] = mag * np.sin(tilt) * np.cos(az), mag * np.sin(tilt) * np.sin(az), mag * np.cos(tilt)
    if nu == 4:
        P[:, 3] = rng.standard_normal(n) * t_max  # the roll torque: any value passes through
    mid = 0.5 * (t_min + t_max)
    P[:8, :3] = [[0.0, 0.0, 0.0], [0.0, 0.0, mid], [0.0, 0.0, t_min], [0.0, 0.0, t_max], [math.tan(ang) * mid, 0.0, mid],
                 [0.0, -math.tan(ang) * mid, mid], [t_max * math.sin(ang), 0.0, t_max * math.cos(ang)], [0.3 * t_min, 0.0, -t_max]]
    return P


@pytest.mark.parametrize("name", NAMES)
def test_projection_alone(lqr_lib, name):
    """sat() by itself: 200 probe inputs, each the constant input of a two-node zero-order-hold 'trajectory' with a zero gain, one plant
    step each (u_cmd = -0 (x - x_ref) + U[0] is the probe to the bit).  out_u against the twin's saturate at 4 ulp; every result satisfies
    the three constraints to 1e-12 T_max; the probes the twin returns unchanged come back bitwise; a second pass over the results moves
    them by at most 4 ulp; n_sat is 1 exactly where the twin moves the probe, and max_clip is that distance."""
    m = MODELS[name]
    d = np.load(os.path.join(GOLDEN, f"lqr_{name}.npz"))
    lim = np.array([1.0e5, 3.0e5, 0.3])
    P = probes(name, lim)
    n, nu = P.shape
    x0 = d["zoh_X"][0, 0]
    from scpp_amd import _lib

    c = _lib.LqrContext(m, 2, n, False, 0, lqr_lib)
    c.set_flow_params(d["par"])
    c.set_input_limits(lim)

    def one_step(Uin):
        c.set_trajectories(np.tile(x0, (n, 2, 1)), Uin.reshape(n, 1, nu), np.ones(n))
        c.set_gains(np.zeros((n, 2, nu, x0.size)))
        o = fly(c, np.tile(x0, (n, 1)), x0, max_steps=1)
        assert (o["steps"] == 1).all() and (o["status"] == 1).all(), (o["steps"], o["status"])  # one step, then the step cap
        return o

    o1 = one_step(P)
    tw = np.array([sr.saturate(m, p, lim) for p in P])
    worst = float(ulps(o1["u"], tw).max())
    viol = max(sr.violation(m, u, lim) for u in o1["u"])
    inside = (tw == P).all(axis=1)
    print(f"{name}: {n} probes, {int(inside.sum())} inside the set; device vs twin {worst:.1f} ulp (bar 4), worst constraint violation "
          f"{viol:.2e} (bar {1e-12 * lim[1]:.1e})")
    assert 20 <= inside.sum() <= n - 100  # the cloud does land inside and outside
    assert worst <= 4.0
    assert viol <= 1e-12 * lim[1]
    assert same(o1["u"][inside], P[inside])
    assert (o1["n_sat"] == (~inside).astype(np.int32)).all()
    clip = np.sqrt(((P - tw) ** 2).sum(axis=1))
    assert np.abs(o1["max_clip"] - clip).max() <= 1e-12 * lim[1] and (o1["max_clip"][inside] == 0.0).all()
    if nu == 4:
        assert same(o1["u"][:, 3], P[:, 3])  # the fourth input passes through
    o2 = one_step(o1["u"])
    c.close()
    again = float(ulps(o2["u"], o1["u"]).max())
    print(f"{name}: sat(sat(u)) vs sat(u) {again:.1f} ulp (bar 4)")
    assert again <= 4.0


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------
_cases = {}
FACTOR_T, FACTOR_ANGLE, SEED = 0.95, 0.9, 6  # chosen on the twin alone so that the preconditions of test_flights_against_the_twin hold in all six cases


def biting_case(lqr_lib, name, hold):
    """B = 2 trajectories of K = 5 (hetero), 2 dispersed starts each (1 % Gaussian on node 0), Riccati gains of the library under test, and
    one limits row PER TRAJECTORY that bites: T_max = FACTOR_T x the largest thrust the unlimited twin commands on that trajectory's two
    flights, angle_max = FACTOR_ANGLE x the largest commanded angle (thrust-vector models: the tilt of the thrust vector; Rocket2D: the
    gimbal), T_min = half the smallest commanded axial thrust.  Computed once per case and shared; nobody writes to it."""
    key = (lqr_lib, name, hold)
    if key in _cases:
        return _cases[key]
    m, K, B, S = MODELS[name], 5, 2, 2
    h = hetero(name, hold, K)
    X, U, t, par = h["X"][:B], h["U"][:B], h["t"][:B], h["par"][:B]
    c = new_context(lqr_lib, name, hold, K, B, h, rows=slice(0, B))
    c.set_trajectories(X, U, t)
    assert c.compute_gains_riccati(2) == B * K
    G = c.download_gains()["gains"]
    c.close()
    xs = np.repeat(X[:, 0], S, axis=0)
    xs = xs * (1.0 + 0.01 * np.random.default_rng(SEED).standard_normal(xs.shape))
    x_final = h["X"][0, -1]
    free = sr.fan(m, par, X, U, G, t, xs, x_final, S, None, 0.01, 200)
    lim = np.zeros((B, 3))
    for b in range(B):
        Ua = np.concatenate([free[f]["U_applied"] for f in range(b * S, (b + 1) * S)])
        if name == "rocket2d":
            thrust, axial, angle = Ua[:, 1], Ua[:, 1], np.abs(Ua[:, 0])
        else:
            thrust, axial = np.linalg.norm(Ua[:, :3], axis=1), Ua[:, 2]
            angle = np.arctan2(np.linalg.norm(Ua[:, :2], axis=1), Ua[:, 2])
        lim[b] = [0.5 * max(axial.min(), 0.0), FACTOR_T * thrust.max(), FACTOR_ANGLE * angle.max()]
    tw = sr.fan(m, par, X, U, G, t, xs, x_final, S, lim, 0.01, 200)
    out = dict(m=m, K=K, B=B, S=S, h=h, X=X, U=U, t=t, par=par, G=G, xs=xs, x_final=x_final, lim=lim, free=free, twin=tw)
    _cases[key] = out
    return out


@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_flights_against_the_twin(lqr_lib, name, hold):
    """The biting case, flown as one fan with the record of every step.  Preconditions, on the twin alone: every flight has
    0 < n_sat < steps, and no commanded input lies within 1e-6 T_max of a limit (sr.margin; Rocket2D's gimbal limit is an angle: within
    1e-6 angle_max) -- so a last-bit difference in u_cmd cannot flip a clip decision and n_sat is compared exactly.  Device against twin: n_sat
    equal, steps equal, max_clip, final x and last u to 1e-9 (relative to the largest entry; the unlimited loop measures 4e-16), every
    recorded input inside the set to 1e-12 T_max, and the recorded inputs are the twin's applied inputs to 1e-9."""
    k = biting_case(lqr_lib, name, hold)
    m, S, lim, tw = k["m"], k["S"], k["lim"], k["twin"]
    F = k["B"] * S
    for f, e in enumerate(tw):
        assert e["status"] == 0 and 0 < e["n_sat"] < e["steps"] <= 200, (f, e["n_sat"], e["steps"], e["status"])
        assert e["min_margin"] > 1e-6, (f, e["min_margin"])
    c = new_context(lqr_lib, name, hold, k["K"], k["B"], k["h"], rows=slice(0, k["B"]))
    c.set_trajectories(k["X"], k["U"], k["t"])
    c.set_gains(k["G"])
    c.set_input_limits(lim)
    o = fly(c, k["xs"], k["x_final"], S, 200, n_record=F, write_steps=1)
    c.close()
    assert o["n_finite"] == F and (o["status"] == 0).all()
    for f, e in enumerate(tw):
        row = lim[f // S]
        dx = np.abs(o["x"][f] - e["x"]).max() / np.abs(e["x"]).max()
        du = np.abs(o["u"][f] - e["u"]).max() / np.abs(e["u"]).max()
        dc = abs(o["max_clip"][f] - e["max_clip"]) / e["max_clip"]
        n = int(o["record"]["n"][f])
        Ur = o["record"]["U"][f, :n]
        viol = max(sr.violation(m, u, row) for u in Ur)
        dr = np.abs(Ur - e["U_applied"]).max() / np.abs(e["U_applied"]).max()
        print(f"{name} {hold} flight {f}: {e['steps']} steps, n_sat {o['n_sat'][f]} (twin {e['n_sat']}), max_clip {o['max_clip'][f]:.6g}, "
              f"vs twin x {dx:.2e} u {du:.2e} clip {dc:.2e} record {dr:.2e} (bar 1e-9), worst violation {viol:.2e}, twin margin {e['min_margin']:.3g}")
        assert o["steps"][f] == e["steps"] == n and o["n_sat"][f] == e["n_sat"]
        assert dx <= 1e-9 and du <= 1e-9 and dc <= 1e-9 and dr <= 1e-9, (f, dx, du, dc, dr)
        assert viol <= 1e-12 * row[1], (f, viol)
        # the bar tells the limited loop from the unlimited one: the largest clip is >= 1e-4 of the inputs the record is compared in, 1e5 bars
        assert e["max_clip"] >= 1e-4 * np.abs(e["U_applied"]).max()


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_nothing_changes_when_nothing_clips(lqr_lib, name, hold):
    """With limits unset, track_samples(samples = 1) is bitwise track, and n_sat = max_clip = 0.  With limits so wide that the twin reports
    n_sat == 0 on every flight (T_min = 0, T_max = 10 x the largest commanded thrust, angle_max = 1.5 rad), every output is bitwise the
    unlimited flight's and n_sat == 0, max_clip == 0."""
    k = biting_case(lqr_lib, name, hold)
    m, B = k["m"], k["B"]
    xs = k["xs"][::k["S"]]  # one start per trajectory
    c = new_context(lqr_lib, name, hold, k["K"], B, k["h"], rows=slice(0, B))
    c.set_trajectories(k["X"], k["U"], k["t"])
    c.set_gains(k["G"])
    assert c.track(xs, k["x_final"], 0.01, 20, 200) == B
    plain = c.track_download()
    plain.update(c.track_download_saturation())
    fan = fly(c, xs, k["x_final"], 1)
    for key in FLIGHT_KEYS + ("n_sat", "max_clip"):
        assert same(plain[key], fan[key]), key
    assert (plain["n_sat"] == 0).all() and (plain["max_clip"] == 0.0).all()
    big = max(np.abs(e["U_applied"]).max() for e in k["free"])
    wide = np.array([0.0, 10.0 * big, 1.5])
    tw = sr.fan(m, k["par"], k["X"], k["U"], k["G"], k["t"], xs, k["x_final"], 1, wide, 0.01, 200)
    assert all(e["n_sat"] == 0 and e["status"] == 0 for e in tw)
    c.set_input_limits(wide)
    lo = fly(c, xs, k["x_final"], 1)
    c.close()
    for key in FLIGHT_KEYS:
        assert same(plain[key], lo[key]), key
    assert (lo["n_sat"] == 0).all() and (lo["max_clip"] == 0.0).all()
    assert (plain["steps"] > 50).all()


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hold", [("rocketquat", "foh"), ("rocket2d", "zoh"), ("lander3dof", "foh")])
def test_fan_layout(lqr_lib, name, hold):
    """B = 3 heterogeneous trajectories (own nodes, flight time, parameter row, limits row), samples = 22: 66 flights, a full block of 64
    plus two, with the trajectory boundaries (flights 22, 44) inside a block.  Limits row b: T_max = (0.97 - 0.02 b) x the trajectory's
    largest nominal thrust, angle_max = (0.6 + 0.1 b) x its largest nominal angle (a floor of 1e-3), T_min = 0.
    Flights 0, 21, 22, 43, 63, 64, 65 are each bitwise what a batch_max = 1, samples = 1 context computes from that trajectory's rows and
    that start, limits on; the limits clip on every trajectory.  With limits off the whole fan is bitwise the replicated batch, 66 copies
    of X, U, t, G and par through scpp_hip_lqr_track.
    The mutation this is for: indexing the limits row or the parameter row by the flight f instead of the trajectory f / samples (or the
    other way round for x_start and the outputs).  Flights 21 and 22, 43 and 63 sit on either side of a boundary and get different rows."""
    m, K, B, S = MODELS[name], 5, 3, 22
    F = B * S
    h = hetero(name, hold, K)
    X, U, t, par = h["X"], h["U"], h["t"], h["par"]
    lim = np.zeros((B, 3))
    for b in range(B):
        if name == "rocket2d":
            thrust, angle = U[b][:, 1].max(), np.abs(U[b][:, 0]).max()
        else:
            thrust = np.linalg.norm(U[b][:, :3], axis=1).max()
            angle = np.arctan2(np.linalg.norm(U[b][:, :2], axis=1), U[b][:, 2]).max()
        lim[b] = [0.0, (0.97 - 0.02 * b) * thrust, max((0.6 + 0.1 * b) * angle, 1e-3)]
    c = new_context(lqr_lib, name, hold, K, B, h)
    c.set_trajectories(X, U, t)
    assert c.compute_gains_riccati(2) == B * K
    G = c.download_gains()["gains"]
    xs = np.repeat(X[:, 0], S, axis=0)
    xs = xs * (1.0 + 0.01 * np.random.default_rng(66).standard_normal(xs.shape))
    x_final = X[0, -1]
    off = fly(c, xs, x_final, S)
    c.set_input_limits(lim)
    on = fly(c, xs, x_final, S)
    c.close()
    assert on["n_finite"] == off["n_finite"] == F and (on["status"] == 0).all() and (off["status"] == 0).all()
    assert (off["n_sat"] == 0).all() and all((on["n_sat"][b * S:(b + 1) * S] > 0).any() for b in range(B))
    print(f"{name}: flights clipped per trajectory {[int((on['n_sat'][b * S:(b + 1) * S] > 0).sum()) for b in range(B)]} of {S}, steps "
          f"{sorted(set(on['steps'].tolist()))}")
    for f in (0, 21, 22, 43, 63, 64, 65):
        b = f // S
        c1 = new_context(lqr_lib, name, hold, K, 1, h, rows=slice(b, b + 1))
        c1.set_trajectories(X[b:b + 1], U[b:b + 1], t[b:b + 1])
        c1.set_gains(G[b:b + 1])
        c1.set_input_limits(lim[b])
        one = fly(c1, xs[f:f + 1], x_final, 1)
        c1.close()
        for key in FLIGHT_KEYS + ("n_sat", "max_clip"):
            assert same(one[key][0], on[key][f]), (f, key)
    rep = np.arange(F) // S
    hr = dict(h, par=par[rep])
    cr_ = new_context(lqr_lib, name, hold, K, F, hr)
    cr_.set_trajectories(X[rep], U[rep], t[rep])
    cr_.set_gains(G[rep])
    assert cr_.track(xs, x_final, 0.01, 20, 200) == F
    replicated = cr_.track_download()
    cr_.close()
    for key in FLIGHT_KEYS:
        assert same(replicated[key], off[key]), key


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------
def test_abi(lqr_lib):
    """The refused limits rows, samples = 0, a limits batch of 2 against 3 trajectories, download_saturation before a flight, NULL restores
    bitwise-unlimited flights, limits invalidate neither gains nor a covariance sweep, and a small fan, a larger one (the flight buffers
    grow past batch_max) and the small one again give the same rows."""
    from scpp_amd import _lib

    L = _lib.load_lqr_library(lqr_lib)
    p = _lib._p
    name, hold, K, B = "rocketquat", "foh", 5, 3
    h = hetero(name, hold, K)
    c = new_context(lqr_lib, name, hold, K, B, h)
    ns, mc = np.zeros(B, dtype=np.int32), np.zeros(B)
    assert L.scpp_hip_lqr_track_download_saturation(c.h, p(ns), p(mc)) == E_STATE  # no flight yet
    c.set_trajectories(h["X"], h["U"], h["t"])
    assert c.compute_gains_riccati(2) == B * K
    gains = c.download_gains()
    c.set_covariance_inputs(h["S0"], h["w"])
    assert c.propagate_covariance(2, True) == B
    cov = c.download_covariance(True)
    assert L.scpp_hip_lqr_track_download_saturation(c.h, p(ns), p(mc)) == E_STATE
    good = [1.0e5, 4.0e5, 0.3]
    nan, inf = float("nan"), float("inf")
    refused = [[nan, 4e5, 0.3], [1e5, inf, 0.3], [1e5, 4e5, nan], [-1.0, 4e5, 0.3], [1e5, 1e5, 0.3], [2e5, 1e5, 0.3], [1e5, 4e5, 0.0],
               [1e5, 4e5, -0.1], [1e5, 4e5, math.pi / 2], [1e5, 4e5, 2.0], [3.9e5, 4e5, 0.3]]  # the last: T_min > T_max cos(angle_max)
    for row in refused:
        a = np.array(row)
        assert L.scpp_hip_lqr_set_input_limits(c.h, p(a), 1) == E_ARG, row
        a3 = np.array([good, row, good])
        assert L.scpp_hip_lqr_set_input_limits(c.h, p(a3), 3) == E_ARG, row
    a = np.array(good)
    assert L.scpp_hip_lqr_set_input_limits(c.h, p(a), 0) == E_ARG and L.scpp_hip_lqr_set_input_limits(c.h, p(a), B + 1) == E_ARG
    # T_min > T_max cos(angle_max) is a condition of the thrust-vector rule only: the box of Rocket2D takes it
    c2 = _lib.LqrContext(MODELS["rocket2d"], 2, 1, True, 0, lqr_lib)
    a2 = np.array([3.9e5, 4e5, 0.3])
    assert L.scpp_hip_lqr_set_input_limits(c2.h, p(a2), 1) == 0
    c2.close()

    xs = np.repeat(h["X"][:, 0], 2, axis=0) * (1.0 + 0.01 * np.random.default_rng(9).standard_normal((2 * B, h["X"].shape[2])))
    xf = np.ascontiguousarray(h["X"][0, -1])
    n = ctypes.c_int()

    def raw(xs_, Bt, samples):
        return L.scpp_hip_lqr_track_samples(c.h, p(np.ascontiguousarray(xs_)), p(xf), Bt, samples, 0.01, 20, 200, 0, 1, ctypes.byref(n))

    assert raw(xs, B, 0) == E_ARG and raw(xs, B, -1) == E_ARG
    assert raw(xs, 2, 3) == E_ARG  # B is the number of trajectories
    free = fly(c, xs, xf, 2)
    two = np.array([good, good])
    assert L.scpp_hip_lqr_set_input_limits(c.h, p(two), 2) == 0  # accepted here, judged at launch like the flow parameters
    assert raw(xs, B, 2) == E_STATE
    assert L.scpp_hip_lqr_track(c.h, p(np.ascontiguousarray(xs[::2])), p(xf), B, 0.01, 20, 200, 0, 1, ctypes.byref(n)) == E_STATE
    tight = np.array([0.0, 3.0e5, 0.005])
    c.set_input_limits(tight)
    lim_on = fly(c, xs, xf, 2)
    assert (lim_on["n_sat"] > 0).all() and (lim_on["max_clip"] > 0).all() and not same(lim_on["x"], free["x"])
    # new trajectories do not clear the limits
    c.set_trajectories(h["X"], h["U"], h["t"])
    c.set_gains(gains["gains"])
    again = fly(c, xs, xf, 2)
    for key in FLIGHT_KEYS + ("n_sat", "max_clip"):
        assert same(again[key], lim_on[key]), key
    c.set_input_limits(None)
    back = fly(c, xs, xf, 2)
    for key in FLIGHT_KEYS + ("n_sat", "max_clip"):
        assert same(back[key], free[key]), key
    c.close()

    # limits leave gains and a covariance sweep as they are
    c = new_context(lqr_lib, name, hold, K, B, h)
    c.set_trajectories(h["X"], h["U"], h["t"])
    assert c.compute_gains_riccati(2) == B * K
    c.set_covariance_inputs(h["S0"], h["w"])
    assert c.propagate_covariance(2, True) == B
    c.set_input_limits(tight)
    g2, cov2 = c.download_gains(), c.download_covariance(True)
    for key in gains:
        assert same(g2[key], gains[key]), key
    for key in cov:
        assert same(cov2[key], cov[key]), key
    # a small fan, a larger one, the small one again
    small = fly(c, xs, xf, 2)
    S = 30
    xl = np.repeat(h["X"][:, 0], S, axis=0) * (1.0 + 0.01 * np.random.default_rng(10).standard_normal((S * B, h["X"].shape[2])))
    xl[::S] = xs[::2]  # the first flight of every trajectory is the small fan's
    large = fly(c, xl, xf, S)
    assert large["x"].shape[0] == S * B and large["n_finite"] == S * B
    small2 = fly(c, xs, xf, 2)
    c.close()
    for key in FLIGHT_KEYS + ("n_sat", "max_clip"):
        assert same(small[key], small2[key]), key
        assert same(small[key][::2], large[key][::S]), key
    for key in FLIGHT_KEYS + ("n_sat", "max_clip"):
        assert same(small[key], lim_on[key]), key


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------------
def test_sigma_point_fan_with_and_without_limits(lqr_lib):
    """What the feature is for (Rocket2D).  Along the dynamically exact golden nominal the 2 nx + 1 sigma-point starts of the covariance
    cross-check (test_lqr_covariance.py) are flown as ONE fan of 13 flights on ONE trajectory.  Limits wide (nothing clips): the
    sigma-point covariance agrees with the sweep's S(T) within the cross-check's own bar, twice the stored xc_gap -- the fan is a drop-in
    for the replicated batch there.  Limits tight (T_max and the gimbal limit inside the range the unlimited flights command): n_sat > 0,
    and the final spread differs from the unlimited one by more than that same bar -- the linear answer no longer describes the loop."""
    name = "rocket2d"
    d = np.load(os.path.join(GOLDEN, f"lqr_{name}.npz"))
    cg = np.load(os.path.join(GOLDEN, f"lqr_covariance_{name}.npz"))
    from scpp_amd import _lib

    X, U, t, G = d["foh_X"][:1], d["foh_U"][:1], d["foh_t"][:1], d["foh_G_ref"][:1]
    eps, S0 = float(cg["xc_eps"]), cg["sigma0"]
    xs = cr.sigma_point_starts(X[0, 0], S0, eps)
    F = xs.shape[0]
    c = _lib.LqrContext(MODELS[name], X.shape[1], 1, True, 0, lqr_lib)
    c.set_weights(d["q"], d["r"])
    c.set_flow_params(d["par"])
    c.set_trajectories(X, U, t)
    c.set_gains(G)
    ts = float(d["time_step"])
    c.set_input_limits([0.0, 10.0 * np.abs(U[0][:, 1]).max(), 1.5])
    n = c.track_samples(xs, X[0, -1], F, ts, 20, 2000)
    wide = c.track_download()
    wide.update(c.track_download_saturation())
    c.set_covariance_inputs(S0, None)
    assert c.propagate_covariance(int(cg["steps"]), False) == 1
    sweep = c.download_covariance(False)
    assert n == F and (wide["status"] == 0).all() and (wide["n_sat"] == 0).all()
    bar = 2.0 * float(cg["xc_gap"])
    S_wide = cr.sigma_point_covariance(wide["x"], eps)
    gap = cr.rel_gap(S_wide, sweep["final_cov"][0])
    c.set_input_limits(tight_limits_2d(U[0]))
    assert c.track_samples(xs, X[0, -1], F, ts, 20, 2000) == F
    tight = c.track_download()
    tight.update(c.track_download_saturation())
    c.close()
    S_tight = cr.sigma_point_covariance(tight["x"], eps)
    moved = cr.rel_gap(S_tight, S_wide)
    print(f"{name}: fan of {F} sigma-point flights vs sweep {gap:.3e} (bar {bar:.3e}); with tight limits n_sat {tight['n_sat'].tolist()}, "
          f"spread moved by {moved:.3e} of max|S(T)| (must exceed the bar)")
    assert gap <= bar
    assert (tight["status"] == 0).all() and (tight["n_sat"] > 0).all()
    assert moved > bar


def tight_limits_2d(U):
    """limits inside the nominal's own range of Rocket2D inputs (gimbal, thrust): thrust between the 25th and 60th percentile of the
    nominal thrust, gimbal within 30 % of its largest nominal deflection"""
    return np.array([np.percentile(U[:, 1], 25), np.percentile(U[:, 1], 60), 0.3 * np.abs(U[:, 0]).max()])

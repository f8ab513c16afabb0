"""Process noise in the tracking loop (scpp_hip_lqr_set_disturbance, scpp_hip_lqr_disturbance_normals): every test that touches the library
runs the SAME assertions on the CPU emulation of the kernel sources (`emu`) and, marked gpu, on the device library (`hip`).

Checker: tests/lqr_disturbance_reference.py (Philox4x32-10 on Python ints, Box-Muller with `math`, a numpy RKF78 over the oracle's flow map
plus d, the loop rules of the other reference modules); it shares no code with the kernels.  Inputs: tests/golden/lqr_<model>.npz, cut to
K = 5 nodes by test_lqr_batch_layout.hetero, and for the dispersion test the dynamically exact Lander3dof nominal itself.

Bars.  Normals against the twin 1e-13 absolute: |rho| <= 8.6, the argument of cos is rounded to 9e-16, libm is good to a few ulp, times 10.
Moments of 1.8 M normals: five standard errors of each estimator.  Flights against the twin 1e-9 relative to the largest entry, the suite's
flight bar; n_sat exact, fair because the cases assert on the twin alone that no commanded input comes within 1e-6 T_max of a limit.
Bitwise wherever two device computations must agree.  The dispersion statistic: five standard deviations of a chi-square with 6 N degrees
of freedom."""
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN

import lqr_disturbance_reference as dr
import oracle_lib
from lqr_discrete_reference import segment_and_fraction
from test_lqr_batch_layout import MODELS, hetero, new_context, same

NAMES = ["rocketquat", "rocket2d", "lander3dof"]
HOLDS = ["foh", "zoh"]
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
E_ARG = -1
FLIGHT_KEYS = ("x", "u", "t", "steps", "status", "err0", "err1", "max_dev")
ALL_KEYS = FLIGHT_KEYS + ("n_sat", "max_clip")
SEED = 0x1234_5678_9ABC_DEF1  # both key words in use


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


def fly(c, xs, x_final, samples=1, substeps=4, max_steps=200, n_record=0, write_steps=1, time_step=0.01):
    """one fan on context c: the flight outputs, the two saturation outputs and, with n_record, the record"""
    n = c.track_samples(xs, x_final, samples, time_step, substeps, max_steps, n_record, write_steps)
    o = c.track_download()
    o.update(c.track_download_saturation())
    o["n_finite"] = n
    if n_record:
        o["record"] = c.track_record()
    return o


def rel(a, b):
    """largest |a - b| relative to the largest |b| (0 where both vanish)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    s = np.abs(b).max()
    return float(np.abs(a - b).max() / s) if s > 0 else float(np.abs(a).max())


# ---- 1. the twin is right --------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """Philox4x32-10 of the twin against the three known answers (counter and key all zero, all ones, and the digits of pi)"""
    h = lambda c: " ".join("%08x" % v for v in c)  # noqa: E731
    assert h(dr.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert h(dr.philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert h(dr.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    assert 0.0 < dr.uniform(0, 0) == 2.0 ** -53 and dr.uniform(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53 < 1.0


@pytest.mark.parametrize("name", NAMES)
def test_twin_plant_step_without_noise_is_the_oracles(name):
    """plant_step with d = 0 and the oracle's 20 substeps against oracle_lib.simulate, five steps in a row from golden node 0: 1e-13 relative"""
    import __graft_entry__ as g

    g.build_oracle()
    d = np.load(os.path.join(GOLDEN, f"lqr_{name}.npz"))
    x, u = d["foh_X"][0, 0], d["foh_U"][0, 0]
    xa, xb = x.copy(), x.copy()
    for _ in range(5):
        xa = dr.plant_step(MODELS[name], d["par"], xa, u, np.zeros_like(x), 0.01, 20)
        xb = oracle_lib.simulate(MODELS[name], d["par"], 0.01, u, u, xb)
    gap = rel(xa, xb)
    print(f"{name}: twin plant step vs oracle_simulate {gap:.2e} (bar 1e-13)")
    assert gap <= 1e-13


# ---- 2. the generator alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_normals_against_the_twin(lqr_lib, name):
    """flights {0, 1, 2, 2^32 + 1} x steps {0..3, 10^6} at the model's nx: 1e-13 absolute"""
    from scpp_amd import _lib

    c = _lib.LqrContext(MODELS[name], 2, 1, True, 0, lqr_lib)
    worst = 0.0
    for g0, ng in ((0, 3), (2 ** 32 + 1, 1)):
        for s0, ns in ((0, 4), (10 ** 6, 1)):
            z = c.disturbance_normals(SEED, g0, ng, s0, ns)
            tw = dr.normals_block(SEED, range(g0, g0 + ng), range(s0, s0 + ns), c.nx)
            assert z.shape == tw.shape == (ng, ns, c.nx)
            worst = max(worst, float(np.abs(z - tw).max()))
    c.close()
    print(f"{name}: nx = {c.nx}, normals vs twin {worst:.2e} (bar 1e-13)")
    assert worst <= 1e-13


def test_normals_moments(lqr_lib):
    """flights 0..4095, steps 0..63, nx = 7 (n = 1.8 M): mean, variance, lag-1 correlation along each of the three indices and the share of
    |z| > 3, each within five standard errors"""
    from scpp_amd import _lib

    c = _lib.LqrContext(MODELS["lander3dof"], 2, 1, True, 0, lqr_lib)
    z = c.disturbance_normals(SEED, 0, 4096, 0, 64)
    c.close()
    n = z.size
    assert z.shape == (4096, 64, 7) and np.isfinite(z).all()
    mean, var = float(z.mean()), float((z * z).mean())
    lag = [float((z[1:] * z[:-1]).mean()), float((z[:, 1:] * z[:, :-1]).mean()), float((z[:, :, 1:] * z[:, :, :-1]).mean())]
    p3 = math.erfc(3.0 / math.sqrt(2.0))
    tail = float((np.abs(z) > 3.0).mean())
    print(f"n = {n}: mean {mean:.2e} (bar {5 / math.sqrt(n):.2e}), variance - 1 {var - 1:.2e} (bar {5 * math.sqrt(2 / n):.2e}), lag-1 correlation "
          f"along f, n, r {lag[0]:.2e} {lag[1]:.2e} {lag[2]:.2e}, P(|z| > 3) {tail:.5f} (expected {p3:.5f}, bar {5 * math.sqrt(p3 * (1 - p3) / n):.1e})")
    assert abs(mean) <= 5.0 / math.sqrt(n)
    assert abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / n)
    for v in lag:
        assert abs(v) <= 5.0 / math.sqrt(n)
    assert abs(p3 - 0.0027) < 1e-5 and abs(tail - p3) <= 5.0 * math.sqrt(p3 * (1.0 - p3) / n)


# ---- 3. scale, deterministically -------------------------------------------------------------------------------------------------------------
def test_scale_of_one_plant_step(lqr_lib):
    """Lander3dof (x = m, r, v), one plant step of 0.01 s in 20 substeps, a constant input (two-node zero-order-hold 'trajectory', zero gain), w on the
    three velocities only, 8 flights.  The velocity slopes depend on neither r nor v and the mass is not disturbed, so noise on minus noise
    off is dv = sqrt(w time_step) z (1e-12 of the largest entry) and dr = 0.5 sqrt(w / time_step) z time_step^2 (1e-9: RKF78 integrates the
    linear velocity difference exactly); the mass is bitwise the same."""
    from scpp_amd import _lib

    name, F, ts = "lander3dof", 8, 0.01
    g = np.load(os.path.join(GOLDEN, f"lqr_{name}.npz"))
    x0, u0 = g["zoh_X"][0, 0], g["zoh_U"][0, 0]
    w = np.array([0.0, 0.0, 0.0, 0.0, 1.0e4, 2.5e3, 4.0e4])
    c = _lib.LqrContext(MODELS[name], 2, 1, False, 0, lqr_lib)
    c.set_flow_params(g["par"])
    c.set_trajectories(np.tile(x0, (1, 2, 1)), u0.reshape(1, 1, -1), np.ones(1))
    c.set_gains(np.zeros((1, 2, u0.size, x0.size)))
    xs = np.tile(x0, (F, 1))
    off = fly(c, xs, x0, F, 20, 1)
    c.set_disturbance(w, SEED, 5)
    on = fly(c, xs, x0, F, 20, 1)
    c.close()
    assert (on["steps"] == 1).all() and (off["steps"] == 1).all() and (on["status"] == 1).all()
    z = dr.normals_block(SEED, range(5, 5 + F), [0], 7)[:, 0, 4:]
    dv, dpos = on["x"][:, 4:] - off["x"][:, 4:], on["x"][:, 1:4] - off["x"][:, 1:4]
    ev = np.sqrt(w[4:] * ts) * z
    er = 0.5 * np.sqrt(w[4:] / ts) * z * ts * ts
    print(f"dv vs sqrt(w dt) z {rel(dv, ev):.2e} (bar 1e-12), dr vs d dt^2 / 2 {rel(dpos, er):.2e} (bar 1e-9), largest dv {np.abs(ev).max():.3g}")
    assert rel(dv, ev) <= 1e-12
    assert rel(dpos, er) <= 1e-9
    assert same(on["x"][:, 0], off["x"][:, 0])


# ---- 4. flights against the twin -------------------------------------------------------------------------------------------------------------
VARIANTS = ["plain", "limits", "hold", "feedforward"]
_cases = {}


def noise_w(X, zero=1):
    """a disturbance that moves every state but one by about 1 % of its scale per sqrt(second): w_r = (0.01 max |X[.., r]|)^2, a state that is
    zero along the nominal counts as 1; w[zero] = 0"""
    s = np.abs(X).reshape(-1, X.shape[-1]).max(axis=0)
    w = (0.01 * np.where(s > 0, s, 1.0)) ** 2
    w[zero] = 0.0
    return w


def flight_case(name, hold, variant):
    """B = 3 heterogeneous trajectories of K = 5, two 1 % dispersed starts each, substeps = 4, at most 200 plant steps.  The gains (and the
    feedforward terms) come from the emulation build whatever library is under test, so the twin's flights are computed once per case and
    shared; nobody writes to them.  plain: Riccati gains.  limits: the same under one limits row per trajectory, T_max = (0.97 - 0.02 b) x
    the largest nominal thrust, angle_max = (0.6 + 0.1 b) x the largest nominal angle, T_min = 0 (test_fan_layout's rows).  hold: discrete
    gains, the correction latched per segment.  feedforward: affine gains with their term."""
    key = (name, hold, variant)
    if key in _cases:
        return _cases[key]
    import __graft_entry__ as g

    emu = g.build_lqr_emu()
    m, K, B, S = MODELS[name], 5, 3, 2
    h = hetero(name, hold, K, B)
    X, U, t, par = h["X"], h["U"], h["t"], h["par"]
    c = new_context(emu, name, hold, K, B, h)
    c.set_trajectories(X, U, t)
    ff = lim = None
    if variant == "hold":
        assert c.compute_gains_discrete(2) == B * K
    elif variant == "feedforward":
        assert c.compute_gains_affine(2) == B * K
        ff = c.download_affine()["ff"]
    else:
        assert c.compute_gains_riccati(2) == B * K
    G = c.download_gains()["gains"]
    c.close()
    if variant == "limits":
        lim = np.zeros((B, 3))
        for b in range(B):
            if name == "rocket2d":
                thrust, angle = U[b][:, 1].max(), np.abs(U[b][:, 0]).max()
            else:
                thrust = np.linalg.norm(U[b][:, :3], axis=1).max()
                angle = np.arctan2(np.linalg.norm(U[b][:, :2], axis=1), U[b][:, 2]).max()
            lim[b] = [0.0, (0.97 - 0.02 * b) * thrust, max((0.6 + 0.1 * b) * angle, 1e-3)]
    xs = np.repeat(X[:, 0], S, axis=0)
    xs = xs * (1.0 + 0.01 * np.random.default_rng(77).standard_normal(xs.shape))
    w = noise_w(X)
    x_final = X[0, -1]
    tw = dr.fan(m, par, X, U, G, t, xs, x_final, w, SEED, 3, S, lim, variant == "hold", ff, 0.01, 4, 200)
    out = dict(K=K, B=B, S=S, h=h, G=G, ff=ff, lim=lim, xs=xs, w=w, x_final=x_final, twin=tw)
    _cases[key] = out
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_flights_against_the_twin(lqr_lib, name, hold, variant):
    """Six disturbed flights (w non-zero on all states but one, flight_offset 3) against the twin: x, u, t, steps, status, err0, err1 and
    max_dev to 1e-9, n_sat exact after the twin alone has shown that no commanded input comes within 1e-6 T_max of a limit.  The noise is
    what is compared: the undisturbed flight misses the bar by orders of magnitude."""
    k = flight_case(name, hold, variant)
    h, tw = k["h"], k["twin"]
    F = k["B"] * k["S"]
    if variant == "limits":
        assert all(e["min_margin"] > 1e-6 for e in tw), [e["min_margin"] for e in tw]
        assert any(e["n_sat"] > 0 for e in tw)
    c = new_context(lqr_lib, name, hold, k["K"], k["B"], h)
    c.set_trajectories(h["X"], h["U"], h["t"])
    c.set_gains(k["G"])
    if variant == "limits":
        c.set_input_limits(k["lim"])
    if variant == "hold":
        c.set_feedback_hold(1)
    if variant == "feedforward":
        c.set_feedforward_terms(k["ff"])
        c.set_feedforward(1)
    off = fly(c, k["xs"], k["x_final"], k["S"])
    c.set_disturbance(k["w"], SEED, 3)
    o = fly(c, k["xs"], k["x_final"], k["S"])
    c.close()
    assert o["n_finite"] == F
    worst = 0.0
    for f, e in enumerate(tw):
        gaps = {key: rel(o[key][f], e[key]) for key in ("x", "u", "t", "err0", "err1", "max_dev")}
        worst = max(worst, max(gaps.values()))
        assert o["steps"][f] == e["steps"] and o["status"][f] == e["status"] == 0, (f, o["steps"][f], e["steps"], o["status"][f])
        assert o["n_sat"][f] == e["n_sat"], (f, o["n_sat"][f], e["n_sat"])
        assert all(v <= 1e-9 for v in gaps.values()), (f, gaps)
        assert rel(o["max_clip"][f], e["max_clip"]) <= 1e-9
        assert rel(off["x"][f], e["x"]) > 1e-6  # 1e3 bars
    print(f"{name} {hold} {variant}: steps {[e['steps'] for e in tw]}, n_sat {[e['n_sat'] for e in tw]}, worst gap to the twin {worst:.2e} (bar 1e-9)")


# ---- 5. bitwise properties -------------------------------------------------------------------------------------------------------------------
_small = {}


def small(lqr_lib, name="rocketquat", hold="foh", B=3):
    """B heterogeneous trajectories of K = 5 with Riccati gains of the library under test, a disturbance and two starts per trajectory"""
    key = (lqr_lib, name, hold, B)
    if key not in _small:
        K = 5
        h = hetero(name, hold, K, B)
        c = new_context(lqr_lib, name, hold, K, B, h)
        c.set_trajectories(h["X"], h["U"], h["t"])
        assert c.compute_gains_riccati(2) == B * K
        G = c.download_gains()["gains"]
        c.close()
        _small[key] = dict(name=name, hold=hold, K=K, B=B, h=h, G=G, w=noise_w(h["X"]), x_final=h["X"][0, -1])
    return _small[key]


def context_of(lqr_lib, k, rows=None):
    """a context with the trajectories `rows` (an index array, repeats allowed; default all) of the case and their gains"""
    h = k["h"]
    rows = np.arange(k["B"]) if rows is None else np.asarray(rows)
    c = new_context(lqr_lib, k["name"], k["hold"], k["K"], len(rows), dict(h, par=h["par"][rows]))
    c.set_trajectories(h["X"][rows], h["U"][rows], h["t"][rows])
    c.set_gains(k["G"][rows])
    return c


def starts(k, S, seed=5):
    xs = np.repeat(k["h"]["X"][:, 0], S, axis=0)
    return xs * (1.0 + 0.01 * np.random.default_rng(seed).standard_normal(xs.shape))


def test_same_seed_same_bits_other_seed_other_bits(lqr_lib):
    k = small(lqr_lib)
    xs = starts(k, 2)
    c = context_of(lqr_lib, k)
    c.set_disturbance(k["w"], SEED, 0)
    a = fly(c, xs, k["x_final"], 2)
    b = fly(c, xs, k["x_final"], 2)
    c.set_disturbance(k["w"], SEED + 1, 0)
    other = fly(c, xs, k["x_final"], 2)
    c.close()
    assert (a["status"] == 0).all() and (a["steps"] > 20).all()
    for key in ALL_KEYS:
        assert same(a[key], b[key]), key
    assert (a["x"] != other["x"]).any(axis=1).all()


def test_fan_equals_replicated_trajectories(lqr_lib):
    """6 flights as 3 trajectories x samples = 2 and as 6 duplicated trajectories x samples = 1"""
    k = small(lqr_lib)
    xs = starts(k, 2)
    c = context_of(lqr_lib, k)
    c.set_disturbance(k["w"], SEED, 0)
    fan = fly(c, xs, k["x_final"], 2)
    c.close()
    c = context_of(lqr_lib, k, np.arange(6) // 2)
    c.set_disturbance(k["w"], SEED, 0)
    rep = fly(c, xs, k["x_final"], 1)
    c.close()
    for key in ALL_KEYS:
        assert same(fan[key], rep[key]), key


def test_fan_split_over_two_calls_with_flight_offset(lqr_lib):
    """65 flights (5 trajectories x 13, one past a wavefront) in one call, and the same flights as a call of 64 (flight_offset 0) and a call
    of 1 (flight_offset 64), each on replicated trajectories"""
    k = small(lqr_lib, B=5)
    S = 13
    xs = starts(k, S)
    c = context_of(lqr_lib, k)
    c.set_disturbance(k["w"], SEED, 0)
    fan = fly(c, xs, k["x_final"], S)
    c.close()
    rows = np.arange(65) // S
    c = context_of(lqr_lib, k, rows[:64])
    c.set_disturbance(k["w"], SEED, 0)
    first = fly(c, xs[:64], k["x_final"], 1)
    c.close()
    c = context_of(lqr_lib, k, rows[64:])
    c.set_disturbance(k["w"], SEED, 64)
    last = fly(c, xs[64:], k["x_final"], 1)
    c.set_disturbance(k["w"], SEED, 63)
    wrong = fly(c, xs[64:], k["x_final"], 1)
    c.close()
    for key in ALL_KEYS:
        assert same(fan[key], np.concatenate([first[key], last[key]])), key
    assert not same(wrong["x"], last["x"])


def test_record_and_step_cap_do_not_change_a_flight(lqr_lib):
    """A flight with max_steps = m is row m - 1 of the record of a longer one; n_record and write_steps change nothing"""
    k = small(lqr_lib)
    xs = starts(k, 2)
    F = xs.shape[0]
    c = context_of(lqr_lib, k)
    c.set_disturbance(k["w"], SEED, 0)
    plain = fly(c, xs, k["x_final"], 2)
    full = fly(c, xs, k["x_final"], 2, n_record=F, write_steps=1)
    some = fly(c, xs, k["x_final"], 2, n_record=2, write_steps=7)
    m = 17
    short = fly(c, xs, k["x_final"], 2, max_steps=m)
    c.close()
    for key in ALL_KEYS:
        assert same(plain[key], full[key]) and same(plain[key], some[key]), key
    assert (plain["steps"] > m).all() and (short["steps"] == m).all() and (short["status"] == 1).all()
    assert same(short["x"], full["record"]["X"][:, m - 1]) and same(short["u"], full["record"]["U"][:, m - 1])
    n = full["record"]["n"]
    assert (n == plain["steps"]).all()
    assert all(same(full["record"]["X"][f, n[f] - 1], plain["x"][f]) for f in range(F))
    assert same(some["record"]["X"][:, 1], full["record"]["X"][:2, 7])


@pytest.mark.parametrize("name,hold", [("rocketquat", "foh"), ("rocket2d", "zoh"), ("lander3dof", "foh")])
def test_off_is_bitwise_off_and_zero_intensity_changes_nothing(lqr_lib, name, hold):
    """set_disturbance(None) restores, bit for bit, the flights of a context that never had a disturbance; w = 0 equals noise off under =="""
    k = small(lqr_lib, name, hold)
    xs = starts(k, 2)
    c = context_of(lqr_lib, k)
    never = fly(c, xs, k["x_final"], 2)
    c.close()
    c = context_of(lqr_lib, k)
    c.set_disturbance(k["w"], SEED, 0)
    on = fly(c, xs, k["x_final"], 2)
    c.set_disturbance(None)
    back = fly(c, xs, k["x_final"], 2)
    c.set_disturbance(np.zeros_like(k["w"]), SEED, 0)
    zero = fly(c, xs, k["x_final"], 2)
    c.close()
    assert (on["x"] != never["x"]).any(axis=1).all()
    for key in ALL_KEYS:
        assert same(back[key], never[key]), key
        assert zero[key].shape == never[key].shape and (zero[key] == never[key]).all(), key


# ---- 6. ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_abi(lqr_lib):
    """A negative or non-finite w is refused and leaves the accepted setting in place; the argument checks of disturbance_normals; the
    setting invalidates neither gains nor a covariance sweep"""
    from scpp_amd import _lib

    L = _lib.load_lqr_library(lqr_lib)
    p = _lib._p
    k = small(lqr_lib)
    h = k["h"]
    xs = starts(k, 2)
    c = context_of(lqr_lib, k)
    c.set_covariance_inputs(h["S0"], h["w"])
    assert c.propagate_covariance(2, True) == k["B"]
    cov = c.download_covariance(True)
    c.set_disturbance(k["w"], SEED, 2)
    accepted = fly(c, xs, k["x_final"], 2)
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        for at in (0, c.nx - 1):
            w = np.array(k["w"])
            w[at] = bad
            assert L.scpp_hip_lqr_set_disturbance(c.h, p(w), SEED + 9, 0) == E_ARG, (bad, at)
    assert L.scpp_hip_lqr_set_disturbance(None, p(np.array(k["w"])), 0, 0) == E_ARG
    still = fly(c, xs, k["x_final"], 2)
    for key in ALL_KEYS:
        assert same(still[key], accepted[key]), key
    cov2, g2 = c.download_covariance(True), c.download_gains(False)
    for key in cov:
        assert same(cov2[key], cov[key]), key
    assert same(g2["gains"], k["G"])
    z = np.zeros((2, 3, c.nx))
    assert L.scpp_hip_lqr_disturbance_normals(c.h, SEED, 0, 2, 0, 3, p(z)) == 0 and (z != 0).all()
    assert L.scpp_hip_lqr_disturbance_normals(c.h, SEED, 0, 0, 0, 3, p(z)) == E_ARG
    assert L.scpp_hip_lqr_disturbance_normals(c.h, SEED, 0, -1, 0, 3, p(z)) == E_ARG
    assert L.scpp_hip_lqr_disturbance_normals(c.h, SEED, 0, 2, 0, 0, p(z)) == E_ARG
    assert L.scpp_hip_lqr_disturbance_normals(c.h, SEED, 0, 2, 0, 3, None) == E_ARG
    assert L.scpp_hip_lqr_disturbance_normals(None, SEED, 0, 2, 0, 3, p(z)) == E_ARG
    # asking for normals reads and changes no setting
    after = fly(c, xs, k["x_final"], 2)
    c.close()
    for key in ALL_KEYS:
        assert same(after[key], accepted[key]), key


# ---- 7. what it is for -----------------------------------------------------------------------------------------------------------------------
def predicted_covariance(model, par, X, U, G, t_max, w, time_step, steps):
    """S after `steps` plant steps of the linearised disturbed loop, from the oracle's Jacobians alone: per step, at the tracker's own (i, a),
    expm([[A, B, I], [0]] time_step) gives Phi, Gamma_B, Gamma_d; Acl = Phi - Gamma_B K_t; S <- Acl S Acl' + Gamma_d diag(w / time_step) Gamma_d'"""
    K, nU = X.shape[0], U.shape[0]
    nx, nu = X.shape[1], U.shape[1]
    S = np.zeros((nx, nx))
    Wd = np.diag(np.asarray(w) / time_step)
    t = 0.0
    for _ in range(steps):
        i, a = segment_and_fraction(K, t_max, t)
        j = i + 1 if nU == K else i
        _, A, Bm = oracle_lib.flow(model, X[i] + a * (X[i + 1] - X[i]), U[i] + a * (U[j] - U[i]), par)
        M = np.zeros((2 * nx + nu, 2 * nx + nu))
        M[:nx, :nx], M[:nx, nx:nx + nu], M[:nx, nx + nu:] = A, Bm, np.eye(nx)
        E = oracle_lib.expm(M * time_step)
        Phi, Gb, Gd = E[:nx, :nx], E[:nx, nx:nx + nu], E[:nx, nx + nu:]
        Acl = Phi - Gb @ (G[i] + a * (G[j] - G[i]))
        S = Acl @ S @ Acl.T + Gd @ Wd @ Gd.T
        t += time_step
    return S


def test_dispersion_of_a_fan_is_the_linear_prediction(lqr_lib):
    """Lander3dof, the dynamically exact golden nominal (first-order hold, trajectory 0, its G_ref): 2048 flights from X[0] under
    disturbance_std = 0.1 on the velocities, substeps = 2, 300 plant steps (every flight ends at the step cap), and one flight without noise.
    The (r, v) block of x_f - x_noise_off, whitened with the Cholesky factor of the same block of the predicted S, has
    sum |y|^2 / (6 N) = 1 +- 5 sqrt(2 / (6 N)) = 1 +- 0.0638 (a numpy prototype with an RK4 plant gave 0.988, 0.989, 1.003 over three
    seeds)."""
    from scpp_amd import _lib

    name, N, steps = "lander3dof", 2048, 300
    d = np.load(os.path.join(GOLDEN, f"lqr_{name}.npz"))
    X, U, t, G = d["foh_X"][:1], d["foh_U"][:1], d["foh_t"][:1], d["foh_G_ref"][:1]
    ts = float(d["time_step"])
    assert steps * ts < float(t[0])
    w = np.zeros(7)
    w[4:] = 0.1 ** 2
    c = _lib.LqrContext(MODELS[name], X.shape[1], 1, True, 0, lqr_lib)
    c.set_weights(d["q"], d["r"])
    c.set_flow_params(d["par"])
    c.set_trajectories(X, U, t)
    c.set_gains(G)
    off = fly(c, X[0, :1], X[0, -1], 1, 2, steps, time_step=ts)
    c.set_disturbance(w, 20261020, 0)
    on = fly(c, np.tile(X[0, 0], (N, 1)), X[0, -1], N, 2, steps, time_step=ts)
    c.close()
    assert (on["status"] == 1).all() and (on["steps"] == steps).all() and off["status"][0] == 1
    S = predicted_covariance(MODELS[name], d["par"], X[0], U[0], G[0], float(t[0]), w, ts, steps)
    blk = S[1:, 1:]
    e = on["x"][:, 1:] - off["x"][0, 1:]
    y = np.linalg.solve(np.linalg.cholesky(blk), e.T)
    stat = float((y * y).sum() / (6 * N))
    bar = 5.0 * math.sqrt(2.0 / (6 * N))
    ratios = e.var(axis=0) / np.diag(blk)
    print(f"{name}: {N} flights x {steps} steps, statistic {stat:.4f} (1 +- {bar:.4f}), condition number of the block {np.linalg.cond(blk):.1f}, "
          f"per-entry variance ratios r {ratios[:3].round(3).tolist()} v {ratios[3:].round(3).tolist()}")
    assert abs(stat - 1.0) <= bar

"""Linear MPC (csrc/mpc_kernel.h, csrc/mpc_setup.h) at EVERY supported horizon K = 3 .. 8, per input column, on populations whose optimum
is not the idle plan.  launchMpcSolve picks mpc_solve_kernel<14> for the shipped K = 7 and mpc_solve_kernel<16> for every other K: with
K in {3, 4, 5, 6, 8} the second instantiation runs with a padded tile (nv = 6 .. 14 of 16 variables), with half-filled MFMA row blocks
(nlp = 8 (K - 1) = 24, 40, 56 box rows) and with the full tile (nv = 16).  Every test runs the SAME assertions on the CPU emulation of the
kernel sources (`emu`) and, marked gpu, on the device library (`hip`).

Checker: the condensed twin of oracle/mpc.hpp through tests/mpc_compare.py, which measures its bars on the twin alone (100 x the twin's
rounding floor, per row and column); every precondition of a case (statuses, active set, sensitivity to the neighbour's x_final) is asserted
on the twin alone as well.  The twin itself is pinned against the literal, reference-shaped solver in tests/test_oracle_mpc.py."""
import numpy as np
import pytest

import scpp_amd

import mpc_compare as mc

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
B = 16
MAX_LEFT_OUT = 2
_cache = {}


@pytest.fixture(scope="module", params=BACKENDS)
def library(request):
    """the solver library of the emulation build or of the device build"""
    return request.getfixturevalue("emu_lib" if request.param == "emu" else "hip_lib")


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    """configuration roots per (K, braking), written once"""
    base = tmp_path_factory.mktemp("mpc_horizons")
    src = scpp_amd.Rocket2D().getParameterFolder()

    def root(K, braking=False):
        key = ("root", K, braking)
        if key not in _cache:
            _cache[key] = mc.write_config(base / f"k{K}{'b' if braking else ''}", src, K, braking)
        return _cache[key]

    return root


def _model(root):
    m = scpp_amd.Rocket2D(root).loadParameters()
    m.p.constrain_initial_final = False  # model.info: "enable for SC and disable for MPC/LQR"
    return m


def _algorithm(root, library, batch_max=B, **kw):
    return scpp_amd.MPCAlgorithm(_model(root), batch_max=batch_max, library=library).initialize(**kw)


def _solve(a, x0, xf):
    a.setInitialState(x0); a.setFinalState(np.broadcast_to(xf, x0.shape).copy())
    n = a.solve()
    out = a.getSolution()
    assert n == int((out["status"] >= 0).sum())
    return out


def _shared(key, make):
    """a reference is computed once per process and shared between the backends"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _braking_targets(x0):
    """x_final[b] = x_init[b], positions shifted, velocities, tilt and rate 0: a stop a few tens of metres away"""
    n = x0.shape[0]
    xf = np.zeros_like(x0)
    xf[:, 0] = x0[:, 0] + np.linspace(-30.0, 30.0, n)
    xf[:, 1] = x0[:, 1] + np.linspace(-20.0, 60.0, n)
    return xf


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", mc.HORIZONS)
def test_solve_at_every_horizon(oracle, library, roots, K):
    """shipped weights, the common x_final, 16 randomised start states"""
    root = roots(K)
    m = _model(root)
    x0 = m.randomized_initial_states(B)

    def make():
        ref = mc.twin_reference(oracle.MPC(root), x0, m.p.x_final, m.p)
        assert (ref["status"] == 0).all(), ref["status"]
        return ref

    ref = _shared(("solve", K), make)
    a = _algorithm(root, library)
    assert a.K == K
    out = _solve(a, x0, m.p.x_final)
    mc.check_against_twin(out, ref, a, f"solve K={K}", MAX_LEFT_OUT)
    mc.check_constraints(out, ref["solved"], m.p)
    a.ctx.close()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", mc.HORIZONS)
def test_braking_population_at_every_horizon(oracle, library, roots, K):
    """Cheap thrust and a per-row target: the upper thrust bound, interior thrust levels and a per-controller x_final at once.  With the
    shipped weights every plan of every other MPC test idles at T_min on every stage."""
    root = roots(K, braking=True)
    m = _model(root)
    p = m.p
    x0 = m.randomized_initial_states(B)
    xf = _braking_targets(x0)

    def make():
        o = oracle.MPC(root)
        ref = mc.twin_reference(o, x0, xf, p)
        assert (ref["status"] == 0).all(), ref["status"]
        T = ref["U"][:, :, 1]
        assert (T.max(axis=1) > 0.999 * p.T_max).all()                                               # a stage at the upper bound
        assert ((T > p.T_min + 1e-3 * p.T_max) & (T < 0.999 * p.T_max)).any(axis=1).all()          # a stage strictly between the bounds
        # the neighbour's x_final gives another thrust plan: right row and wrong row are >= 100 bars apart
        sep = np.array([np.abs(o.solve(x0[b], xf[(b + 1) % B], kind=1)["U"][:, 1] - T[b]).max() for b in range(B)]) / p.T_max
        assert (sep >= 1e-3).all() and (sep[ref["kept"]] >= 100.0 * ref["bar"][ref["kept"], 1]).all(), sep
        # independent of the twin's own arithmetic: the literal, reference-shaped solver finds no better plan
        for b in range(B):
            lit = o.solve(x0[b], xf[b], kind=0)
            assert lit["status"] in (0, 1)
            assert ref["cost"][b].sum() <= (lit["input_cost"] + lit["error_cost"]) * (1 + 1e-6), (b, ref["cost"][b].sum(), lit)
        return ref

    ref = _shared(("braking", K), make)
    a = _algorithm(root, library)
    out = _solve(a, x0, xf)
    mc.check_against_twin(out, ref, a, f"braking K={K}", MAX_LEFT_OUT)
    mc.check_constraints(out, ref["solved"], p)
    a.ctx.close()


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------
def _spread_targets(x_final, n):
    """per-row targets around the shipped one, tens of metres apart between neighbours and from row 0 (2.7 m of spacing moves error_cost
    by only 4.5e-5 relative on the least sensitive row)"""
    i = np.arange(n)
    xf = np.tile(x_final, (n, 1))
    xf[:, 0] += 90.0 * (-1.0) ** i * (1.0 + i / n)
    xf[:, 1] += 60.0 * ((i % 3) - 1.0) + 5.0 * i
    return xf


@pytest.mark.parametrize("K", (3, 7, 8))
def test_per_controller_final_state(oracle, library, roots, K):
    """Shipped weights, x_final of its own for every row.  The plan idles whatever the target, so U shows a wrong row only at 1e-8 of T_max;
    error_cost shows it: asserted at 1e-7 relative where the neighbour's (and row 0's) target moves it by >= 1e-3."""
    root = roots(K)
    m = _model(root)
    x0 = m.randomized_initial_states(B)
    xf = _spread_targets(m.p.x_final, B)

    def make():
        o = oracle.MPC(root)
        ref = mc.twin_reference(o, x0, xf, m.p)
        assert (ref["status"] == 0).all(), ref["status"]
        for b in range(B):
            for other in {(b + 1) % B, (b - 1) % B, 0} - {b}:
                q = o.solve(x0[b], xf[other], kind=1)
                assert q["status"] == 0 and abs(q["error_cost"] - ref["cost"][b, 1]) >= 1e-3 * ref["cost"][b, 1], (b, other)
        return ref

    ref = _shared(("final", K), make)
    a = _algorithm(root, library)
    out = _solve(a, x0, xf)
    assert (np.abs(out["cost"][:, 1] - ref["cost"][:, 1]) <= 1e-7 * ref["cost"][:, 1]).all()
    mc.check_against_twin(out, ref, a, f"x_final K={K}", MAX_LEFT_OUT)
    a.ctx.close()


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------
# iteration caps chosen on the twin (shipped weights, the first 8 randomised states): (every row ends with -1, every row ends with 1).  K = 3 ends
# with -1 under every cap up to 6 and with 1 under 8 and 9; K = 8 with -1 up to 9 and with 1 from 10 on.  6 rather than 5 and 11 rather than 10
# because there the final gap of every row is a factor 2 away from 5e-5 (under cap 10 at K = 8 it is 1.4e-5 .. 3.4e-5 on three rows, and
# the easy states of K = 3 stop at 3.2e-5 under cap 5)
CAPS = {3: (6, 8), 8: (9, 11)}


def _decided(term):
    """Rows whose exit cannot be changed by a last-digit difference between kernel and twin: with every threshold of the two exit rules
    (reduced accuracy: pres, dres < 1e-4 and gap or relgap < 5e-5; optimal: pres, dres < 1e-8 and gap or relgap < 1e-8) halved and with every
    threshold doubled, the final pres, dres, gap, relgap give the same two answers.  (A quantity within a factor 2 of a threshold that the
    rule does not depend on -- relgap next to 5e-5 when gap is 2e-6 -- does not take the row out.)"""
    pres, dres, gap, relgap = term.T

    def rules(f):
        return (((pres < 1e-4 * f) & (dres < 1e-4 * f) & ((gap < 5e-5 * f) | (relgap < 5e-5 * f))),
                ((pres < 1e-8 * f) & (dres < 1e-8 * f) & ((gap < 1e-8 * f) | (relgap < 1e-8 * f))))

    (i0, o0), (i1, o1) = rules(0.5), rules(2.0)
    return (i0 == i1) & (o0 == o1)


def _easy_states(K, m, x0):
    """start states that the shipped problem solves to reduced accuracy WITHIN the lower cap (found on the twin): they give a controller a
    plan before the capped solve of x0.  K = 3: at the target itself, a millimetre apart; K = 8: at rest at half of x0's position"""
    n = x0.shape[0]
    if K == 3:
        xe = np.tile(m.p.x_final, (n, 1))
        xe[:, 1] += 1e-3 * np.arange(n) / n
        return xe
    return np.hstack([0.5 * x0[:, :2], np.zeros((n, 4))])


@pytest.mark.parametrize("K", sorted(CAPS))
def test_iteration_limit_and_reduced_accuracy_exits(oracle, library, roots, K):
    """status -1 (iteration limit: nothing is written) and status 1 (reduced accuracy: the saved iterate) through initialize(maxit=...)"""
    root = roots(K)
    m = _model(root)
    n = 8
    x0 = m.randomized_initial_states(n)
    xe = _easy_states(K, m, x0)
    lo, hi = CAPS[K]

    def capped(cap, x, want):
        def make():
            o = oracle.MPC(root)
            o.set_tolerances(maxit=cap)
            ref = dict(mc.twin_reference(o, x, m.p.x_final, m.p))
            ref["decided"] = _decided(ref["term"])
            if want is not None:
                assert ref["decided"].sum() >= n - 1 and (ref["status"][ref["decided"]] == want).all(), (cap, ref["status"], ref["term"])
            return ref

        return make

    r_lo, r_hi = _shared(("caps", K, lo), capped(lo, x0, -1)), _shared(("caps", K, hi), capped(hi, x0, 1))
    r_easy = _shared(("caps easy", K), capped(lo, xe, None))
    easy = r_easy["decided"] & (r_easy["status"] >= 0)
    assert easy.sum() >= n // 2 and r_easy["U"][easy].any(axis=(1, 2)).all(), (r_easy["status"], r_easy["term"])
    # ---- the higher cap: status 1 everywhere, the plan is the saved iterate
    a = _algorithm(root, library, batch_max=n, maxit=hi)
    out = _solve(a, x0, m.p.x_final)
    mc.check_against_twin(out, r_hi, a, f"status 1 K={K}", 1, rows=r_hi["decided"])
    a.ctx.close()
    # ---- the lower cap: first the easy states (a plan for at least half of the controllers), then x0: -1, and the plan is still there
    a = _algorithm(root, library, batch_max=n, maxit=lo)
    prev = _solve(a, xe, m.p.x_final)
    mc.check_against_twin(prev, r_easy, a, f"status 1 before -1 K={K}", 1, rows=r_easy["decided"])
    out = _solve(a, x0, m.p.x_final)
    d = r_lo["decided"]
    assert (out["status"][d] == -1).all() and np.array_equal(out["iters"][d], r_lo["iters"][d])
    for k in ("U", "X", "cost"):
        assert np.array_equal(out[k][d], prev[k][d]), k
    a.ctx.close()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (3, 8))
def test_closed_loop_at_the_edge_horizons(request, oracle, library, roots, K):
    """MPC_sim.cpp:49-86 for 4 loops of 40 steps against the oracle's loop: the only path that drives mpc_solve_kernel<16> with an
    `active` mask and with states that come from the device's own plant step"""
    root = roots(K)
    m = _model(root)
    x0 = m.randomized_initial_states(4, first=11)

    def make():
        o = oracle.MPC(root)
        return [o.sim(x0[b], max_steps=40) for b in range(4)]

    q = _shared(("loop", K), make)
    a = _algorithm(root, library, batch_max=4)
    r = scpp_amd.MPCSim(a, max_steps=40).run(x0)
    print(f"closed loop K={K}: ipm_iters {r['ipm_iters'].tolist()} twin {[v['ipm_iters'] for v in q]} failed {r['failed_solves'].tolist()}")
    for b in range(4):
        assert r["steps"][b] == q[b]["steps"] == 40 and r["failed_solves"][b] == q[b]["failed_solves"] and r["reached"][b] == q[b]["reached"]
        assert np.abs(r["x"][b] - q[b]["x"]).max() < 1e-8 * np.abs(q[b]["x"]).max()  # the bar of test_gpu_mpc_closed_loop_parity
        if "emu" in request.node.callspec.id:
            assert r["ipm_iters"][b] == q[b]["ipm_iters"]
    a.ctx.close()


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------------
def test_resetup_on_one_context(library, roots):
    """scpp_hip_mpc_setup with K = 8, then 3, then 7 on ONE context, a solve after each: every row bitwise the row of a fresh context at that
    K (no stale constants, no stale padding rows or columns of the 16 x 16 tile, no stale plan behind the shorter horizon's stride)"""
    x0 = _model(roots(8)).randomized_initial_states(B)
    xf = _braking_targets(x0)
    one = None
    for K in (8, 3, 7):
        fresh = _algorithm(roots(K, braking=True), library)
        want = _solve(fresh, x0, xf)
        assert (want["status"] == 0).all()
        if one is None:
            one = _algorithm(roots(K, braking=True), library)
        else:
            one.ctx.mpc_setup(fresh.options(), fresh.model.flow_params())
        one.setInitialState(x0); one.setFinalState(xf)
        assert one.ctx.mpc_solve(x0, xf) == B
        got = one.ctx.mpc_download()
        for k in ("X", "U", "cost", "status", "iters"):
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (K, k)
        fresh.ctx.close()
    one.ctx.close()

"""The stage schedule of the segment integration (csrc/discretize_kernel.h: DISC_STAGE_SCHEDULE, csrc/common.h: RK_SKIP_DEAD) changes the ORDER
of the work -- three wavefront barriers per stage instead of five, the hoists from registers, two copies of the stage values, the per-call
set-up outside the segment loop, the dead RKF78 stage left out -- and never the arithmetic.  The claim is bitwise, so there is no tolerance
anywhere in this file: every comparison is np.array_equal against the old structure, which stays in the sources (schedule 0, 13 stages)."""
import os
import subprocess

import numpy as np
import pytest

import scpp_amd
from scpp_amd._lib import MODE_FOH, MODE_VT

# (name, model class, mode, zero-order hold): RocketQuat FOH with free and with fixed final time, RocketQuat ZOH, Rocket2D (6 states),
# Lander3dof (7 states: an odd number)
CASES = [
    ("rocketquat_foh_vt", "RocketQuat", MODE_FOH | MODE_VT, False),
    ("rocketquat_foh_fixed", "RocketQuat", MODE_FOH, False),
    ("rocketquat_zoh", "RocketQuat", MODE_VT, True),
    ("rocket2d", "Rocket2D", MODE_FOH | MODE_VT, False),
    ("lander3dof", "Lander3dof", MODE_FOH | MODE_VT, False),
]
STEPS = (1, 2, 5, 0)  # pinned step counts and the step-length rule


def _model(name):
    return getattr(scpp_amd, name)().loadParameters()


def _flow_params(m):
    if m.modelName == "Rocket2D":
        return m.flow_params()
    return m.flow_params(nondimensionalize=False)


def _trajectories(m, K, B, zoh, seed=7):
    """B made-up trajectories in SI units: the states from a randomised start to the model's final state, perturbed; thrust near hover, never
    zero; segment lengths from 0.02 s to 1.7 s, so that the step-length rule takes every count from 1 to 5 within one batch."""
    rng = np.random.default_rng(seed + 100 * K + B)
    x0 = m.randomized_initial_states(B)
    nu = {14: 4, 6: 2, 7: 3}[x0.shape[1]]
    xf = np.array(list(m.p.x_final), dtype=np.float64)
    w = np.linspace(0.0, 1.0, K)[None, :, None]
    X = x0[:, None, :] * (1.0 - w) + xf[None, None, :] * w
    X = X * (1.0 + 1e-2 * rng.standard_normal(X.shape)) + 1e-3 * rng.standard_normal(X.shape)
    nk = K - 1 if zoh else K
    U = np.zeros((B, nk, nu))
    if m.modelName == "Rocket2D":
        U[..., 0] = 0.05 * rng.standard_normal((B, nk))
        U[..., 1] = -m.p.g_I[1] * m.p.m * (1.0 + 0.2 * rng.uniform(-1, 1, (B, nk)))
    else:
        g = abs(float(m.p.g_I[2]))
        mass = X[:, :nk, 0]
        U[..., 0] = 0.05 * g * mass * rng.standard_normal((B, nk))
        U[..., 1] = 0.05 * g * mass * rng.standard_normal((B, nk))
        U[..., 2] = g * mass * (1.0 + 0.2 * rng.uniform(-1, 1, (B, nk)))
    seg = np.geomspace(0.02, 1.7, B)
    rng.shuffle(seg)
    sigma = seg * (K - 1)
    return X, U, sigma


def _discretize_all(lib, models, Ks, B, cases=CASES, steps=STEPS, env=None):
    """{(case, K, steps): (A, B, C, S, Z)}; `env`: environment the contexts are created under"""
    out = {}
    for name, mname, mode, zoh in cases:
        m = models[mname]
        for K in Ks:
            X, U, sigma = _trajectories(m, K, B, zoh)
            old = {k: os.environ.get(k) for k in (env or {})}
            os.environ.update(env or {})
            try:
                ctx = scpp_amd.Context(m.model_id, K=K, batch_max=B, library=lib)
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            ctx.set_flow_params(np.tile(_flow_params(m), (B, 1)))
            ctx.upload_traj(X, U, sigma)
            for st in steps:
                ctx.set_discretization_steps(st)
                ctx.discretize(mode)
                out[(name, K, st)] = ctx.download_dd()
            ctx.close()
    return out


def _assert_same(a, b):
    """every array the case's mode produces: C exists under first-order hold only, S with a free final time only (the kernel leaves the
    other buffer alone)"""
    modes = {name: mode for name, _, mode, _ in CASES}
    assert a.keys() == b.keys()
    for key in a:
        for nm, p, q in zip("ABCSZ", a[key], b[key]):
            if (nm == "C" and not modes[key[0]] & MODE_FOH) or (nm == "S" and not modes[key[0]] & MODE_VT):
                continue
            assert np.isfinite(p).all(), (key, nm)
            assert np.array_equal(p, q), (key, nm, float(np.abs(p - q).max()))
        assert np.abs(a[key][0]).max() > 0.5  # something was integrated: A = Phi(dt) is near the identity


@pytest.fixture(scope="module")
def models():
    return {n: _model(n) for n in ("RocketQuat", "Rocket2D", "Lander3dof")}


@pytest.fixture(scope="module")
def emu_ref_lib(tmp_path_factory):
    """The kernel sources on the emulator once more, with the three switches off: the old stage schedule in every kernel, 13 stages everywhere."""
    import __graft_entry__ as g

    ref = str(tmp_path_factory.mktemp("disc_schedule") / "libscpp_emu_ref.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-DSCPP_HIP_EMU", "-DDISC_STAGE_SCHEDULE=0", "-DDISC_OVERLAP=0", "-DRK_SKIP_DEAD=0",
                           "-I" + os.path.join(g.ROOT, "tests", "emu"), "-shared", "-o", ref, "-x", "c++", os.path.join(g.CSRC, "scpp_hip.cpp")],
                          stderr=subprocess.DEVNULL)
    return ref


def test_emu_discretize_is_bitwise_the_old_schedule(emu_lib, emu_ref_lib, models):
    """scpp_hip_discretize + scpp_hip_download_dd, shipped build against the build with the switches off: K = 3 and 5, B = 9 (one more than the
    8-way XCD block map), 1, 2, 5 steps and the step-length rule."""
    new = _discretize_all(emu_lib, models, (3, 5), 9)
    ref = _discretize_all(emu_ref_lib, models, (3, 5), 9)
    _assert_same(new, ref)


def test_emu_schedule_hook_is_the_old_schedule(emu_lib, emu_ref_lib, models):
    """A context created under SCPP_DISC_SCHEDULE=0 launches the old schedule with 13 stages from the SHIPPED library: what the GPU test below
    compares against is the structure of the reference build."""
    hook = _discretize_all(emu_lib, models, (3,), 9, steps=(5, 0), env={"SCPP_DISC_SCHEDULE": "0"})
    ref = _discretize_all(emu_ref_lib, models, (3,), 9, steps=(5, 0))
    _assert_same(hook, ref)


@pytest.mark.parametrize("mname", ["RocketQuat", "Rocket2D", "Lander3dof"])
def test_emu_persistent_stream_is_bitwise_the_old_schedule(emu_lib, emu_ref_lib, models, mname):
    """One SCvx streaming job through the persistent kernel: K = 4, five instances through two slots, at most four iterations -- slots are
    refilled, the integration's LDS region is reused after every solve, and the copy of Ys a stage writes must come out right across segments
    and calls.  Every result row, J (`nonlinear_cost`: the cost step leaves the dead stage out too) included."""
    m = models[mname]
    xs = m.randomized_initial_states(5, first=10)  # (at K = 4 one of Rocket2D's first five runs into the cap of 256 solves: 20 s on the emulator)
    rows = []
    for lib in (emu_lib, emu_ref_lib):
        alg = scpp_amd.SCvxAlgorithm(m, K=4, batch_max=2, library=lib, max_iterations=4).initialize()
        alg.ctx.set_stream_engine(scpp_amd._lib.STREAM_PERSISTENT)
        alg.solveStream(xs, slots=2)
        rows.append(alg.ctx.stream_download_rows())
        so = alg.getStreamSolution()
        assert (so["instance"] == np.arange(5)).all() and (so["status"] == 0).all() and (so["solves"] >= so["sc_iters"]).all() and (so["sc_iters"] >= 1).all()
        assert np.isfinite(so["nonlinear_cost"]).all()
        alg.ctx.close()
    assert np.array_equal(rows[0], rows[1])


def test_emu_simulate_is_bitwise_the_old_schedule(emu_lib, emu_ref_lib, models):
    for mname in ("RocketQuat", "Rocket2D", "Lander3dof"):
        m = models[mname]
        B = 5
        X, U, sigma = _trajectories(m, 3, B, False)
        out = []
        for lib in (emu_lib, emu_ref_lib):
            ctx = scpp_amd.Context(m.model_id, K=3, batch_max=B, library=lib)
            ctx.set_flow_params(np.tile(_flow_params(m), (B, 1)))
            out.append(ctx.simulate(sigma / 2.0, U[:, 0], U[:, 1], X[:, 0]))
            ctx.close()
        assert np.isfinite(out[0]).all() and np.abs(out[0] - X[:, 0]).max() > 0
        assert np.array_equal(out[0], out[1]), mname


@pytest.mark.gpu
def test_gpu_discretize_is_bitwise_the_old_schedule(hip_lib, models):
    """On the device: two contexts of one process, one of them created under SCPP_DISC_SCHEDULE=0 (old schedule, 13 stages).  A, B, C, S, Z
    bitwise equal on the emulator's cases and on one K = 50, B = 16 RocketQuat FOH case.  The persistent-engine == pool-engine tests tie the
    persistent kernel to discretize_kernel; this ties discretize_kernel to the old schedule."""
    new = _discretize_all(hip_lib, models, (3, 5), 9)
    old = _discretize_all(hip_lib, models, (3, 5), 9, env={"SCPP_DISC_SCHEDULE": "0"})
    _assert_same(new, old)
    big = CASES[:1]
    new = _discretize_all(hip_lib, models, (50,), 16, cases=big, steps=(5, 0))
    old = _discretize_all(hip_lib, models, (50,), 16, cases=big, steps=(5, 0), env={"SCPP_DISC_SCHEDULE": "0"})
    _assert_same(new, old)

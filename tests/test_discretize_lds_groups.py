"""The LDS read groups of the segment integration (csrc/discretize_kernel.h: DISC_LDS_GROUPS) change the ORDER of LDS operations inside a
stage's barrier intervals -- every factor of a table pass requested before the first product, the operands of the product requested together
before the first MFMA, a stage's share of the input table requested one stage ahead, the columns of the z identity and the segment's global
loads as groups -- and never an expression.  The claim is bitwise, so there is no tolerance anywhere in this file.  On the emulator the shipped
build is compared with a -DDISC_LDS_GROUPS=0 build (the statement order of before); on the device with the same library's contexts created
under SCPP_DISC_SCHEDULE=0, which launch the old stage schedule with all 13 stages: code the switch does not reach.  A read moved across one of
the stage's three barriers (the previous stage's W_J / W_F / W_X, the other copy of the stage values) shows in both."""
import os
import subprocess

import numpy as np
import pytest

import scpp_amd
from test_discretize_schedule import CASES, _assert_same, _discretize_all
from test_setup_schedule import bits, environment

OLD_SCHEDULE = {"SCPP_DISC_SCHEDULE": "0"}
ROCKETQUAT = [c for c in CASES if c[1] == "RocketQuat"]  # first-order hold with free and with fixed final time, zero-order hold
BATCH_KEYS = ("X", "U", "sigma", "nu_norm", "nonlinear_cost", "trust_region", "sc_iters", "solves", "converged", "status", "ipm_iters")


@pytest.fixture(scope="module")
def models():
    return {n: getattr(scpp_amd, n)().loadParameters() for n in ("RocketQuat", "Rocket2D", "Lander3dof")}


@pytest.fixture(scope="module")
def emu_ungrouped_lib(tmp_path_factory):
    """The kernel sources on the emulator once more, with the one switch off."""
    import __graft_entry__ as g

    ref = str(tmp_path_factory.mktemp("disc_lds_groups") / "libscpp_emu_ungrouped.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-DSCPP_HIP_EMU", "-DDISC_LDS_GROUPS=0", "-I" + os.path.join(g.ROOT, "tests", "emu"),
                           "-shared", "-o", ref, "-x", "c++", os.path.join(g.CSRC, "scpp_hip.cpp")], stderr=subprocess.DEVNULL)
    return ref


def _stream(lib, model, K, x0, slots, foh, steps=None, max_iterations=4):
    """one streaming job through the persistent kernel: (result rows, solution)"""
    alg = scpp_amd.SCvxAlgorithm(model, K=K, batch_max=slots, library=lib, max_iterations=max_iterations).initialize()
    alg.ctx.set_stream_engine(scpp_amd._lib.STREAM_PERSISTENT)
    if steps is not None:
        alg.ctx.set_discretization_steps(steps)
    alg.opts.interpolate_input = int(foh)
    alg.ctx.scvx_solve_stream(model.sc_params(), alg.opts, x0, slots=slots)
    rows = alg.ctx.stream_download_rows()
    so = alg.getStreamSolution()
    alg.ctx.close()
    return rows, so


def _batch(lib, model, K, x0, foh, env, steps=None, max_iterations=4):
    """the batch entry point (scpp_hip_scvx_solve) on the same instances, run as rounds of kernel launches by a context created under `env`"""
    alg = scpp_amd.SCvxAlgorithm(model, K=K, batch_max=len(x0), library=lib, max_iterations=max_iterations)
    with environment(env):
        alg.initialize()
    # the rounds of launches, not the persistent kernel (the batch entry's default at these sizes too): discretize_kernel does the integration
    alg.ctx.set_stream_engine(scpp_amd._lib.STREAM_POOLS)
    if steps is not None:
        alg.ctx.set_discretization_steps(steps)
    alg.opts.interpolate_input = int(foh)
    alg.ctx.scvx_setup(model.sc_params(), alg.opts, x0)
    alg.ctx.scvx_solve()
    out = alg.getSolution()
    alg.ctx.close()
    return out


def _assert_stream_is_batch(so, ref, what):
    assert (so["instance"] == np.arange(len(ref["X"]))).all() and (so["status"] == 0).all(), what
    assert (ref["sc_iters"] >= 1).all() and np.isfinite(ref["X"]).all(), what
    for key in BATCH_KEYS:
        assert np.array_equal(bits(so[key]), bits(ref[key])), (what, key)


def test_emu_discretize_is_bitwise_the_ungrouped_order(emu_lib, emu_ungrouped_lib, models):
    """A, B, C, S, Z of scpp_hip_discretize for the three models and both input holds: K = 3 (two segments: the smallest case with a segment
    boundary, where the LDS region is reused and the first stage's share of the input table is requested anew) and K = 5, 9 instances, 1, 2 and
    5 pinned steps and the step-length rule (segments of 0.02 s to 1.7 s: every count from 1 to 5 within the batch)."""
    new = _discretize_all(emu_lib, models, (3, 5), 9)
    ref = _discretize_all(emu_ungrouped_lib, models, (3, 5), 9)
    _assert_same(new, ref)


@pytest.mark.parametrize("mname,foh", [("RocketQuat", True), ("RocketQuat", False), ("Rocket2D", True), ("Lander3dof", True)],
                         ids=["rocketquat_foh", "rocketquat_zoh", "rocket2d", "lander3dof"])
def test_emu_persistent_stream_is_bitwise_the_ungrouped_order(emu_lib, emu_ungrouped_lib, models, mname, foh):
    """One SCvx streaming job through the persistent kernel: K = 4, five instances through two slots, at most four iterations -- a wavefront
    walks through the three segments of its instance, the solver overwrites the integration's LDS region between two calls, slots are refilled."""
    m = models[mname]
    xs = m.randomized_initial_states(5, first=10)
    new, so = _stream(emu_lib, m, 4, xs, 2, foh)
    ref, _ = _stream(emu_ungrouped_lib, m, 4, xs, 2, foh)
    assert (so["instance"] == np.arange(5)).all() and (so["status"] == 0).all() and (so["sc_iters"] >= 1).all() and np.isfinite(so["nonlinear_cost"]).all()
    assert np.array_equal(bits(new), bits(ref))


@pytest.mark.gpu
def test_gpu_discretize_is_bitwise_the_old_schedule(hip_lib, models):
    """discretize_kernel for RocketQuat, first-order hold (free and fixed final time) and zero-order hold, K = 3 and 5, 9 instances (more than 8
    crosses the block-to-XCD map), 1 and 5 steps: one step has no step before it, five exercise the hand-over from stage 12 to stage 0 (with 12
    live stages the copy of the stage values a stage writes is fixed by the stage index)."""
    new = _discretize_all(hip_lib, models, (3, 5), 9, cases=ROCKETQUAT, steps=(1, 5))
    old = _discretize_all(hip_lib, models, (3, 5), 9, cases=ROCKETQUAT, steps=(1, 5), env=OLD_SCHEDULE)
    _assert_same(new, old)


@pytest.mark.gpu
@pytest.mark.parametrize("foh", [True, False], ids=["foh", "zoh"])
def test_gpu_persistent_engine_is_bitwise_the_old_schedule(hip_lib, models, foh):
    """The persistent kernel's integration step (the grouped order, 12 stages) against the batch entry point of a context created under
    SCPP_DISC_SCHEDULE=0, whose discretize_kernel launches are the old schedule: K = 3 and 5, 9 instances in 9 slots, 1 and 5 steps."""
    m = models["RocketQuat"]
    x0 = m.randomized_initial_states(9, first=10)
    for K in (3, 5):
        for steps in (1, 5):
            _, so = _stream(hip_lib, m, K, x0, 9, foh, steps=steps)
            ref = _batch(hip_lib, m, K, x0, foh, OLD_SCHEDULE, steps=steps)
            _assert_stream_is_batch(so, ref, (K, steps, foh))


@pytest.mark.gpu
def test_gpu_streaming_job_is_bitwise_the_old_schedule(hip_lib, models):
    """40 RocketQuat instances through 16 slots of the persistent kernel at K = 50, to convergence: every slot is refilled, and every row is
    bitwise what scpp_hip_scvx_solve computes for that instance with the old schedule."""
    m = models["RocketQuat"]
    x0 = m.randomized_initial_states(40, first=200)
    _, so = _stream(hip_lib, m, 50, x0, 16, True, max_iterations=None)
    ref = _batch(hip_lib, m, 50, x0, True, OLD_SCHEDULE, max_iterations=None)
    assert int(so["converged"].sum()) >= 36  # the shipped scenario converges
    _assert_stream_is_batch(so, ref, "K = 50")

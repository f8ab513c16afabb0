"""The once-per-solve phases of the interior-point solver (csrc/ipm_solve.h: IPM_SETUP_SCHEDULE -- set-up, warm start, data norms, the solve's
own copies) issue their memory operations in groups instead of element by element.  Only the ORDER of loads and stores differs, so the claim
is bitwise and there is no tolerance anywhere in this file: a context created under SCPP_SETUP_SCHEDULE=0 runs the element-wise functions,
which stay in the sources, and every comparison is np.array_equal on the uint64 views of what the two contexts of one process return."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import scpp_amd

MODELS = ("RocketQuat", "Rocket2D", "Lander3dof")  # NX * NX = 196, 36, 49 ; NX * NU = 56, 12, 21: chunk remainders, an odd state count
OLD = {"SCPP_SETUP_SCHEDULE": "0"}
# RocketQuat instances 8 and 9 at K = 5: instance 8 takes 8 sub-problem solves for 6 iterations (picked on the emulator; the test asserts it)
REJECT_FIRST, REJECT_COUNT, REJECT_ITERATIONS = 8, 2, 10


@contextlib.contextmanager
def environment(env):
    """the variables a context is created under (scpp_hip_create reads the hook once, per context)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_bitwise(new, old, what):
    assert new.keys() == old.keys()
    for key in new:
        assert np.array_equal(bits(new[key]), bits(old[key])), (what, key)


def scvx_batch(lib, model, K, foh, x0, env, max_iterations=4):
    """the SCvx batch entry: X, U, sigma, every per-instance scalar, the iteration / solve / status counts"""
    alg = scpp_amd.SCvxAlgorithm(model, K=K, batch_max=len(x0), library=lib, max_iterations=max_iterations)
    with environment(env):
        alg.initialize()
    alg.opts.interpolate_input = int(foh)
    alg.ctx.scvx_setup(model.sc_params(), alg.opts, x0)
    alg.ctx.scvx_solve()
    out = alg.getSolution()
    alg.ctx.close()
    return out


def sc_batch(lib, model, K, foh, x0, env):
    """the SC mode with a free final time: the S column of the dynamics and the sigma border are live"""
    alg = scpp_amd.SCAlgorithm(model, K=K, batch_max=len(x0), library=lib)
    with environment(env):
        alg.initialize()
    alg.opts.interpolate_input = int(foh)
    assert alg.opts.free_final_time == 1
    alg.ctx.sc_setup(model.sc_params(), alg.opts, x0)
    alg.ctx.sc_solve()
    out = alg.getSolution()
    alg.ctx.close()
    return out


def stream_rows(lib, model, K, x0, slots, env, max_iterations=3):
    alg = scpp_amd.SCvxAlgorithm(model, K=K, batch_max=slots, library=lib, max_iterations=max_iterations)
    with environment(env):
        alg.initialize()
    alg.ctx.set_stream_engine(scpp_amd._lib.STREAM_PERSISTENT)
    alg.solveStream(x0, slots=slots)
    rows = alg.ctx.stream_download_rows()
    so = alg.getStreamSolution()
    alg.ctx.close()
    return rows, so


@pytest.fixture(scope="module")
def models():
    return {n: getattr(scpp_amd, n)().loadParameters() for n in MODELS}


@pytest.mark.parametrize("foh", [True, False], ids=["foh", "zoh"])
@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("mname", MODELS)
def test_emu_scvx_batch_is_bitwise_the_elementwise_setup(emu_lib, models, mname, K, foh):
    """K = 3: two segments, fewer than any chunk.  Two instances: cold set-ups, warm re-solves and (where a candidate is rejected) re-solves on
    unchanged data."""
    m = models[mname]
    x0 = m.randomized_initial_states(2)
    new = scvx_batch(emu_lib, m, K, foh, x0, {})
    old = scvx_batch(emu_lib, m, K, foh, x0, OLD)
    assert (old["status"] == 0).all() and (old["sc_iters"] >= 1).all() and np.isfinite(old["X"]).all()
    assert_bitwise(new, old, (mname, K, foh))


@pytest.mark.parametrize("foh", [True, False], ids=["foh", "zoh"])
@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("mname", MODELS)
def test_emu_sc_free_final_time_is_bitwise_the_elementwise_setup(emu_lib, models, mname, K, foh):
    m = models[mname]
    x0 = m.randomized_initial_states(2)
    new = sc_batch(emu_lib, m, K, foh, x0, {})
    old = sc_batch(emu_lib, m, K, foh, x0, OLD)
    assert (old["sc_iters"] >= 2).all() and np.isfinite(old["X"]).all()  # at least one warm-started solve
    assert_bitwise(new, old, (mname, K, foh))


def test_emu_rejected_candidate_is_bitwise_the_elementwise_setup(emu_lib, models):
    """A run with rejected candidates: the re-solve keeps the field-major copy of the dynamics and takes the data norm from the warm-start
    block (dd_same, gsave[13])."""
    m = models["RocketQuat"]
    x0 = m.randomized_initial_states(REJECT_COUNT, first=REJECT_FIRST)
    old = scvx_batch(emu_lib, m, 5, True, x0, OLD, max_iterations=REJECT_ITERATIONS)
    assert (old["solves"] > old["sc_iters"]).any(), (old["solves"], old["sc_iters"])  # the precondition: a candidate was rejected
    new = scvx_batch(emu_lib, m, 5, True, x0, {}, max_iterations=REJECT_ITERATIONS)
    assert_bitwise(new, old, "rejected candidate")


@pytest.mark.parametrize("mname", MODELS)
def test_emu_persistent_stream_is_bitwise_the_elementwise_setup(emu_lib, models, mname):
    """Nine instances through four slots of the persistent kernel: a cold set-up on a workspace that holds another instance's leftovers."""
    m = models[mname]
    x0 = m.randomized_initial_states(9, first=10)
    new, so = stream_rows(emu_lib, m, 4, x0, 4, {})
    old, _ = stream_rows(emu_lib, m, 4, x0, 4, OLD)
    assert (so["instance"] == np.arange(9)).all() and (so["status"] == 0).all() and (so["sc_iters"] >= 1).all()
    assert np.array_equal(bits(new), bits(old))


_INJECT = """
import json, os, sys, numpy as np, scpp_amd
m = scpp_amd.RocketQuat().loadParameters()
alg = scpp_amd.SCAlgorithm(m, K=5, batch_max=1, library=sys.argv[1]).initialize()
alg.ctx.sc_setup(m.sc_params(), alg.opts, m.randomized_initial_states(1))
alg.ctx.sc_iterate()
first = int(alg.ctx.download()['ipm_iters'][0])
alg.ctx.sc_iterate()
o = alg.ctx.download()
print('RESULT ' + json.dumps(dict(first=first, ipm_iters=int(o['ipm_iters'][0]), status=int(o['status'][0]), sigma=o['sigma'].view(np.uint64).tolist(),
                                  X=o['X'].view(np.uint64).ravel().tolist(), U=o['U'].view(np.uint64).ravel().tolist(),
                                  nu_norm=o['nu_norm'].view(np.uint64).tolist(), sum_delta=o['sum_delta'].view(np.uint64).tolist())))
"""


def _two_solves(emu_lib, inject, env):
    """a cold and a warm-started sub-problem solve in a fresh process (the injection hook counts the residual evaluations of its process)"""
    import json

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ, PYTHONPATH=root, **env)
    e.pop("SCPP_EMU_INJECT_RES", None)
    if inject:
        e["SCPP_EMU_INJECT_RES"] = inject
    out = subprocess.run([sys.executable, "-c", _INJECT, emu_lib], env=e, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])


def test_emu_warm_attempt_repeated_cold_is_bitwise_the_elementwise_setup(emu_lib):
    """The fault-injection hook of the emulator build (SCPP_EMU_INJECT_RES) hands the warm-started second solve a negative gap at its second
    residual evaluation, where no fall-back iterate exists yet: the attempt is given up after one iteration and repeated from the cold
    initialisation, on a workspace the warm attempt has written.  Once under each path."""
    plain = _two_solves(emu_lib, "", {})
    assert plain["status"] == 0 and plain["first"] > 4
    spec = "%d:0:0:-1e-3" % (plain["first"] + 2)  # the cold solve evaluates first + 1 times; + 1: the warm solve's second evaluation
    new = _two_solves(emu_lib, spec, {})
    old = _two_solves(emu_lib, spec, OLD)
    assert old["status"] == 0 and old["first"] == plain["first"]
    # the injection took effect: one warm iteration, then a whole cold solve (a fall-back iterate returned instead would end the solve after that one iteration)
    assert old["ipm_iters"] != plain["ipm_iters"] and old["ipm_iters"] - old["first"] - 1 > 4
    assert new == old

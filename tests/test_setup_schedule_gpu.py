"""On the device: the grouped once-per-solve phases (csrc/ipm_solve.h: IPM_SETUP_SCHEDULE) against the element-wise ones, two contexts of one
process, one of them created under SCPP_SETUP_SCHEDULE=0.  Bitwise: np.array_equal on uint64 views, no tolerance (tests/test_setup_schedule.py
makes the same comparison on the emulator at the shapes where the chunking can go wrong)."""
import numpy as np
import pytest

import scpp_amd
from test_setup_schedule import OLD, assert_bitwise, bits, scvx_batch, stream_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models():
    return {n: getattr(scpp_amd, n)().loadParameters() for n in ("RocketQuat", "Rocket2D", "Lander3dof")}


@pytest.mark.parametrize("mname,K", [("RocketQuat", 5), ("RocketQuat", 50), ("Rocket2D", 30), ("Lander3dof", 30)])
def test_gpu_scvx_batch_is_bitwise_the_elementwise_setup(hip_lib, models, mname, K):
    """64 instances through the SCvx batch entry with the configured iteration limit: cold set-ups, warm re-solves, re-solves after rejected
    candidates on unchanged data."""
    m = models[mname]
    x0 = m.randomized_initial_states(64)
    new = scvx_batch(hip_lib, m, K, True, x0, {}, max_iterations=None)
    old = scvx_batch(hip_lib, m, K, True, x0, OLD, max_iterations=None)
    assert np.isfinite(old["X"]).all() and (old["sc_iters"] >= 1).all() and (old["solves"] >= old["sc_iters"]).all()
    assert_bitwise(new, old, (mname, K))


def test_gpu_persistent_stream_is_bitwise_the_elementwise_setup(hip_lib, models):
    """96 RocketQuat instances through 64 slots of the persistent kernel at K = 50: refilled slots set up cold on another instance's workspace."""
    m = models["RocketQuat"]
    x0 = m.randomized_initial_states(96)
    new, so = stream_rows(hip_lib, m, 50, x0, 64, {}, max_iterations=None)
    old, _ = stream_rows(hip_lib, m, 50, x0, 64, OLD, max_iterations=None)
    assert (so["instance"] == np.arange(96)).all() and (so["sc_iters"] >= 1).all() and np.isfinite(so["X"]).all()
    assert np.array_equal(bits(new), bits(old))

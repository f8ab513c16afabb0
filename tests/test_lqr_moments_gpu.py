"""The moments sweep at size on the device: 256 RocketQuat trajectories from solveStream, the affine law's gains, the covariance sweep and the
moments sweep timed in the same run (5 RKF78 steps per segment), with the feedforward term and without it, and 256 flights each
(tools/lqr_rate.py, moments=5).  No pass / fail on time: every trajectory is accounted for by its status, nothing non-finite leaves the
device, and the covariance block is the covariance sweep's.  The figures are printed (one JSON object); DESIGN.md section 5.2 records those of
the 8192-trajectory run."""
import json
import os
import sys

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_lqr_moments_at_size(hip_lib):
    import __graft_entry__ as g

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lqr_rate

    n = 256
    lqr = os.environ.get("SCPP_LQR_LIBRARY") or (g.LQR_LIB if os.path.exists(g.LQR_LIB) else g.build_lqr())
    r = lqr_rate.measure(n, repeat=2, library=hip_lib, lqr_library=lqr, moments=5)
    print(json.dumps(r, indent=1))
    assert r["moments_trajectories"] == n and r["moments_rhs"] == n * 49 * 5 * 13
    assert r["moments_wall_s"] > 0 and r["moments_covariance_wall_s"] > 0
    assert len(r["moments_nominal_last_node_to_target_p5_p50_p95"]) == 3
    for key in ("moments_ff", "moments_noff"):
        assert r[f"{key}_status_ok"] + r[f"{key}_status_gains_incomplete"] + r[f"{key}_status_nonfinite"] == n and r[f"{key}_status_other"] == 0
        assert r[f"{key}_status_ok"] > 0 and r[f"{key}_status_ok"] <= r["moments_covariance_status_ok"]  # m can fail a trajectory that S alone passes
        assert r[f"{key}_nonfinite_values"] == 0
        assert r[f"{key}_covariance_block_equal"] or r[f"{key}_status_ok"] < r["moments_covariance_status_ok"]
        assert len(r[f"{key}_mean_final_norm_p5_p50_p95"]) == 3 and len(r[f"{key}_flown_to_last_node_p5_p50_p95"]) == 3
    # the default leg is what it is without this one
    assert r["gain_nodes"] == n * 50 and r["flights_finite"] + r["flights_nonfinite"] == n

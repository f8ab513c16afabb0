"""Closed-loop covariance sweep at size on the device: 8192 RocketQuat trajectories from solveStream, one forward sweep each under the
finite-horizon gains (5 RKF78 steps per segment: 3185 right-hand sides per trajectory), next to the frozen-time and Riccati legs of the same
run (tools/lqr_rate.py, riccati=5, covariance=5).  No pass / fail on time: every trajectory is accounted for by its status, nothing
non-finite leaves the device.  The figures are printed (one JSON object); DESIGN.md section 5.2 records them."""
import json
import os
import sys

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_lqr_covariance_at_size(hip_lib):
    import __graft_entry__ as g

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lqr_rate

    lqr = os.environ.get("SCPP_LQR_LIBRARY") or (g.LQR_LIB if os.path.exists(g.LQR_LIB) else g.build_lqr())
    r = lqr_rate.measure(8192, repeat=2, library=hip_lib, lqr_library=lqr, riccati=5, covariance=5)
    print(json.dumps(r, indent=1))
    assert r["covariance_trajectories"] == 8192 and r["covariance_nodes"] == 8192 * 50 and r["covariance_rhs"] == 8192 * 49 * 5 * 13
    assert r["covariance_status_ok"] + r["covariance_status_gains_incomplete"] + r["covariance_status_nonfinite"] == 8192
    assert r["covariance_status_other"] == 0
    assert r["covariance_nonfinite_values"] == 0
    assert r["covariance_wall_s"] > 0 and len(r["covariance_final_position_std_p5_p50_p95"]) == 3
    assert r["covariance_thrust_3sigma_max"] >= 0
    # the frozen-time and Riccati legs of the same run: their keys and their meaning are unchanged
    assert r["gain_nodes"] == 8192 * 50 and r["gains_nonfinite_values"] == 0 and r["output_nonfinite_values"] == 0
    assert r["riccati_nodes"] == 8192 * 50 and r["riccati_rhs"] == 8192 * 49 * 5 * 13
    assert r["riccati_status_ok"] + r["riccati_status_nonfinite"] == r["riccati_nodes"] and r["riccati_status_other"] == 0
    assert r["riccati_gains_nonfinite_values"] == 0 and r["riccati_output_nonfinite_values"] == 0

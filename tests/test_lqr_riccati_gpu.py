"""Finite-horizon LQR gains at size on the device: 8192 RocketQuat trajectories from solveStream, one Riccati sweep each (5 RKF78 steps per
segment: 3185 right-hand sides per trajectory), 8192 flights under those gains next to the frozen-time ones (tools/lqr_rate.py, riccati=5).
No pass / fail on time: every node is accounted for by its status, nothing non-finite leaves the device, every flight is accounted for.
The figures are printed (one JSON object); DESIGN.md section 5.2 says which of them have been recorded."""
import json
import os
import sys

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_lqr_riccati_at_size(hip_lib):
    import __graft_entry__ as g

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lqr_rate

    lqr = os.environ.get("SCPP_LQR_LIBRARY") or (g.LQR_LIB if os.path.exists(g.LQR_LIB) else g.build_lqr())
    r = lqr_rate.measure(8192, repeat=2, library=hip_lib, lqr_library=lqr, riccati=5)
    print(json.dumps(r, indent=1))
    assert r["riccati_nodes"] == 8192 * 50 and r["riccati_rhs"] == 8192 * 49 * 5 * 13
    assert r["riccati_status_ok"] + r["riccati_status_nonfinite"] == r["riccati_nodes"] and r["riccati_status_other"] == 0
    assert r["riccati_steps_behind_node0"] in (0, 49 * 5)
    assert r["riccati_gains_nonfinite_values"] == 0 and r["riccati_output_nonfinite_values"] == 0
    assert r["riccati_flights_completed"] + r["riccati_flights_step_cap"] + r["riccati_flights_nonfinite"] == 8192
    assert r["riccati_flights_finite"] == 8192 - r["riccati_flights_nonfinite"]
    assert r["riccati_wall_s"] > 0 and len(r["riccati_final_error_p5_p50_p95"]) == 3
    # the frozen-time leg of the same run: its keys and their meaning are unchanged
    assert r["gain_nodes"] == 8192 * 50 and r["gains_nonfinite_values"] == 0 and r["output_nonfinite_values"] == 0

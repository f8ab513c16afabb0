"""LQR tracking at size on the device: 8192 RocketQuat trajectories from solveStream, gains for all 409 600 nodes, 8192 flights from the
randomised initial states (tools/lqr_rate.py).  No pass / fail on time: every gain status is 0 or counted and reported, nothing non-finite
leaves the device.  The figures are printed; the recorded ones are in profiles/r07_lqr_rate.json and DESIGN.md section 5."""
import json
import os
import sys

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_lqr_at_size(hip_lib):
    import __graft_entry__ as g

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lqr_rate

    lqr = os.environ.get("SCPP_LQR_LIBRARY") or (g.LQR_LIB if os.path.exists(g.LQR_LIB) else g.build_lqr())
    r = lqr_rate.measure(8192, repeat=2, library=hip_lib, lqr_library=lqr)
    print(json.dumps(r, indent=1))
    assert r["gain_nodes"] == 8192 * 50
    assert r["gain_status_ok"] + r["gain_status_iteration_limit"] + r["gain_status_nonfinite"] == r["gain_nodes"]
    assert r["gains_nonfinite_values"] == 0 and r["output_nonfinite_values"] == 0
    # every flight is accounted for by its status (completed, step cap, retired non-finite), and the count the entry point returns agrees
    assert r["flights_completed"] + r["flights_step_cap"] + r["flights_nonfinite"] == 8192
    assert r["flights_finite"] == 8192 - r["flights_nonfinite"]
    assert r["tracked_plant_steps"] > 0

"""Sampled-data LQR gains at size on the device: 1024 RocketQuat trajectories from solveStream, one discrete Riccati recursion each (5 RKF78
steps per segment for [Phi | Gamma]), 1024 flights under those gains with the feedback term held over a segment, next to the frozen-time
leg (tools/lqr_rate.py, discrete=5).  No pass / fail on time: every node is accounted for by its status, nothing non-finite leaves the
device, every flight is accounted for, and the keys of the other legs are what they are without this one.  The figures are printed (one
JSON object); DESIGN.md section 5.2 says which of them have been recorded."""
import json
import os
import sys

import pytest

from conftest import ROOT

DEFAULT_KEYS = {
    "workload", "n", "K", "scvx_converged", "solve_wall_s", "gain_nodes", "gain_status_ok", "gain_status_iteration_limit", "gain_status_nonfinite",
    "gains_nonfinite_values", "sign_iterations_per_node", "sign_iterations_max", "gains_wall_s", "gains_per_s", "track_wall_s",
    "tracked_plant_steps", "tracked_plant_steps_per_s", "flights_finite", "flights_completed", "flights_step_cap", "flights_nonfinite",
    "output_nonfinite_values", "final_error_p5_p50_p95", "initial_error_p50", "max_excursion_p50", "timing",
}


@pytest.mark.gpu
def test_lqr_discrete_at_size(hip_lib):
    import __graft_entry__ as g

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lqr_rate

    n = 1024
    lqr = os.environ.get("SCPP_LQR_LIBRARY") or (g.LQR_LIB if os.path.exists(g.LQR_LIB) else g.build_lqr())
    r = lqr_rate.measure(n, repeat=2, library=hip_lib, lqr_library=lqr, discrete=5)
    print(json.dumps(r, indent=1))
    assert r["discrete_nodes"] == n * 50 and r["discrete_rhs"] == n * 49 * 5 * 13
    assert r["discrete_status_ok"] + r["discrete_status_nonfinite"] == r["discrete_nodes"] and r["discrete_status_other"] == 0
    assert r["discrete_status_ok"] > 0 and r["discrete_steps_behind_node0"] in (0, 49 * 5)
    assert r["discrete_gains_nonfinite_values"] == 0 and r["discrete_output_nonfinite_values"] == 0
    assert r["discrete_flights_completed"] + r["discrete_flights_step_cap"] + r["discrete_flights_nonfinite"] == n
    assert r["discrete_flights_finite"] == n - r["discrete_flights_nonfinite"]
    assert r["discrete_hold"] == "node" and r["discrete_wall_s"] > 0 and r["discrete_track_wall_s"] > 0
    assert len(r["discrete_final_error_p5_p50_p95"]) == 3
    # the frozen-time leg of the same run: its keys and their meaning are unchanged, and the new leg adds discrete_* only
    assert {k for k in r if not k.startswith("discrete_")} == DEFAULT_KEYS
    assert r["gain_nodes"] == n * 50 and r["gains_nonfinite_values"] == 0 and r["output_nonfinite_values"] == 0
    assert r["flights_completed"] + r["flights_step_cap"] + r["flights_nonfinite"] == n

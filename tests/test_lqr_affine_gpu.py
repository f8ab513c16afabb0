"""The affine finite-horizon sweep at size on the device: 256 RocketQuat trajectories from solveStream, the Riccati sweep and the affine sweep
timed in the same run (5 RKF78 steps per segment), 256 flights with the feedforward term and 256 without (tools/lqr_rate.py, riccati=5,
affine=5).  No pass / fail on time: every node is accounted for by its status, nothing non-finite is downloaded, every flight is accounted
for.  The figures are printed (one JSON object); DESIGN.md section 5.2 records those of the 8192-trajectory run."""
import json
import os
import sys

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_lqr_affine_at_size(hip_lib):
    import __graft_entry__ as g

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lqr_rate

    n = 256
    lqr = os.environ.get("SCPP_LQR_LIBRARY") or (g.LQR_LIB if os.path.exists(g.LQR_LIB) else g.build_lqr())
    r = lqr_rate.measure(n, repeat=2, library=hip_lib, lqr_library=lqr, riccati=5, affine=5)
    print(json.dumps(r, indent=1))
    assert r["affine_nodes"] == n * 50 and r["affine_rhs"] == n * 49 * 5 * 13
    assert r["affine_status_ok"] + r["affine_status_nonfinite"] == r["affine_nodes"] and r["affine_status_other"] == 0
    assert r["affine_status_ok"] > 0 and r["affine_status_ok"] <= r["affine_riccati_status_ok"]  # p and s can fail a node that P alone passes
    assert r["affine_steps_behind_node0"] in (0, 49 * 5)
    assert r["affine_nonfinite_values"] == 0
    assert r["affine_wall_s"] > 0 and r["affine_riccati_wall_s"] > 0
    for key in ("affine_ff", "affine_noff"):
        assert r[f"{key}_flights_completed"] + r[f"{key}_flights_step_cap"] + r[f"{key}_flights_nonfinite"] == n
        assert r[f"{key}_output_nonfinite_values"] == 0 and len(r[f"{key}_final_error_p5_p50_p95"]) == 3
    # the legs before it are what they are without it
    assert r["riccati_nodes"] == n * 50 and r["gain_nodes"] == n * 50 and r["riccati_gains_nonfinite_values"] == 0
    # without the term the flights are the Riccati leg's
    assert r["affine_noff_final_error_p5_p50_p95"] == r["riccati_final_error_p5_p50_p95"]

"""LQR tracking at size (for the record and for rocprofv3): N RocketQuat trajectories from SCvxAlgorithm.solveStream, one LQR gain per node
(N x 50), N tracked flights of the nonlinear plant from the randomised initial states.  Prints one JSON line.

    python tools/lqr_rate.py [--n 8192] [--repeat 3] [--riccati STEPS] [--covariance STEPS] [--out FILE]

--riccati STEPS (measure(riccati=STEPS)) adds a leg with the finite-horizon gains: one Riccati sweep per trajectory (STEPS RKF78 steps per
segment), the same N flights under those gains.  It only ADDS keys (riccati_*); the others keep their meaning.

--covariance STEPS (measure(covariance=STEPS)) adds the closed-loop covariance sweep of every trajectory (STEPS RKF78 steps per segment) under
the gains the tracker holds at that point: the Riccati gains when --riccati is given too, else the frozen-time ones.  It only ADDS keys
(covariance_*).  The initial covariance is diagonal: 1 % of the largest |state| over the batch (a floor of 1e-3) as the standard deviation of
every state; the disturbance intensity is 1 % of that variance per second.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import scpp_amd  # noqa: E402


def measure(n=8192, K=50, repeat=3, slots=4096, library=None, lqr_library=None, riccati=None, covariance=None):
    model = scpp_amd.RocketQuat().loadParameters()
    x0 = model.randomized_initial_states(n)
    alg = scpp_amd.SCvxAlgorithm(model, K=K, batch_max=min(slots, n), library=library).initialize()
    alg.solveStream(x0[:min(n, 256)])  # warm
    t = time.perf_counter()
    nconv = alg.solveStream(x0)
    sol = alg.getStreamSolution()
    t_solve = time.perf_counter() - t
    alg.ctx.close()
    trk = scpp_amd.LQRTracker(model, sol["X"], sol["U"], sol["sigma"], library=lqr_library, compute=False)
    trk.ctx.compute_gains()  # warm (first launch loads the code object)
    trk.ctx.synchronize()
    tg = []
    for _ in range(repeat):
        t = time.perf_counter()
        n_ok = trk.ctx.compute_gains()  # returns after the status of every node is on the host
        tg.append(time.perf_counter() - t)
    trk.computeGains()
    st, it = trk.status, trk.iterations
    tt = []
    for _ in range(repeat):
        t = time.perf_counter()
        out = trk.track(x0)
        tt.append(time.perf_counter() - t)
    ric = riccati_leg(trk, x0, int(riccati), repeat) if riccati else {}
    if covariance:
        ric.update(covariance_leg(trk, int(covariance), repeat, "riccati" if riccati else "frozen"))
    trk.close()
    fin = out["status"] != -2
    e = out["err1"][fin]
    q = [float(v) for v in np.percentile(e, [5, 50, 95])] if e.size else []
    res = {
        "workload": f"{n} RocketQuat trajectories x {K} nodes: LQR gains (tangent system, 26 x 26 Hamiltonian), {n} tracked flights, time step 0.01 s, 20 RKF78 steps each",
        "n": int(n), "K": int(K), "scvx_converged": int(nconv), "solve_wall_s": t_solve,
        "gain_nodes": int(st.size), "gain_status_ok": int(n_ok), "gain_status_iteration_limit": int((st == -1).sum()), "gain_status_nonfinite": int((st == -2).sum()),
        "gains_nonfinite_values": int((~np.isfinite(trk.gains)).sum()),
        "sign_iterations_per_node": float(it[st == 0].mean()) if (st == 0).any() else None, "sign_iterations_max": int(it.max()),
        "gains_wall_s": min(tg), "gains_per_s": st.size / min(tg),
        "track_wall_s": min(tt), "tracked_plant_steps": int(out["steps"].sum()), "tracked_plant_steps_per_s": float(out["steps"].sum() / min(tt)),
        "flights_finite": int(out["n_finite"]), "flights_completed": int((out["status"] == 0).sum()), "flights_step_cap": int((out["status"] == 1).sum()),
        "flights_nonfinite": int((out["status"] == -2).sum()),
        "output_nonfinite_values": int(sum((~np.isfinite(out[k])).sum() for k in ("x", "u", "t", "err0", "err1", "max_dev"))),
        "final_error_p5_p50_p95": q, "initial_error_p50": float(np.median(out["err0"][fin])) if fin.any() else None,
        "max_excursion_p50": float(np.median(out["max_dev"][fin])) if fin.any() else None,
        "timing": f"wall clock, best of {repeat}; gains include the download of the per-node status, flights the upload of the starts and the download of the results",
    }
    res.update(ric)
    return res


def riccati_leg(trk, x0, steps, repeat):
    """finite-horizon gains on the tracker's trajectories, then the same flights under them"""
    trk.ctx.compute_gains_riccati(steps)  # warm
    tr = []
    for _ in range(repeat):
        t = time.perf_counter()
        n_ok = trk.ctx.compute_gains_riccati(steps)  # returns after the status of every node is on the host
        tr.append(time.perf_counter() - t)
    trk.computeGainsRiccati(steps, keep=False)
    st, it = trk.status, trk.iterations
    out = trk.track(x0)
    fin = out["status"] != -2
    e = out["err1"][fin]
    rhs = trk.B * (trk.K - 1) * steps * 13
    return {
        "riccati_steps_per_segment": steps, "riccati_wall_s": min(tr), "riccati_rhs": int(rhs), "riccati_rhs_per_s": rhs / min(tr),
        "riccati_nodes": int(st.size), "riccati_status_ok": int(n_ok), "riccati_status_nonfinite": int((st == -2).sum()),
        "riccati_status_other": int(((st != 0) & (st != -2)).sum()), "riccati_gains_nonfinite_values": int((~np.isfinite(trk.gains)).sum()),
        "riccati_steps_behind_node0": int(it[:, 0].max()),
        "riccati_flights_finite": int(out["n_finite"]), "riccati_flights_completed": int((out["status"] == 0).sum()),
        "riccati_flights_step_cap": int((out["status"] == 1).sum()), "riccati_flights_nonfinite": int((out["status"] == -2).sum()),
        "riccati_output_nonfinite_values": int(sum((~np.isfinite(out[k])).sum() for k in ("x", "u", "t", "err0", "err1", "max_dev"))),
        "riccati_final_error_p5_p50_p95": [float(v) for v in np.percentile(e, [5, 50, 95])] if e.size else [],
        "riccati_max_excursion_p50": float(np.median(out["max_dev"][fin])) if fin.any() else None,
    }


def covariance_leg(trk, steps, repeat, law):
    """the closed-loop covariance sweep on the tracker's trajectories under the gains it holds"""
    sd = np.maximum(0.01 * np.nanmax(np.abs(trk.X), axis=(0, 1)), 1e-3)
    sigma0, w = np.diag(sd * sd), 0.01 * sd * sd
    trk.ctx.set_covariance_inputs(sigma0, w)
    trk.ctx.propagate_covariance(steps)  # warm
    tc = []
    for _ in range(repeat):
        t = time.perf_counter()
        n_ok = trk.ctx.propagate_covariance(steps)  # returns after the status of every trajectory is on the host
        tc.append(time.perf_counter() - t)
    o = trk.ctx.download_covariance()
    st = o["status"]
    ok = st != -2
    rhs = trk.B * (trk.K - 1) * steps * 13
    pos = np.sqrt((o["state_std"][ok, -1, 1:4] ** 2).sum(axis=1))  # RocketQuat: states 1..3 are the position
    # inputs 0..2 are the thrust vector (input 3: the roll torque); 3 sigma of its norm at every node
    thrust = 3.0 * np.sqrt(np.maximum(np.trace(o["input_cov"][ok][:, :, :3, :3], axis1=2, axis2=3), 0.0)) if ok.any() else np.zeros(0)
    return {
        "covariance_steps_per_segment": steps, "covariance_gains": law, "covariance_wall_s": min(tc), "covariance_rhs": int(rhs),
        "covariance_rhs_per_s": rhs / min(tc), "covariance_trajectories": int(st.size), "covariance_nodes": int(st.size * trk.K),
        "covariance_status_ok": int(n_ok), "covariance_status_gains_incomplete": int((st == 2).sum()),
        "covariance_status_nonfinite": int((st == -2).sum()), "covariance_status_other": int(((st != 0) & (st != 2) & (st != -2)).sum()),
        "covariance_nonfinite_values": int(sum((~np.isfinite(o[k])).sum() for k in ("state_std", "input_cov", "final_cov"))),
        "covariance_final_position_std_p5_p50_p95": [float(v) for v in np.percentile(pos, [5, 50, 95])] if pos.size else [],
        "covariance_thrust_3sigma_max": float(thrust.max()) if thrust.size else 0.0,
        "covariance_thrust_3sigma_p50": float(np.median(thrust.max(axis=1))) if thrust.size else 0.0,
        "covariance_initial_std": [float(v) for v in sd],
    }


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--riccati", type=int, default=0, help="RKF78 steps per segment of the finite-horizon leg (0: no such leg)")
    ap.add_argument("--covariance", type=int, default=0, help="RKF78 steps per segment of the covariance leg (0: no such leg)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.n, repeat=a.repeat, riccati=a.riccati, covariance=a.covariance)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

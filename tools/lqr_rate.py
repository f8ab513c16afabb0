"""LQR tracking at size (for the record and for rocprofv3): N RocketQuat trajectories from SCvxAlgorithm.solveStream, one LQR gain per node
(N x 50), N tracked flights of the nonlinear plant from the randomised initial states.  Prints one JSON line.

    python tools/lqr_rate.py [--n 8192] [--repeat 3] [--riccati STEPS] [--covariance STEPS] [--saturate] [--samples N[,N..]] [--discrete STEPS] [--covariance-discrete STEPS] [--filter STEPS]
                             [--affine STEPS] [--moments STEPS] [--disturbance] [--out FILE]

--riccati STEPS (measure(riccati=STEPS)) adds a leg with the finite-horizon gains: one Riccati sweep per trajectory (STEPS RKF78 steps per
segment), the same N flights under those gains.  It only ADDS keys (riccati_*); the others keep their meaning.

--covariance STEPS (measure(covariance=STEPS)) adds the closed-loop covariance sweep of every trajectory (STEPS RKF78 steps per segment) under
the gains the tracker holds at that point: the Riccati gains when --riccati is given too, else the frozen-time ones.  It only ADDS keys
(covariance_*).  The initial covariance is diagonal: 1 % of the largest |state| over the batch (a floor of 1e-3) as the standard deviation of
every state; the disturbance intensity is 1 % of that variance per second.

--saturate (measure(saturate=True)) flies the N flights of the default leg again, from the same starts and under the same frozen-time gains,
with the input limits of the model's parameters inside the loop (LQRTracker.setInputLimits("model")), and once more without them timed the
same way.  It only ADDS keys (saturate_*): the time of the flight call with and without limits and their ratio, plant steps/s, the share
of flights with n_sat > 0, and the final errors with and without limits on the same starts.

--samples N[,N..] (measure(samples=[..])) flies, for each N, N flights per trajectory as one fan (scpp_hip_lqr_track_samples) under the
frozen-time gains, without limits unless --saturate is given too: flight 0 of a trajectory starts where the trajectory was solved from, the
others 1 % (Gaussian, fixed seed) off that state.  It only ADDS the key samples_legs, one entry per N.

--discrete STEPS (measure(discrete=STEPS)) adds, after every other leg, the sampled-data gains: one discrete Riccati recursion per trajectory
(STEPS RKF78 steps per segment for the transition matrices), then the N flights of the default leg under those gains with the feedback term
held over a segment (track(hold="node")).  It only ADDS keys (discrete_*): the sweep's wall time, transition right-hand sides/s, the status
counts and the flights.

--covariance-discrete STEPS (measure(covariance_discrete=STEPS)) adds, last of all, the covariance sweep of the loop that holds its correction
over a segment (LQRTracker.covariance(hold="node"), STEPS RKF78 steps per segment for the transition matrices and for the accumulated
disturbance) under the gains the tracker holds at that point: the sampled-data gains when --discrete is given too.  Inputs as the covariance
leg's.  It only ADDS keys (covariance_discrete_*): the sweep's wall time, right-hand sides/s (one counted per stage; with a disturbance every
stage evaluates the Jacobian twice), the status counts and the final position standard deviation, next to the continuous sweep's under the
same gains and inputs in the same run (covariance_discrete_continuous_*).

--affine STEPS (measure(affine=STEPS)) adds, after every other leg, the affine finite-horizon sweep (gains and feedforward terms against the
defect of the solver's trajectories, STEPS RKF78 steps per segment), timed next to the Riccati sweep at the same STEPS IN THE SAME RUN
(affine_riccati_wall_s: the yardstick of affine_wall_s), then the N flights of the default leg under those gains with the feedforward term and
without it.  It only ADDS keys (affine_*): the two wall times and their ratio, right-hand sides/s, the status counts, and per flight leg the
final errors (err1) and the largest excursion (max_dev): nothing of it needs a record.

--moments STEPS (measure(moments=STEPS)) adds, last of all, the sweep of the closed-loop mean next to the covariance
(LQRTracker.moments, STEPS RKF78 steps per segment) under the affine law's gains, which the leg computes itself, timed next to the covariance
sweep on the same gains and inputs IN THE SAME RUN (moments_covariance_wall_s: the yardstick of moments_wall_s), with the feedforward term
and without it.  It only ADDS keys (moments_*): the wall times and their ratio, right-hand sides/s, the status counts, and per trajectory
the split of the final error: |m(T)| with and without the term (where the linearised loop's centre ends relative to the nominal's last
node), |X[K-1] - x_final| (the nominal's own last node against the target) and the flown |x(T) - X[K-1]| of the default leg's flights under
the same gains, each as 5 / 50 / 95 % over the trajectories.

--disturbance (measure(disturbance=True)) flies, right after the default leg and under its frozen-time gains, the N flights of the default leg
with process noise on the plant (LQRTracker.track(disturbance=w); w is the covariance leg's intensity: 1 % of the initial variance per
second) and once more without it, timed the same way IN THE SAME RUN.  It only ADDS keys (disturbance_*): the two flight-call times and
their ratio, plant steps/s with and without noise, and the status counts.  Together with --samples N[,..] and --covariance STEPS it also
flies a fan of N (the first of the list) disturbed flights per trajectory, all from the start the trajectory was solved from, and reports the
fan's sample standard deviation of the final position (per trajectory, over its N flights) next to the covariance sweep's under the same
gains, the same w and sigma0 = 0: 5 / 50 / 95 % over the trajectories of both and of their ratio, and the pooled ratio sqrt(mean fan
variance / mean sweep variance).

--filter STEPS (measure(filter=STEPS)) adds, right after the covariance leg and under the same gains, the filter sweep
(LqrContext.filter, STEPS RKF78 steps per segment, taken as given): the Kalman-Bucy error covariance alone (filter_alone_*) and together with
the covariance of the estimate under the loop closed on it (filter_loop_*), next to the covariance sweep on the same gains and inputs IN THE
SAME RUN (filter_covariance_wall_s: the yardstick).  sigma0 and w are the covariance leg's; the sensors read r, v and q (ny = 10) with
v_m = 8 h (H sigma0 H')_mm, h = the largest dt of the batch / STEPS, which is h rho = 1/8, the front ends' step rule.  It only ADDS keys:
wall times, right-hand sides/s (one counted per stage), status counts and non-finite values of both variants.

The flight call of the saturate, samples and disturbance legs is timed at the context (upload of the starts, the kernel, the synchronisation; no download of results),
best of --repeat.
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


def measure(n=8192, K=50, repeat=3, slots=4096, library=None, lqr_library=None, riccati=None, covariance=None, saturate=False, samples=(), discrete=None,
            covariance_discrete=None, affine=None, moments=None, disturbance=False, filter=None):
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
    sat = saturate_leg(trk, x0, repeat) if saturate else {}
    if samples:
        sat["samples_legs"] = [samples_leg(trk, x0, int(N), repeat, bool(saturate)) for N in samples]
    if disturbance:
        sat.update(disturbance_leg(trk, x0, repeat, int(samples[0]) if samples else 0, int(covariance or 0)))
    ric = riccati_leg(trk, x0, int(riccati), repeat) if riccati else {}
    if covariance:
        ric.update(covariance_leg(trk, int(covariance), repeat, "riccati" if riccati else "frozen"))
    if filter:
        ric.update(filter_leg(trk, int(filter), repeat, "riccati" if riccati else "frozen"))
    if discrete:
        ric.update(discrete_leg(trk, x0, int(discrete), repeat))
    if covariance_discrete:
        ric.update(covariance_discrete_leg(trk, int(covariance_discrete), repeat, "discrete" if discrete else "riccati" if riccati else "frozen"))
    if affine:
        ric.update(affine_leg(trk, x0, int(affine), repeat))
    if moments:
        ric.update(moments_leg(trk, x0, int(moments), repeat))
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
    res.update(sat)
    res.update(ric)
    return res


def time_flights(trk, xs, samples, repeat):
    """best-of-repeat wall time of the flight call alone (upload of the starts, kernel, synchronisation), then the downloaded results"""
    x_final = np.array(list(trk.model.p.x_final), dtype=np.float64)
    max_steps = int(np.ceil(float(np.nanmax(trk.t)) / 0.01)) + 2
    tt = []
    for _ in range(repeat + 1):  # the first call is the warm-up (code object of this instantiation, growth of the flight buffers)
        t = time.perf_counter()
        trk.ctx.track_samples(xs, x_final, samples, 0.01, 20, max_steps)
        tt.append(time.perf_counter() - t)
    out = trk.ctx.track_download()
    out.update(trk.ctx.track_download_saturation())
    return min(tt[1:]), out


def final_errors(out):
    e = out["err1"][out["status"] != -2]
    return [float(v) for v in np.percentile(e, [5, 50, 95])] if e.size else []


def saturate_leg(trk, x0, repeat):
    """the default leg's flights with the model's input limits in the loop, and without them, timed the same way on the same starts"""
    trk.setInputLimits(None)
    t_off, off = time_flights(trk, x0, 1, repeat)
    trk.setInputLimits("model")
    t_on, on = time_flights(trk, x0, 1, repeat)
    trk.setInputLimits(None)
    steps = int(on["steps"].sum())
    return {
        "saturate_limits": [float(v) for v in scpp_amd.model_input_limits(trk.model)],
        "saturate_flight_call_s": t_on, "saturate_off_flight_call_s": t_off, "saturate_over_off": t_on / t_off,
        "saturate_plant_steps": steps, "saturate_plant_steps_per_s": steps / t_on,
        "saturate_off_plant_steps": int(off["steps"].sum()), "saturate_off_plant_steps_per_s": float(off["steps"].sum() / t_off),
        "saturate_flights_clipped_share": float((on["n_sat"] > 0).mean()), "saturate_steps_clipped_share": float(on["n_sat"].sum() / max(steps, 1)),
        "saturate_max_clip_p50_max": [float(np.median(on["max_clip"])), float(on["max_clip"].max())],
        "saturate_flights_completed": int((on["status"] == 0).sum()), "saturate_flights_nonfinite": int((on["status"] == -2).sum()),
        "saturate_final_error_p5_p50_p95": final_errors(on), "saturate_off_final_error_p5_p50_p95": final_errors(off),
        "saturate_off_n_sat_total": int(off["n_sat"].sum()),
    }


def disturbance_leg(trk, x0, repeat, N, cov_steps, seed=20261020):
    """the default leg's flights with process noise on the plant and without it, timed the same way on the same starts; with N and cov_steps
    a fan of N disturbed flights per trajectory from the trajectory's own start against the covariance sweep from sigma0 = 0"""
    sd = np.maximum(0.01 * np.nanmax(np.abs(trk.X), axis=(0, 1)), 1e-3)
    w = 0.01 * sd * sd  # the covariance leg's disturbance intensity
    trk.setInputLimits(None)
    trk.ctx.set_disturbance(None)
    t_off, off = time_flights(trk, x0, 1, repeat)
    trk.ctx.set_disturbance(w, seed, 0)
    t_on, on = time_flights(trk, x0, 1, repeat)
    steps = int(on["steps"].sum())
    res = {
        "disturbance_intensity": [float(v) for v in w], "disturbance_seed": int(seed),
        "disturbance_flight_call_s": t_on, "disturbance_off_flight_call_s": t_off, "disturbance_over_off": t_on / t_off,
        "disturbance_plant_steps": steps, "disturbance_plant_steps_per_s": steps / t_on,
        "disturbance_off_plant_steps": int(off["steps"].sum()), "disturbance_off_plant_steps_per_s": float(off["steps"].sum() / t_off),
        "disturbance_flights_completed": int((on["status"] == 0).sum()), "disturbance_flights_nonfinite": int((on["status"] == -2).sum()),
        "disturbance_final_error_p5_p50_p95": final_errors(on), "disturbance_off_final_error_p5_p50_p95": final_errors(off),
    }
    if N > 1 and cov_steps > 0:
        nx = x0.shape[1]
        t_fan, fan = time_flights(trk, np.repeat(x0, N, axis=0), N, repeat)
        trk.ctx.set_covariance_inputs(np.zeros((nx, nx)), w)
        n_ok = trk.ctx.propagate_covariance(cov_steps)
        o = trk.ctx.download_covariance()
        done = (fan["status"].reshape(-1, N) == 0).all(axis=1) & (o["status"] != -2)
        pos = fan["x"].reshape(-1, N, nx)[done][:, :, 1:4]  # RocketQuat: states 1..3 are the position
        fan_var = pos.var(axis=1, ddof=1).sum(axis=1)
        sweep_var = (o["state_std"][done, -1, 1:4] ** 2).sum(axis=1)
        pct = lambda v: [float(q) for q in np.percentile(v, [5, 50, 95])] if v.size else []  # noqa: E731
        res.update({
            "disturbance_fan_samples": N, "disturbance_fan_flights": int(fan["x"].shape[0]), "disturbance_fan_flight_call_s": t_fan,
            "disturbance_fan_plant_steps_per_s": float(fan["steps"].sum() / t_fan), "disturbance_fan_trajectories_compared": int(done.sum()),
            "disturbance_sweep_steps_per_segment": cov_steps, "disturbance_sweep_status_ok": int(n_ok),
            "disturbance_fan_final_position_std_p5_p50_p95": pct(np.sqrt(fan_var)),
            "disturbance_sweep_final_position_std_p5_p50_p95": pct(np.sqrt(sweep_var)),
            "disturbance_fan_over_sweep_p5_p50_p95": pct(np.sqrt(fan_var / sweep_var)),
            "disturbance_fan_over_sweep_pooled": float(np.sqrt(fan_var.mean() / sweep_var.mean())) if done.any() else None,
        })
    trk.ctx.set_disturbance(None)
    return res


def samples_leg(trk, x0, N, repeat, saturate):
    """N flights per trajectory as one fan: flight 0 from the trajectory's own start, the others 1 % off it"""
    xs = np.repeat(x0, N, axis=0).reshape(x0.shape[0], N, -1)
    xs[:, 1:] *= 1.0 + 0.01 * np.random.default_rng(20261018).standard_normal(xs[:, 1:].shape)
    xs = xs.reshape(-1, x0.shape[1])
    trk.setInputLimits("model" if saturate else None)
    t, out = time_flights(trk, xs, N, repeat)
    trk.setInputLimits(None)
    steps = int(out["steps"].sum())
    return {
        "samples": N, "flights": int(xs.shape[0]), "limits": bool(saturate), "flight_call_s": t, "plant_steps": steps, "plant_steps_per_s": steps / t,
        "wavefronts": int((xs.shape[0] + 63) // 64), "flights_completed": int((out["status"] == 0).sum()),
        "flights_nonfinite": int((out["status"] == -2).sum()), "flights_clipped_share": float((out["n_sat"] > 0).mean()),
        "final_error_p5_p50_p95": final_errors(out),
    }


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


def affine_leg(trk, x0, steps, repeat):
    """the affine sweep on the tracker's trajectories next to the Riccati sweep at the same step count, then the default leg's flights under its
    gains with and without the feedforward term"""
    def timed(sweep):
        sweep(steps)  # warm
        tc = []
        for _ in range(repeat):
            t = time.perf_counter()
            n_ok = sweep(steps)  # returns after the status of every node is on the host
            tc.append(time.perf_counter() - t)
        return min(tc), n_ok

    t_r, ok_r = timed(trk.ctx.compute_gains_riccati)
    t_a, n_ok = timed(trk.ctx.compute_gains_affine)
    trk.computeGainsAffine(steps, keep=False)
    st, it, ff = trk.status, trk.iterations, trk.affine()["ff"]
    rhs = trk.B * (trk.K - 1) * steps * 13
    res = {
        "affine_steps_per_segment": steps, "affine_wall_s": t_a, "affine_riccati_wall_s": t_r, "affine_over_riccati": t_a / t_r,
        "affine_rhs": int(rhs), "affine_rhs_per_s": rhs / t_a, "affine_nodes": int(st.size), "affine_status_ok": int(n_ok),
        "affine_riccati_status_ok": int(ok_r), "affine_status_nonfinite": int((st == -2).sum()),
        "affine_status_other": int(((st != 0) & (st != -2)).sum()),
        "affine_nonfinite_values": int((~np.isfinite(trk.gains)).sum() + (~np.isfinite(ff)).sum()),
        "affine_steps_behind_node0": int(it[:, 0].max()),
        "affine_feedforward_norm_p50_max": [float(v) for v in np.percentile(np.linalg.norm(ff, axis=2).max(axis=1), [50, 100])],
    }
    for key, on in (("affine_ff", True), ("affine_noff", False)):
        out = trk.track(x0, feedforward=on)
        fin = out["status"] != -2
        res.update({
            f"{key}_flights_completed": int((out["status"] == 0).sum()), f"{key}_flights_step_cap": int((out["status"] == 1).sum()),
            f"{key}_flights_nonfinite": int((out["status"] == -2).sum()),
            f"{key}_output_nonfinite_values": int(sum((~np.isfinite(out[k])).sum() for k in ("x", "u", "t", "err0", "err1", "max_dev"))),
            f"{key}_final_error_p5_p50_p95": final_errors(out),
            f"{key}_max_excursion_p5_p50_p95": [float(v) for v in np.percentile(out["max_dev"][fin], [5, 50, 95])] if fin.any() else [],
        })
    trk.ctx.set_feedforward(0)
    return res


def moments_leg(trk, x0, steps, repeat):
    """the moments sweep on the tracker's trajectories under the affine law next to the covariance sweep on the same gains and inputs, then the
    split of the final error: the predicted mean at T, the nominal's last node against the target, and the flown distance to that node"""
    trk.computeGainsAffine(steps, keep=False)
    sd = np.maximum(0.01 * np.nanmax(np.abs(trk.X), axis=(0, 1)), 1e-3)
    trk.ctx.set_covariance_inputs(np.diag(sd * sd), 0.01 * sd * sd)

    def timed(sweep):
        sweep()  # warm
        tc = []
        for _ in range(repeat):
            t = time.perf_counter()
            n_ok = sweep()  # returns after the status of every trajectory is on the host
            tc.append(time.perf_counter() - t)
        return min(tc), n_ok

    def pct(v):
        v = v[np.isfinite(v)]
        return [float(q) for q in np.percentile(v, [5, 50, 95])] if v.size else []

    t_c, ok_c = timed(lambda: trk.ctx.propagate_covariance(steps))
    cov = trk.ctx.download_covariance()
    x_final = np.array(list(trk.model.p.x_final), dtype=np.float64)
    rhs = trk.B * (trk.K - 1) * steps * 13
    res = {"moments_steps_per_segment": steps, "moments_covariance_wall_s": t_c, "moments_covariance_status_ok": int(ok_c), "moments_rhs": int(rhs),
           "moments_covariance_rhs_per_s": rhs / t_c, "moments_trajectories": int(trk.B),
           "moments_nominal_last_node_to_target_p5_p50_p95": pct(np.linalg.norm(trk.X[:, -1] - x_final, axis=1))}
    for key, on in (("moments_ff", True), ("moments_noff", False)):
        t_m, n_ok = timed(lambda: trk.ctx.propagate_moments(steps, False, on))
        o = trk.ctx.download_covariance()
        o.update(trk.ctx.download_moments())
        st = o["status"]
        ok = st != -2
        fl = trk.track(x0, feedforward=on)
        fin = ok & (fl["status"] != -2)
        res.update({
            f"{key}_wall_s": t_m, f"{key}_over_covariance": t_m / t_c, f"{key}_rhs_per_s": rhs / t_m, f"{key}_status_ok": int(n_ok),
            f"{key}_status_gains_incomplete": int((st == 2).sum()), f"{key}_status_nonfinite": int((st == -2).sum()),
            f"{key}_status_other": int(((st != 0) & (st != 2) & (st != -2)).sum()),
            f"{key}_nonfinite_values": int(sum((~np.isfinite(o[k])).sum() for k in ("state_std", "input_cov", "final_cov", "mean", "input_mean"))),
            f"{key}_covariance_block_equal": bool(all(np.array_equal(o[k], cov[k]) for k in ("state_std", "input_cov", "final_cov", "status"))),
            f"{key}_mean_final_norm_p5_p50_p95": pct(np.linalg.norm(o["mean"][ok, -1], axis=1)),
            f"{key}_mean_final_position_p5_p50_p95": pct(np.linalg.norm(o["mean"][ok, -1, 1:4], axis=1)),  # RocketQuat: states 1..3
            f"{key}_input_mean_max_norm_p50_max": [float(v) for v in np.percentile(np.linalg.norm(o["input_mean"][ok], axis=2).max(axis=1), [50, 100])] if ok.any() else [],
            f"{key}_flown_to_last_node_p5_p50_p95": pct(np.linalg.norm(fl["x"][fin] - trk.X[fin, -1], axis=1)),
            f"{key}_flown_minus_mean_p5_p50_p95": pct(np.linalg.norm(fl["x"][fin] - trk.X[fin, -1] - o["mean"][fin, -1], axis=1)),
            f"{key}_flown_final_error_p5_p50_p95": pct(fl["err1"][fin]),
            f"{key}_flights_nonfinite": int((fl["status"] == -2).sum()),
        })
    trk.ctx.set_feedforward(0)
    res["moments_wall_s"], res["moments_over_covariance"] = res["moments_ff_wall_s"], res["moments_ff_over_covariance"]
    return res


def discrete_leg(trk, x0, steps, repeat):
    """sampled-data gains on the tracker's trajectories, then the default leg's flights under them with the feedback term held over a segment"""
    trk.ctx.compute_gains_discrete(steps)  # warm
    td = []
    for _ in range(repeat):
        t = time.perf_counter()
        n_ok = trk.ctx.compute_gains_discrete(steps)  # returns after the status of every node is on the host
        td.append(time.perf_counter() - t)
    trk.computeGainsDiscrete(steps, keep=False)
    st, it = trk.status, trk.iterations
    tt = []
    for _ in range(repeat):
        t = time.perf_counter()
        out = trk.track(x0, hold="node")
        tt.append(time.perf_counter() - t)
    trk.ctx.set_feedback_hold(0)
    fin = out["status"] != -2
    e = out["err1"][fin]
    # RocketQuat integrates every segment twice (Phi, then Gamma): two Jacobian evaluations and two tile products per counted right-hand side
    rhs = trk.B * (trk.K - 1) * steps * 13
    return {
        "discrete_steps_per_segment": steps, "discrete_wall_s": min(td), "discrete_rhs": int(rhs), "discrete_rhs_per_s": rhs / min(td),
        "discrete_nodes": int(st.size), "discrete_status_ok": int(n_ok), "discrete_status_nonfinite": int((st == -2).sum()),
        "discrete_status_other": int(((st != 0) & (st != -2)).sum()), "discrete_gains_nonfinite_values": int((~np.isfinite(trk.gains)).sum()),
        "discrete_steps_behind_node0": int(it[:, 0].max()),
        "discrete_hold": "node", "discrete_track_wall_s": min(tt), "discrete_tracked_plant_steps": int(out["steps"].sum()),
        "discrete_tracked_plant_steps_per_s": float(out["steps"].sum() / min(tt)),
        "discrete_flights_finite": int(out["n_finite"]), "discrete_flights_completed": int((out["status"] == 0).sum()),
        "discrete_flights_step_cap": int((out["status"] == 1).sum()), "discrete_flights_nonfinite": int((out["status"] == -2).sum()),
        "discrete_output_nonfinite_values": int(sum((~np.isfinite(out[k])).sum() for k in ("x", "u", "t", "err0", "err1", "max_dev"))),
        "discrete_final_error_p5_p50_p95": [float(v) for v in np.percentile(e, [5, 50, 95])] if e.size else [],
        "discrete_max_excursion_p50": float(np.median(out["max_dev"][fin])) if fin.any() else None,
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


def filter_leg(trk, steps, repeat, law):
    """the filter sweep on the tracker's trajectories, alone and with the loop's tile under the gains held, and the covariance sweep next to it"""
    sd = np.maximum(0.01 * np.nanmax(np.abs(trk.X), axis=(0, 1)), 1e-3)
    sigma0, w = np.diag(sd * sd), 0.01 * sd * sd
    nx = sd.size
    H = np.zeros((10, nx))
    H[np.arange(10), np.arange(1, 11)] = 1.0  # RocketQuat: states 1..10 are r, v, q
    h = float(np.nanmax(trk.t)) / (trk.K - 1) / steps
    v = 8.0 * h * np.einsum("mi,ij,mj->m", H, sigma0, H)
    trk.ctx.set_covariance_inputs(sigma0, w)
    trk.ctx.set_measurement(H, v)
    rhs = trk.B * (trk.K - 1) * steps * 13

    def timed(sweep):
        sweep()  # warm
        tc = []
        for _ in range(repeat):
            t = time.perf_counter()
            n_ok = sweep()  # returns after the status of every trajectory is on the host
            tc.append(time.perf_counter() - t)
        return min(tc), n_ok

    t_c, ok_c = timed(lambda: trk.ctx.propagate_covariance(steps))
    res = {"filter_steps_per_segment": steps, "filter_gains": law, "filter_measurements": 10, "filter_rhs": int(rhs), "filter_trajectories": int(trk.B),
           "filter_covariance_wall_s": t_c, "filter_covariance_status_ok": int(ok_c), "filter_covariance_rhs_per_s": rhs / t_c}
    for key, loop in (("filter_alone", False), ("filter_loop", True)):
        t_f, n_ok = timed(lambda: trk.ctx.filter(steps, loop))
        o = trk.ctx.download_filter(loop)
        st = o["status"]
        ok = st != -2
        std = o["state_std" if loop else "error_std"]
        pos = np.sqrt((std[ok, -1, 1:4] ** 2).sum(axis=1))
        res.update({
            f"{key}_wall_s": t_f, f"{key}_over_covariance": t_f / t_c, f"{key}_rhs_per_s": rhs / t_f, f"{key}_status_ok": int(n_ok),
            f"{key}_status_gains_incomplete": int((st == 2).sum()), f"{key}_status_nonfinite": int((st == -2).sum()),
            f"{key}_status_other": int(((st != 0) & (st != 2) & (st != -2)).sum()),
            f"{key}_nonfinite_values": int(sum((~np.isfinite(a)).sum() for k, a in o.items() if k != "status")),
            f"{key}_final_position_std_p5_p50_p95": [float(q) for q in np.percentile(pos, [5, 50, 95])] if pos.size else [],
        })
    return res


def covariance_discrete_leg(trk, steps, repeat, law):
    """the covariance sweep of the held loop on the tracker's trajectories under the gains it holds, and the continuous sweep next to it"""
    sd = np.maximum(0.01 * np.nanmax(np.abs(trk.X), axis=(0, 1)), 1e-3)
    sigma0, w = np.diag(sd * sd), 0.01 * sd * sd
    trk.ctx.set_covariance_inputs(sigma0, w)

    def timed(sweep):
        sweep(steps)  # warm
        tc = []
        for _ in range(repeat):
            t = time.perf_counter()
            n_ok = sweep(steps)  # returns after the status of every trajectory is on the host
            tc.append(time.perf_counter() - t)
        o = trk.ctx.download_covariance()
        ok = o["status"] != -2
        pos = np.sqrt((o["state_std"][ok, -1, 1:4] ** 2).sum(axis=1))  # RocketQuat: states 1..3 are the position
        return min(tc), n_ok, o, [float(v) for v in np.percentile(pos, [5, 50, 95])] if pos.size else []

    t_c, ok_c, _, pos_c = timed(trk.ctx.propagate_covariance)
    t_d, ok_d, o, pos_d = timed(trk.ctx.propagate_covariance_discrete)
    st = o["status"]
    rhs = trk.B * (trk.K - 1) * steps * 13
    return {
        "covariance_discrete_steps_per_segment": steps, "covariance_discrete_gains": law, "covariance_discrete_wall_s": t_d,
        "covariance_discrete_rhs": int(rhs), "covariance_discrete_rhs_per_s": rhs / t_d, "covariance_discrete_trajectories": int(st.size),
        "covariance_discrete_status_ok": int(ok_d), "covariance_discrete_status_gains_incomplete": int((st == 2).sum()),
        "covariance_discrete_status_nonfinite": int((st == -2).sum()),
        "covariance_discrete_nonfinite_values": int(sum((~np.isfinite(o[k])).sum() for k in ("state_std", "input_cov", "final_cov"))),
        "covariance_discrete_final_position_std_p5_p50_p95": pos_d,
        "covariance_discrete_continuous_wall_s": t_c, "covariance_discrete_continuous_status_ok": int(ok_c),
        "covariance_discrete_continuous_final_position_std_p5_p50_p95": pos_c,
    }


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--riccati", type=int, default=0, help="RKF78 steps per segment of the finite-horizon leg (0: no such leg)")
    ap.add_argument("--covariance", type=int, default=0, help="RKF78 steps per segment of the covariance leg (0: no such leg)")
    ap.add_argument("--saturate", action="store_true", help="the flights again with the model's input limits in the loop")
    ap.add_argument("--samples", default="", help="comma-separated flights per trajectory of the sample-fan legs, e.g. 1,4,16")
    ap.add_argument("--discrete", type=int, default=0, help="RKF78 steps per segment of the sampled-data leg (0: no such leg)")
    ap.add_argument("--covariance-discrete", type=int, default=0, help="RKF78 steps per segment of the held loop's covariance leg (0: no such leg)")
    ap.add_argument("--affine", type=int, default=0, help="RKF78 steps per segment of the affine leg (0: no such leg)")
    ap.add_argument("--moments", type=int, default=0, help="RKF78 steps per segment of the mean-and-covariance leg (0: no such leg)")
    ap.add_argument("--disturbance", action="store_true", help="the flights again with process noise on the plant; with --samples and --covariance also the fan against the sweep")
    ap.add_argument("--filter", type=int, default=0, help="RKF78 steps per segment of the filter leg (0: no such leg)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.n, repeat=a.repeat, riccati=a.riccati, covariance=a.covariance, saturate=a.saturate,
                  samples=[int(v) for v in a.samples.split(",") if v], discrete=a.discrete, covariance_discrete=a.covariance_discrete,
                  affine=a.affine, moments=a.moments, disturbance=a.disturbance, filter=a.filter)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

"""Batched mirrors of the reference's LQR front ends over the C ABI of include/scpp_hip_lqr.h:

    LQRTracker     scpp_core/include/LQRTracker.hpp, src/LQRTracker.cpp:6-65 and the closed loop of scpp/src/SC_tracking.cpp:48-75
    LQRAlgorithm   scpp_core/src/LQRAlgorithm.cpp:6-75 (one gain at the model's operating point)
    LQRSim         scpp/src/LQR_sim.cpp:20-82 (its input clipping, LQR_sim.cpp:55-66, is setInputLimits: off by default)

Every call handles B trajectories / closed loops.  The gains and the flights are computed by the HIP kernels of libscpp_lqr.so; only
getInput (a spot check of one input) is host arithmetic.  There is no CPU fallback."""
import math
import os

import numpy as np

from ._lib import LqrContext
from .parameter_server import ParameterServer


def load_lqr_weights(model):
    """LQRTracker::loadParameters (LQRTracker.cpp:30-41): state_weights / input_weights of <model>/LQR.info; Q = I, R = I without the file."""
    path = os.path.join(model.getParameterFolder(), "LQR.info")
    if not os.path.exists(path):
        return np.ones(model.state_dim), np.ones(model.input_dim)
    ps = ParameterServer(path)
    return (np.array(ps.load_vector("state_weights", model.state_dim), dtype=np.float64),
            np.array(ps.load_vector("input_weights", model.input_dim), dtype=np.float64))


def load_lqr_terminal_weights(model):
    """the optional terminal_weights vector of <model>/LQR.info (diagonal of Qf of the finite-horizon gains); None when the file or the
    vector is absent: Qf = Q"""
    path = os.path.join(model.getParameterFolder(), "LQR.info")
    if not os.path.exists(path):
        return None
    ps = ParameterServer(path)
    if "terminal_weights" not in ps.tree:
        return None
    return np.array(ps.load_vector("terminal_weights", model.state_dim), dtype=np.float64)


def load_lqr_covariance_inputs(model):
    """the optional initial_std and disturbance_std vectors of <model>/LQR.info (standard deviations of the initial state and square roots
    of the disturbance intensity, one entry per state); None for whichever the file does not have"""
    path = os.path.join(model.getParameterFolder(), "LQR.info")
    if not os.path.exists(path):
        return None, None
    ps = ParameterServer(path)
    return tuple(np.array(ps.load_vector(k, model.state_dim), dtype=np.float64) if ps.has(k) else None for k in ("initial_std", "disturbance_std"))


def load_lqr_measurement(model):
    """(H [ny][nx], v [ny]) from the optional measurement_std vector of <model>/LQR.info: one entry per state, the square root of the
    measurement-noise intensity of a sensor that reads that state, 0 for a state that is not measured.  H selects the non-zero entries,
    v_m = std_m^2.  (None, None) when the file or the vector is absent, or no entry is non-zero."""
    path = os.path.join(model.getParameterFolder(), "LQR.info")
    if not os.path.exists(path):
        return None, None
    ps = ParameterServer(path)
    if not ps.has("measurement_std"):
        return None, None
    sd = np.array(ps.load_vector("measurement_std", model.state_dim), dtype=np.float64)
    idx = np.flatnonzero(sd)
    if idx.size == 0:
        return None, None
    H = np.zeros((idx.size, model.state_dim))
    H[np.arange(idx.size), idx] = 1.0
    return H, sd[idx] ** 2


FILTER_MIN_STEPS, FILTER_MAX_STEPS, FILTER_STEP_RATIO = 5, 200, 8.0


def filter_steps(sigma0, H, v, dt_max):
    """(steps, rho) of the filter sweep's step rule: rho = max_m (H sigma0 H')_mm / v_m, the rate of the filter's initial transient, over
    every sigma0 given; steps = the smallest count >= 5 with h rho <= 1/8, h = dt_max / steps (a count that the rule meets to 1e-12
    relative is taken as meeting it).  The count is returned whatever its size; LQRTracker.filter refuses above 200."""
    H = np.asarray(H, dtype=np.float64)
    S = np.asarray(sigma0, dtype=np.float64).reshape(-1, H.shape[1], H.shape[1])
    rho = float((np.einsum("mi,bij,mj->bm", H, S, H) / np.asarray(v, dtype=np.float64)[None, :]).max())
    need = FILTER_STEP_RATIO * rho * float(dt_max)
    return max(FILTER_MIN_STEPS, int(math.ceil(need * (1.0 - 1e-12))) if math.isfinite(need) else FILTER_MAX_STEPS + 1), rho


def si_flow_params(model):
    """the flow-map parameters in SI units (the tracker flies the dimensional plant)"""
    try:
        return np.asarray(model.flow_params(nondimensionalize=False), dtype=np.float64)
    except TypeError:  # Rocket2D has SI parameters only
        return np.asarray(model.flow_params(), dtype=np.float64)


def model_input_limits(model):
    """the limits row (T_min, T_max, angle_max in radians) of scpp_hip_lqr_set_input_limits from a model's parameters: T_min, T_max and
    gimbal_max (RocketQuat, Rocket2D) or pointing_max (Lander3dof), in SI units as the parameter files give them"""
    p = model.p
    angle = p.gimbal_max if hasattr(p, "gimbal_max") else p.pointing_max
    return np.array([p.T_min, p.T_max, angle], dtype=np.float64)


class LQRTracker:
    """Time-varying LQR along B trajectories: X [B][K][nx], U [B][K][nu] (first-order hold) or [B][K-1][nu] (zero-order hold), t [B], all in
    SI units.  The gains are computed at construction, like the reference's constructor.

    horizon="infinite" (the default, the reference's): one frozen-time gain per node, each from an algebraic Riccati equation of its own.
    horizon="finite": the differential Riccati equation swept backwards along each trajectory from P(T) = Qf (terminal_weights, the
    diagonal; None: LQR.info's terminal_weights if present, else Qf = Q), riccati_steps RKF78 steps per segment; keep_riccati=True also
    keeps P(t_k) (the `riccati` property, [B][K][nx][nx]).
    horizon="discrete": the gains of a loop that changes its correction only at the nodes and holds it over a segment (track(hold="node")
    flies it): the discrete Riccati recursion over the segments' transition matrices [Phi | Gamma], from P_{K-1} = Qf as above, with stage
    weights Q dt and R dt, discrete_steps RKF78 steps per segment; keep_discrete=True also keeps P, Phi and Gamma (discrete());
    covariance(hold="node") is the dispersion analysis of that loop.
    horizon="affine": the finite-horizon law for a nominal that does not obey the dynamics (a solver trajectory): the Riccati sweep on the state
    [e; 1], which also yields the feedforward terms k_k of du = -K e - k against the nominal's defect c = f(x_ref, u_ref) - dx_ref/dt, from
    P(T) = Qf as above, affine_steps RKF78 steps per segment; keep_affine=True also keeps P, p and s (affine()).  P and K are those of
    horizon="finite" at the same step count; track() then applies the term unless told otherwise."""

    def __init__(self, model, X, U, t, state_weights=None, input_weights=None, par=None, device=0, library=None, compute=True,
                 horizon="infinite", terminal_weights=None, riccati_steps=5, keep_riccati=False, discrete_steps=5, keep_discrete=False,
                 affine_steps=5, keep_affine=False):
        if horizon not in ("infinite", "finite", "discrete", "affine"):
            raise ValueError(f"horizon = {horizon!r}: 'infinite', 'finite', 'discrete' or 'affine'")
        self.horizon, self.riccati_steps, self.keep_riccati = horizon, int(riccati_steps), bool(keep_riccati)
        self.discrete_steps, self.keep_discrete = int(discrete_steps), bool(keep_discrete)
        self.affine_steps, self.keep_affine = int(affine_steps), bool(keep_affine)
        self.model = model
        nx, nu = model.state_dim, model.input_dim
        X = np.asarray(X, dtype=np.float64)
        self.X = np.ascontiguousarray(X.reshape(-1, X.shape[-2], nx))
        self.B, self.K = self.X.shape[0], self.X.shape[1]
        self.U = np.ascontiguousarray(np.asarray(U, dtype=np.float64).reshape(self.B, -1, nu))
        if self.U.shape[1] not in (self.K, self.K - 1):
            raise ValueError(f"U has {self.U.shape[1]} rows per trajectory; K = {self.K} needs K (first-order hold) or K - 1 (zero-order hold)")
        self.foh = self.U.shape[1] == self.K
        self.t = np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.float64).reshape(-1), (self.B,)))
        q, r = load_lqr_weights(model)
        self.Q = np.asarray(q if state_weights is None else state_weights, dtype=np.float64)
        self.R = np.asarray(r if input_weights is None else input_weights, dtype=np.float64)
        self.ctx = LqrContext(model.model_id, self.K, self.B, self.foh, device, library)
        self.ctx.set_weights(self.Q, self.R)
        self.Qf = None
        if horizon in ("finite", "discrete", "affine"):
            qf = load_lqr_terminal_weights(model) if terminal_weights is None else terminal_weights
            self.Qf = self.Q.copy() if qf is None else np.asarray(qf, dtype=np.float64)
            self.ctx.set_terminal_weights(self.Qf)
        self._riccati = self._discrete = self._affine = None
        self.ctx.set_flow_params(si_flow_params(model) if par is None else par)
        self.ctx.set_trajectories(self.X, self.U, self.t)
        self._gains = None
        self.n_ok = None
        if compute:
            self.computeGains()

    @classmethod
    def from_algorithm(cls, alg, **kw):
        """the tracker of every trajectory a solved SCAlgorithm / SCvxAlgorithm holds (SC_tracking.cpp:26-34)"""
        sol = alg.getSolution()
        U = sol["U"] if alg.opts.interpolate_input else sol["U"][:, :-1]
        return cls(alg.model, sol["X"], U, sol["sigma"], **kw)

    def computeGains(self):
        if self.horizon == "finite":
            return self.computeGainsRiccati()
        if self.horizon == "discrete":
            return self.computeGainsDiscrete()
        if self.horizon == "affine":
            return self.computeGainsAffine()
        self.n_ok = self.ctx.compute_gains()
        self._gains = self.ctx.download_gains()
        self._riccati = self._discrete = self._affine = None
        return self.n_ok

    def computeGainsRiccati(self, steps=None, keep=None):
        """finite-horizon gains of every trajectory (one Riccati sweep each, on the device); they replace the gains held so far"""
        steps = self.riccati_steps if steps is None else int(steps)
        keep = self.keep_riccati if keep is None else bool(keep)
        self.n_ok = self.ctx.compute_gains_riccati(steps, keep)
        self._gains = self.ctx.download_gains()
        self._riccati = self.ctx.download_riccati() if keep else None
        self._discrete = self._affine = None
        return self.n_ok

    def computeGainsDiscrete(self, steps=None, keep=None):
        """sampled-data gains of every trajectory (one discrete Riccati recursion each, on the device); they replace the gains held so far"""
        steps = self.discrete_steps if steps is None else int(steps)
        keep = self.keep_discrete if keep is None else bool(keep)
        self.n_ok = self.ctx.compute_gains_discrete(steps, keep)
        self._gains = self.ctx.download_gains()
        self._discrete = self.ctx.download_discrete() if keep else None
        self._riccati = self._affine = None
        return self.n_ok

    def computeGainsAffine(self, steps=None, keep=None):
        """affine finite-horizon gains and feedforward terms of every trajectory (one sweep of [[P, p], [p', s]] each, on the device); they
        replace the gains held so far"""
        steps = self.affine_steps if steps is None else int(steps)
        keep = self.keep_affine if keep is None else bool(keep)
        self.n_ok = self.ctx.compute_gains_affine(steps, keep)
        self._gains = self.ctx.download_gains()
        self._affine = self.ctx.download_affine(keep)
        self._riccati = self._discrete = None
        return self.n_ok

    def affine(self):
        """dict of ff [B][K][nu] (the feedforward terms k_k) of the last affine sweep and, when kept (keep_affine=True or
        computeGainsAffine(keep=True)), P [B][K][nx][nx], p [B][K][nx], s [B][K]"""
        if self._affine is None:
            raise RuntimeError("no affine sweep held: construct with horizon='affine'")
        return self._affine

    def discrete(self):
        """dict of P [B][K][nx][nx], Phi [B][K-1][nx][nx], Gamma [B][K-1][nx][nu] of the last discrete sweep; needs keep_discrete=True (or
        computeGainsDiscrete(keep=True))"""
        if self._discrete is None:
            raise RuntimeError("no discrete sweep kept: construct with horizon='discrete', keep_discrete=True")
        return self._discrete

    @property
    def riccati(self):
        """P(t_k) [B][K][nx][nx] of the last sweep; needs keep_riccati=True (or computeGainsRiccati(keep=True))"""
        if self._riccati is None:
            raise RuntimeError("no Riccati solution kept: construct with horizon='finite', keep_riccati=True")
        return self._riccati

    def setGains(self, G):
        """user-supplied gains [B][K][nu][nx] instead of the computed ones"""
        self.ctx.set_gains(G)
        self._riccati = self._discrete = self._affine = None
        self._gains = dict(gains=np.array(G, dtype=np.float64).reshape(self.B, self.K, self.model.input_dim, self.model.state_dim), status=None, iters=None)

    @property
    def gains(self):
        return self._gains["gains"]

    @property
    def status(self):
        return self._gains["status"]

    @property
    def iterations(self):
        return self._gains["iters"]

    def getInput(self, t, x, b=0, feedforward=None):
        """LQRTracker::getInput (LQRTracker.cpp:43-65) of trajectory b, on the host: for spot checks of what the device loop applies.
        feedforward as in track(): None includes the term k_t exactly when the gains held came from the affine sweep."""
        X, U, G, t_max = self.X[b], self.U[b], self.gains[b], float(self.t[b])
        tc = min(max(float(t), 0.0), t_max)
        dt = t_max / (self.K - 1)
        a = math.fmod(tc, dt) / dt
        i = min(int(tc / dt), self.K - 2)
        j = i + 1 if self.foh else i
        x_ref = X[i] + a * (X[i + 1] - X[i])
        u = -(G[i] + a * (G[j] - G[i])) @ (np.asarray(x, dtype=np.float64) - x_ref) + U[i] + a * (U[j] - U[i])
        if self._feedforward_on(feedforward):
            ff = self._affine["ff"][b]
            u = u - (ff[i] + a * (ff[j] - ff[i]))
        return u

    def _feedforward_on(self, feedforward):
        on = (self._affine is not None) if feedforward is None else bool(feedforward)
        if on and self._affine is None:
            raise RuntimeError("no feedforward terms held: compute the gains with horizon='affine' (computeGainsAffine)")
        return on

    def setInputLimits(self, lim=None):
        """Input limits inside the closed loop: None (the default) none, "model" the row of the model's parameters (model_input_limits), or
        an array (T_min, T_max, angle_max in radians), one row for all trajectories or [B][3].  The loop then applies u = sat(u_cmd)
        (include/scpp_hip_lqr.h has the rule).  A clip, not an anti-windup design: the gains and the covariance sweep do not know about it."""
        if isinstance(lim, str):
            if lim != "model":
                raise ValueError(f"lim = {lim!r}: None, 'model' or an array")
            lim = model_input_limits(self.model)
        self.ctx.set_input_limits(lim)

    def track(self, x_start, x_final=None, time_step=0.01, substeps=20, max_steps=None, n_record=0, write_steps=30, samples=1, hold="step",
              feedforward=None, disturbance=None, seed=0, flight_offset=0):
        """The loop of SC_tracking.cpp:48-75 on the device, `samples` flights per trajectory from x_start [B * samples][nx] (flight f follows
        trajectory f // samples; samples = 1: one flight per trajectory).  Returns x, u, t, steps, status, err0, err1 (|x - x_final| at
        start / end), max_dev (largest |x - x_ref|), n_sat (plant steps on which the input limits clipped), max_clip (largest
        |u_cmd - u|; both 0 without limits), n_finite and, with n_record > 0, `record` (of the first n_record flights).
        hold="step" (the default): the feedback term changes on every plant step; hold="node": du = -G[i] (x - x_ref) is latched at the
        first plant step of segment i and held over it (the loop horizon="discrete" designs for).
        feedforward: True applies u_cmd = u_ref - K_t (x - x_ref) - k_t with the terms of the affine sweep, False flies without them; None
        (the default) means on exactly when the gains held came from the affine sweep.  Together with hold="node" it is refused.
        disturbance: the diagonal of a process-noise intensity W ([nx], state^2 per second, what covariance() takes); None (the default)
        flies the undisturbed plant.  Plant step n of flight f then integrates dx/dt = f(x, u) + d with d_r = sqrt(w_r / time_step) z_r held
        over the step, z standard normals that are a pure function of (seed, flight_offset + f, n, r): the same seed gives the same flights,
        and a fan split over several calls with flight_offset = the flights flown so far is the fan of one call.  White, diagonal and held
        over a plant step; no measurement noise, no coloured noise, and the gains do not know about it."""
        if hold not in ("step", "node"):
            raise ValueError(f"hold = {hold!r}: 'step' or 'node'")
        self.ctx.set_disturbance(disturbance, seed, flight_offset)
        self.ctx.set_feedback_hold(1 if hold == "node" else 0)
        self.ctx.set_feedforward(1 if self._feedforward_on(feedforward) else 0)
        x_final = self.model.p.x_final if x_final is None else x_final
        x_final = np.array(list(x_final), dtype=np.float64)
        if max_steps is None:
            max_steps = int(math.ceil(float(np.nanmax(self.t)) / time_step)) + 2
        if samples == 1:
            n_finite = self.ctx.track(x_start, x_final, time_step, substeps, max_steps, n_record, write_steps)
        else:
            n_finite = self.ctx.track_samples(x_start, x_final, samples, time_step, substeps, max_steps, n_record, write_steps)
        out = self.ctx.track_download()
        out.update(self.ctx.track_download_saturation())
        out["n_finite"] = n_finite
        if n_record > 0:
            out["record"] = self.ctx.track_record()
        return out

    def covariance(self, sigma0, disturbance=None, steps=5, keep=False, hold="step"):
        """Linear covariance analysis of the closed loop under the gains held, one forward sweep per trajectory on the device.
        hold="step" (the default), the continuous loop: dS/dt = A_cl S + S A_cl' + W, S(0) = sigma0 ([nx][nx] for every trajectory or
        [B][nx][nx], symmetric), A_cl = A - B K_t, W = diag(disturbance) (None: 0), `steps` RKF78 steps per segment.
        hold="node", the loop track(hold="node") flies, du_i = -G[i] dx(t_i) held over segment i: S_{i+1} = Acl_i S_i Acl_i' + Wd_i with
        Acl_i = Phi_i - Gamma_i G[i] from the segment's transition matrices and Wd_i the disturbance the segment accumulates in open loop.
        Returns state_std [B][K][nx], input_cov [B][K][nu][nu] (G[k] S(t_k) G[k]'), final_cov [B][nx][nx], status [B], n_ok and, with
        keep=True, cov [B][K][nx][nx]."""
        if hold not in ("step", "node"):
            raise ValueError(f"hold = {hold!r}: 'step' or 'node'")
        self.ctx.set_covariance_inputs(sigma0, disturbance)
        n_ok = self.ctx.propagate_covariance_discrete(steps, keep) if hold == "node" else self.ctx.propagate_covariance(steps, keep)
        out = self.ctx.download_covariance(keep)
        out["n_ok"] = n_ok
        return out

    def moments(self, sigma0, disturbance=None, mean0=None, steps=5, keep=False, feedforward=None):
        """covariance() of the continuous loop together with where the loop's centre goes, in ONE sweep per trajectory on the device:
        dm/dt = A_cl m + d, m(0) = mean0 ([nx] for every trajectory or [B][nx]; None: 0), d = c - [B k_t], c = f(x_ref, u_ref) - dx_ref/dt the
        defect of the nominal.  feedforward as in track(): True includes the terms of the affine sweep, False leaves them out, None means on
        exactly when the gains held came from the affine sweep.  Returns covariance()'s dict (bitwise that of covariance() at the same steps)
        plus mean [B][K][nx] = m(t_k) and input_mean [B][K][nu] = -G[k] m(t_k) - [ff[k]], the mean correction on top of u_ref.  A
        linearisation about the nominal, of the continuous loop (hold="step") without input limits; the held loop's mean is not built."""
        self.ctx.set_covariance_inputs(sigma0, disturbance)
        n_ok = self.ctx.propagate_moments(steps, keep, self._feedforward_on(feedforward), mean0)
        out = self.ctx.download_covariance(keep)
        out.update(self.ctx.download_moments())
        out["n_ok"] = n_ok
        return out

    def filter(self, sigma0, disturbance=None, H=None, measurement_noise=None, steps=None, closed_loop=None, keep=False):
        """LQG analysis along every trajectory, one forward sweep per trajectory on the device: the Kalman-Bucy filter of the measurement
        y = H e + v (H [ny][nx], one for all trajectories; v white with intensity diag(measurement_noise)), and with closed_loop the
        output-feedback loop du = -K_t e^ under the gains held:
            dSg/dt = A Sg + Sg A' + W - Sg H' V^-1 H Sg,    Sg(0) = sigma0,   L = Sg H' V^-1      (error covariance of e - e^)
            dXh/dt = A_cl Xh + Xh A_cl' + Sg H' V^-1 H Sg,  Xh(0) = 0                             (covariance of the estimate)
        sigma0 and disturbance as in covariance().  H / measurement_noise None: those of LQR.info's measurement_std
        (load_lqr_measurement).  closed_loop None: exactly when the tracker has gains.  steps None: the smallest count >= 5 with
        h rho <= 1/8, rho = max_m (H sigma0 H')_mm / v_m, from the largest rho and dt of the batch (filter_steps); a count above 200 is
        refused, never changed.  Returns L [B][K][nx][ny], error_std [B][K][nx], final_error_cov, status [B], n_ok, steps, with
        closed_loop state_std (sqrt diag (Sg + Xh)), input_cov (G[k] Xh G[k]') and final_state_cov, and with keep=True error_cov and
        estimate_cov [B][K][nx][nx].  A linearisation about the nominal with continuous measurements and continuous feedback; the tracking
        kernel flies no estimator, so no flight corresponds to it."""
        if H is None or measurement_noise is None:
            Hf, vf = load_lqr_measurement(self.model)
            if Hf is None:
                raise ValueError("no measurement: pass H and measurement_noise, or give LQR.info a measurement_std vector")
            H, measurement_noise = (Hf if H is None else H), (vf if measurement_noise is None else measurement_noise)
        H = np.asarray(H, dtype=np.float64).reshape(-1, self.model.state_dim)
        v = np.asarray(measurement_noise, dtype=np.float64).reshape(-1)
        if closed_loop is None:
            closed_loop = self._gains is not None
        if steps is None:
            steps, rho = filter_steps(sigma0, H, v, float(self.t.max()) / (self.K - 1))
            if steps > FILTER_MAX_STEPS:
                raise ValueError(
                    f"filter: the initial transient has the rate rho = max (H sigma0 H')_mm / v_m = {rho:.6g} per second, which needs {steps} "
                    f"steps per segment for h rho <= 1/{FILTER_STEP_RATIO:g}; more than {FILTER_MAX_STEPS} is refused.  Pass steps explicitly, "
                    "or use a larger measurement_noise or a smaller sigma0.")
        self.ctx.set_covariance_inputs(sigma0, disturbance)
        self.ctx.set_measurement(H, v)
        n_ok = self.ctx.filter(steps, closed_loop, keep)
        out = self.ctx.download_filter(closed_loop, keep)
        out["n_ok"], out["steps"] = n_ok, int(steps)
        return out

    def close(self):
        self.ctx.close()


class LQRAlgorithm:
    """LQRAlgorithm.cpp:6-75 for B states at once: one constant gain, linearised at the model's operating point."""

    def __init__(self, model, batch_max=1, device=0, library=None):
        if not hasattr(model, "getOperatingPoint"):
            raise RuntimeError(f"{model.modelName} declares no operating point (the reference: Rocket2D only)")
        self.model, self.batch_max, self.device, self.library = model, batch_max, device, library
        self.initialized = False
        self.x_init = self.x_final = self.u = None
        self.input_limits = None
        self.loadParameters()

    def loadParameters(self):
        q, r = load_lqr_weights(self.model)
        self.setStateWeights(q)
        self.setInputWeights(r)

    def setStateWeights(self, w):
        self.Q = np.asarray(w, dtype=np.float64)

    def setInputWeights(self, w):
        self.R = np.asarray(w, dtype=np.float64)

    def setInputLimits(self, lim=None):
        """the clip of LQR_sim.cpp:55-66 for the loops LQRSim flies with this algorithm: None (the default) none, "model" the limits of the
        model's parameters, or a row (T_min, T_max, angle_max in radians); solve() stays the unlimited control law"""
        self.input_limits = lim

    def initialize(self):
        """LQRAlgorithm.cpp:11-25: the gain kernel on a two-node constant 'trajectory' at the operating point"""
        self.x_eq, self.u_eq = (np.asarray(v, dtype=np.float64) for v in self.model.getOperatingPoint())
        X = np.tile(self.x_eq, (1, 2, 1))
        U = np.tile(self.u_eq, (1, 2, 1))
        trk = LQRTracker(self.model, X, U, [1.0], self.Q, self.R, device=self.device, library=self.library)
        self.status, self.iterations = int(trk.status[0, 0]), int(trk.iterations[0, 0])
        self.K = trk.gains[0, 0].copy()
        trk.close()
        if self.status != 0:
            raise RuntimeError(f"LQR gain at the operating point failed with status {self.status}")
        self.initialized = True
        return self

    def setInitialState(self, x):
        self.x_init = np.asarray(x, dtype=np.float64).reshape(-1, self.model.state_dim)

    def setFinalState(self, x):
        self.x_final = np.asarray(x, dtype=np.float64).reshape(self.model.state_dim)

    def solve(self):
        """LQRAlgorithm.cpp:27-33"""
        assert self.initialized
        self.u = -(self.x_init - self.x_final) @ self.K.T + self.u_eq

    def getSolution(self):
        assert self.u is not None
        return self.u


class LQRSim:
    """LQR_sim.cpp:20-82 for B closed loops on the device: u = -K (x - x_final) + u_eq until |x - x_final| < stop_tol or sim_time."""

    def __init__(self, algorithm, sim_time=5.0, time_step=0.010, stop_tol=0.02):
        self.alg, self.sim_time, self.time_step, self.stop_tol = algorithm, sim_time, time_step, stop_tol
        self.input_limits = algorithm.input_limits

    def setInputLimits(self, lim=None):
        """as LQRTracker.setInputLimits, for the loops of run(); starts as the algorithm's setting"""
        self.input_limits = lim

    def run(self, x_start, x_final=None, n_record=0, write_steps=30, substeps=20, disturbance=None, seed=0, flight_offset=0):
        """disturbance, seed, flight_offset: process noise on the plant, as LQRTracker.track takes it"""
        a = self.alg
        assert a.initialized
        x_start = np.asarray(x_start, dtype=np.float64).reshape(-1, a.model.state_dim)
        B = x_start.shape[0]
        x_final = np.asarray(a.model.p.x_final if x_final is None else x_final, dtype=np.float64)
        trk = LQRTracker(a.model, np.tile(x_final, (B, 2, 1)), np.tile(a.u_eq, (B, 2, 1)), np.full(B, self.sim_time), a.Q, a.R,
                         device=a.device, library=a.library, compute=False)
        trk.setGains(np.tile(a.K, (B, 2, 1, 1)))
        trk.ctx.set_stop_tolerance(self.stop_tol)
        trk.setInputLimits(self.input_limits)
        out = trk.track(x_start, x_final, self.time_step, substeps, None, n_record, write_steps, disturbance=disturbance, seed=seed,
                        flight_offset=flight_offset)
        trk.close()
        return out

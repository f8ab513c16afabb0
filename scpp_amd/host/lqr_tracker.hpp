// C++17 host front end of the LQR tracker over include/scpp_hip_lqr.h: the reference's LQRTracker
//   LQRTracker(model, td), getInput(t, x, u), interpolateGains(t)       scpp_core/include/LQRTracker.hpp, src/LQRTracker.cpp:6-65
// for a batch of trajectories, plus the closed loop of scpp/src/SC_tracking.cpp:48-75 on the device (track).  The gains and the
// flights are computed by libscpp_lqr.so; there is no CPU fallback.
#pragma once
#include <algorithm>
#include <cmath>
#include <filesystem>
#include <utility>

#include "sc_algorithm.hpp"
#include "scpp_hip_lqr.h"

namespace scpp
{

struct lqr_track_result_t
{
    std::vector<Model::state_vector_t> x; // final states
    std::vector<Model::input_vector_t> u; // last inputs
    std::vector<double> t, initial_error, final_error, max_deviation;
    std::vector<int32_t> steps, status;
    std::vector<int32_t> n_sat;   // plant steps on which the input limits clipped (0 without limits)
    std::vector<double> max_clip; // largest |u_cmd - u| met (0 without limits)
    int n_finite = 0;
    // record of the first n_record flights, every write_steps-th step
    std::vector<std::vector<Model::state_vector_t>> X_sim;
    std::vector<std::vector<Model::input_vector_t>> U_sim;
    std::vector<std::vector<double>> t_sim;
};

// which gain law the tracker computes.  finite_horizon = false (the default, the reference's): one frozen-time gain per node.  true: the
// differential Riccati equation swept backwards along each trajectory from P(T) = Qf (scpp_hip_lqr_compute_gains_riccati), riccati_steps
// RKF78 steps per segment; terminal_weights: the diagonal of Qf, empty: LQR.info's terminal_weights if present, else Qf = Q;
// keep_riccati: P(t_k) is downloaded into LQRTracker::riccati.
// discrete = true (finite_horizon must then be false): the sampled-data gains of a loop that changes its correction only at the nodes
// (scpp_hip_lqr_compute_gains_discrete; LQRTracker::setFeedbackHold flies such a loop): the discrete Riccati recursion over the segments'
// transition matrices from P_{K-1} = Qf (terminal_weights as above), discrete_steps RKF78 steps per segment; keep_discrete: P, Phi and Gamma are
// downloaded into LQRTracker::discrete_P, discrete_Phi, discrete_Gamma.
// affine = true (the other two must then be false): the finite-horizon law for a nominal that does not obey the dynamics
// (scpp_hip_lqr_compute_gains_affine): the Riccati sweep on the state [e; 1], which also yields the feedforward terms k_k of du = -K e - k, from
// P(T) = Qf (terminal_weights as above), affine_steps RKF78 steps per segment; the terms are downloaded into LQRTracker::feedforward and
// track() applies them (LQRTracker::setFeedforward(false) flies without); keep_affine: P, p and s are downloaded into affine_P, affine_p, affine_s.
struct lqr_gain_options_t
{
    bool finite_horizon = false;
    int riccati_steps = 5;
    bool keep_riccati = false;
    std::vector<double> terminal_weights;
    bool discrete = false;
    int discrete_steps = 5;
    bool keep_discrete = false;
    bool affine = false;
    int affine_steps = 5;
    bool keep_affine = false;
};

// the closed-loop covariance sweep (scpp_hip_lqr_propagate_covariance): dS/dt = A_cl S + S A_cl' + W, S(0) = sigma0, under the gains the tracker
// holds.  sigma0: one symmetric [NX][NX] matrix for every trajectory or [B][NX][NX], row-major; disturbance: the diagonal of W, empty: W = 0;
// steps: RKF78 steps per segment; keep: S(t_k) of every node is downloaded into lqr_covariance_result_t::cov.
// hold_node: the sweep of the loop that holds its correction over a segment instead (scpp_hip_lqr_propagate_covariance_discrete; the loop
// setFeedbackHold(true) flies): S_{i+1} = Acl_i S_i Acl_i' + Wd_i, Acl_i = Phi_i - Gamma_i G[i].
struct lqr_covariance_options_t
{
    std::vector<double> sigma0;
    std::vector<double> disturbance;
    int steps = 5;
    bool keep = false;
    bool hold_node = false;
};

struct lqr_covariance_result_t
{
    std::vector<double> state_std; // [B][K][NX]  sqrt of the diagonal of S(t_k)
    std::vector<double> input_cov; // [B][K][NU][NU]  G[k] S(t_k) G[k]'
    std::vector<double> final_cov; // [B][NX][NX]
    std::vector<double> cov;       // [B][K][NX][NX], keep only
    std::vector<int32_t> status;   // [B]: SCPP_LQR_OK, SCPP_LQR_GAINS_INCOMPLETE, SCPP_LQR_NONFINITE
    int n_ok = 0;
};

// the covariance sweep of the continuous loop together with the loop's mean (scpp_hip_lqr_propagate_moments): dm/dt = A_cl m + d, m(0) = mean0,
// d = c - [B k_t], c the defect of the nominal.  A linearisation about the nominal, of the continuous loop, without input limits.
struct lqr_moments_result_t : lqr_covariance_result_t
{
    std::vector<double> mean;       // [B][K][NX]  m(t_k)
    std::vector<double> input_mean; // [B][K][NU]  -G[k] m(t_k) - [ff[k]]: the mean correction on top of u_ref
};

// the filter sweep (scpp_hip_lqr_filter): the Kalman-Bucy error covariance Sg of the measurement y = H e + v along every trajectory and, with
// the loop closed on the estimate (du = -K_t e^), the covariance Xh of the estimate; the state covariance of that loop is Sg + Xh.
// sigma0, disturbance, keep: as lqr_covariance_options_t.  H: [ny][NX] row-major, one for all trajectories; measurement_noise: the diagonal
// of V, ny entries > 0; whichever is empty: that of LQR.info's measurement_std (LQRTracker::loadMeasurement).  closed_loop < 0 (the default): exactly
// when the tracker holds gains; 0 / 1: the filter alone / with the loop's covariance.  steps <= 0 (the default): the smallest count >= 5 with
// h rho <= 1/8, rho = max_m (H sigma0 H')_mm / v_m, from the largest rho and dt of the batch (LQRTracker::filterSteps); above 200 the call is
// refused (std::invalid_argument names rho, the count and the way out) and never changes the count.  A linearisation about the nominal with
// continuous measurements and continuous feedback; no flight corresponds to it.
struct lqr_filter_options_t
{
    std::vector<double> sigma0;
    std::vector<double> disturbance;
    std::vector<double> H;
    std::vector<double> measurement_noise;
    int steps = 0;
    int closed_loop = -1;
    bool keep = false;
};

struct lqr_filter_result_t
{
    std::vector<double> L;               // [B][K][NX][ny]  Sg(t_k) H' V^-1
    std::vector<double> error_std;       // [B][K][NX]  sqrt of the diagonal of Sg(t_k)
    std::vector<double> final_error_cov; // [B][NX][NX]
    std::vector<double> error_cov;       // [B][K][NX][NX], keep only
    std::vector<double> state_std;       // [B][K][NX]  sqrt of the diagonal of (Sg + Xh)(t_k); closed loop only, as the next three
    std::vector<double> input_cov;       // [B][K][NU][NU]  G[k] Xh(t_k) G[k]'
    std::vector<double> final_state_cov; // [B][NX][NX]
    std::vector<double> estimate_cov;    // [B][K][NX][NX], keep only
    std::vector<int32_t> status;         // [B]: SCPP_LQR_OK, SCPP_LQR_GAINS_INCOMPLETE, SCPP_LQR_NONFINITE
    int n_ok = 0, ny = 0, steps = 0;
    bool closed_loop = false;
};

class LQRTracker
{
public:
    static constexpr size_t NX = Model::state_dim, NU = Model::input_dim;
    using feedback_matrix_t = std::array<std::array<double, NX>, NU>;

    // LQRTracker.cpp:6-28 for every trajectory of `tds` (all with the same K and hold): the gains are computed here
    // `weights`: (state_weights [NX], input_weights [NU]) instead of those of LQR.info
    LQRTracker(Model::ptr_t model_, const std::vector<trajectory_data_t> &tds_, int device = 0,
               const std::pair<std::array<double, NX>, std::array<double, NU>> *weights = nullptr, const lqr_gain_options_t &options = {})
        : opts(options), model(std::move(model_)), tds(tds_)
    {
        if (tds.empty() || tds[0].n_X() < 2)
            throw std::invalid_argument("LQRTracker: at least one trajectory of at least two nodes");
        const int B = int(tds.size()), K = int(tds[0].n_X());
        const bool foh = tds[0].interpolatedInput();
        const size_t nU = tds[0].n_U();
        if (weights)
        {
            Q = weights->first;
            R = weights->second;
        }
        else
            loadParameters();
        check(scpp_hip_lqr_create(&ctx, device, Model::model_id, K, B, foh ? 1 : 0), "scpp_hip_lqr_create");
        check(scpp_hip_lqr_set_weights(ctx, Q.data(), R.data()), "scpp_hip_lqr_set_weights");
        std::vector<double> par(Model::param_dim);
        model->flowParams(par.data());
        check(scpp_hip_lqr_set_flow_params(ctx, par.data(), 1), "scpp_hip_lqr_set_flow_params");
        std::vector<double> X(size_t(B) * K * NX), U(size_t(B) * nU * NU), t(static_cast<size_t>(B), 0.);
        for (int b = 0; b < B; b++)
        {
            const trajectory_data_t &td = tds[size_t(b)];
            if (int(td.n_X()) != K || td.n_U() != nU)
                throw std::invalid_argument("LQRTracker: trajectories of different shapes");
            for (size_t k = 0; k < size_t(K); k++)
                std::copy(td.X[k].begin(), td.X[k].end(), &X[(size_t(b) * K + k) * NX]);
            for (size_t k = 0; k < nU; k++)
                std::copy(td.U[k].begin(), td.U[k].end(), &U[(size_t(b) * nU + k) * NU]);
            t[size_t(b)] = td.t;
        }
        check(scpp_hip_lqr_set_trajectories(ctx, X.data(), U.data(), t.data(), B), "scpp_hip_lqr_set_trajectories");
        if (int(opts.finite_horizon) + int(opts.discrete) + int(opts.affine) > 1)
            throw std::invalid_argument("LQRTracker: finite_horizon, discrete and affine are three gain laws, choose one");
        if (opts.affine)
        {
            std::vector<double> qf = opts.terminal_weights.empty() ? loadTerminalWeights() : opts.terminal_weights;
            if (!qf.empty() && qf.size() != NX)
                throw std::invalid_argument("LQRTracker: terminal_weights needs one entry per state");
            check(scpp_hip_lqr_set_terminal_weights(ctx, qf.empty() ? nullptr : qf.data()), "scpp_hip_lqr_set_terminal_weights");
            check(scpp_hip_lqr_compute_gains_affine(ctx, opts.affine_steps, opts.keep_affine ? 1 : 0, &n_ok), "scpp_hip_lqr_compute_gains_affine");
            feedforward.resize(size_t(B) * K * NU);
            if (opts.keep_affine)
            {
                affine_P.resize(size_t(B) * K * NX * NX);
                affine_p.resize(size_t(B) * K * NX);
                affine_s.resize(size_t(B) * K);
            }
            check(scpp_hip_lqr_download_affine(ctx, feedforward.data(), opts.keep_affine ? affine_P.data() : nullptr,
                                               opts.keep_affine ? affine_p.data() : nullptr, opts.keep_affine ? affine_s.data() : nullptr),
                  "scpp_hip_lqr_download_affine");
            setFeedforward(true);
        }
        else if (opts.discrete)
        {
            std::vector<double> qf = opts.terminal_weights.empty() ? loadTerminalWeights() : opts.terminal_weights;
            if (!qf.empty() && qf.size() != NX)
                throw std::invalid_argument("LQRTracker: terminal_weights needs one entry per state");
            check(scpp_hip_lqr_set_terminal_weights(ctx, qf.empty() ? nullptr : qf.data()), "scpp_hip_lqr_set_terminal_weights");
            check(scpp_hip_lqr_compute_gains_discrete(ctx, opts.discrete_steps, opts.keep_discrete ? 1 : 0, &n_ok), "scpp_hip_lqr_compute_gains_discrete");
            if (opts.keep_discrete)
            {
                discrete_P.resize(size_t(B) * K * NX * NX);
                discrete_Phi.resize(size_t(B) * (K - 1) * NX * NX);
                discrete_Gamma.resize(size_t(B) * (K - 1) * NX * NU);
                check(scpp_hip_lqr_download_discrete(ctx, discrete_P.data(), discrete_Phi.data(), discrete_Gamma.data()), "scpp_hip_lqr_download_discrete");
            }
        }
        else if (opts.finite_horizon)
        {
            std::vector<double> qf = opts.terminal_weights.empty() ? loadTerminalWeights() : opts.terminal_weights;
            if (!qf.empty() && qf.size() != NX)
                throw std::invalid_argument("LQRTracker: terminal_weights needs one entry per state");
            check(scpp_hip_lqr_set_terminal_weights(ctx, qf.empty() ? nullptr : qf.data()), "scpp_hip_lqr_set_terminal_weights");
            check(scpp_hip_lqr_compute_gains_riccati(ctx, opts.riccati_steps, opts.keep_riccati ? 1 : 0, &n_ok), "scpp_hip_lqr_compute_gains_riccati");
            if (opts.keep_riccati)
            {
                riccati.resize(size_t(B) * K * NX * NX);
                check(scpp_hip_lqr_download_riccati(ctx, riccati.data()), "scpp_hip_lqr_download_riccati");
            }
        }
        else
            check(scpp_hip_lqr_compute_gains(ctx, &n_ok), "scpp_hip_lqr_compute_gains");
        gains.resize(size_t(B) * K);
        status.resize(size_t(B) * K);
        iterations.resize(size_t(B) * K);
        check(scpp_hip_lqr_download_gains(ctx, &gains[0][0][0], status.data(), iterations.data()), "scpp_hip_lqr_download_gains");
    }
    LQRTracker(Model::ptr_t model_, const trajectory_data_t &td, int device = 0,
               const std::pair<std::array<double, NX>, std::array<double, NU>> *weights = nullptr, const lqr_gain_options_t &options = {})
        : LQRTracker(std::move(model_), std::vector<trajectory_data_t>{td}, device, weights, options)
    {
    }
    ~LQRTracker()
    {
        if (ctx)
            scpp_hip_lqr_destroy(ctx);
    }
    LQRTracker(const LQRTracker &) = delete;
    LQRTracker &operator=(const LQRTracker &) = delete;

    // LQRTracker.cpp:30-41; Q = I, R = I without an LQR.info
    void loadParameters()
    {
        Q.fill(1.);
        R.fill(1.);
        const std::string file = Model::getParameterFolder() + "/LQR.info";
        if (!std::filesystem::exists(file))
            return;
        ParameterServer param(file);
        param.loadMatrix("state_weights", Q.data(), int(NX));
        param.loadMatrix("input_weights", R.data(), int(NU));
    }

    // the optional terminal_weights vector of LQR.info; empty without the file or the entry (Qf = Q)
    static std::vector<double> loadTerminalWeights()
    {
        const std::string file = Model::getParameterFolder() + "/LQR.info";
        if (!std::filesystem::exists(file))
            return {};
        ParameterServer param(file);
        if (!param.has("terminal_weights"))
            return {};
        std::vector<double> qf(NX);
        param.loadMatrix("terminal_weights", qf.data(), int(NX));
        return qf;
    }

    const feedback_matrix_t &gain(size_t b, size_t k) const { return gains[b * tds[0].n_X() + k]; }
    int nodesConverged() const { return n_ok; }

    // LQRTracker.cpp:53-65 (host, for spot checks), trajectory b
    feedback_matrix_t interpolateGains(double t, size_t b = 0) const
    {
        const trajectory_data_t &td = tds[b];
        t = std::clamp(t, 0., td.t);
        const double dt = td.t / double(td.n_X() - 1);
        const double a = std::fmod(t, dt) / dt;
        const size_t i = std::min(size_t(t / dt), td.n_X() - 2);
        const feedback_matrix_t &K0 = gain(b, i), &K1 = td.interpolatedInput() ? gain(b, i + 1) : K0;
        feedback_matrix_t K;
        for (size_t r = 0; r < NU; r++)
            for (size_t c = 0; c < NX; c++)
                K[r][c] = K0[r][c] + a * (K1[r][c] - K0[r][c]);
        return K;
    }
    // LQRTracker.cpp:43-51 with trajectoryData.hpp:41-78 (host, for spot checks), trajectory b
    void getInput(double t, const Model::state_vector_t &x, Model::input_vector_t &u, size_t b = 0) const
    {
        const trajectory_data_t &td = tds[b];
        t = std::clamp(t, 0., td.t);
        const double dt = td.t / double(td.n_X() - 1);
        const double a = std::fmod(t, dt) / dt;
        const size_t i = std::min(size_t(t / dt), td.n_X() - 2), j = td.interpolatedInput() ? i + 1 : i;
        const feedback_matrix_t K = interpolateGains(t, b);
        for (size_t r = 0; r < NU; r++)
        {
            double acc = 0.;
            for (size_t c = 0; c < NX; c++)
                acc += K[r][c] * (x[c] - (td.X[i][c] + a * (td.X[i + 1][c] - td.X[i][c])));
            u[r] = -acc + (td.U[i][r] + a * (td.U[j][r] - td.U[i][r]));
            if (feedforward_on)
            {
                const double f0 = feedforward[(b * td.n_X() + i) * NU + r], f1 = feedforward[(b * td.n_X() + j) * NU + r];
                u[r] -= f0 + a * (f1 - f0);
            }
        }
    }

    // input limits inside the closed loop (scpp_hip_lqr_set_input_limits): rows (T_min, T_max, angle_max in radians), one for every trajectory
    // or one per trajectory; empty: none (the default).  A clip, not an anti-windup design: the gains do not know about it.
    void setInputLimits(const std::vector<double> &lim)
    {
        if (lim.size() % 3 != 0)
            throw std::invalid_argument("LQRTracker::setInputLimits: rows of (T_min, T_max, angle_max)");
        check(scpp_hip_lqr_set_input_limits(ctx, lim.empty() ? nullptr : lim.data(), int(lim.size() / 3)), "scpp_hip_lqr_set_input_limits");
    }
    // the limits of the model's parameters: T_min, T_max, gimbal_max
    void setInputLimitsFromModel()
    {
        std::vector<double> lim(3);
        model->inputLimits(lim.data());
        setInputLimits(lim);
    }
    // when the loop updates its feedback term (scpp_hip_lqr_set_feedback_hold): false (the default) on every plant step, true: latched at each
    // node and held over the segment, the loop the discrete gain law designs for.  Stays until it is set again.
    void setFeedbackHold(bool node) { check(scpp_hip_lqr_set_feedback_hold(ctx, node ? 1 : 0), "scpp_hip_lqr_set_feedback_hold"); }
    // whether the loop applies the feedforward term of the affine law (scpp_hip_lqr_set_feedforward): u_cmd = u_ref - K_t (x - x_ref) - k_t.  On
    // after an affine sweep, off otherwise; needs the terms of such a sweep, and is refused together with setFeedbackHold(true) by track().
    void setFeedforward(bool on)
    {
        if (on && feedforward.empty())
            throw std::invalid_argument("LQRTracker::setFeedforward: no feedforward terms held (lqr_gain_options_t::affine)");
        check(scpp_hip_lqr_set_feedforward(ctx, on ? 1 : 0), "scpp_hip_lqr_set_feedforward");
        feedforward_on = on;
    }
    bool feedforwardOn() const { return feedforward_on; }
    // process noise on the plant (scpp_hip_lqr_set_disturbance): w, the diagonal of the disturbance intensity, one entry per state (state^2 per
    // second); empty: none (the default).  Flight f draws as the global flight flight_offset + f of `seed`: the same seed flies the same
    // flights.  White, diagonal, held over a plant step; the gains do not know about it.  Stays until it is set again.
    void setDisturbance(const std::vector<double> &w, unsigned long long seed = 0, unsigned long long flight_offset = 0)
    {
        if (!w.empty() && w.size() != size_t(Model::state_dim))
            throw std::invalid_argument("LQRTracker::setDisturbance: one intensity per state");
        check(scpp_hip_lqr_set_disturbance(ctx, w.empty() ? nullptr : w.data(), seed, flight_offset), "scpp_hip_lqr_set_disturbance");
    }
    // regulator mode (scpp_hip_lqr_set_stop_tolerance) and user-supplied gains [B][K], for LQRAlgorithm::simulate
    void setStopTolerance(double tol) { check(scpp_hip_lqr_set_stop_tolerance(ctx, tol), "scpp_hip_lqr_set_stop_tolerance"); }
    void setGains(const std::vector<feedback_matrix_t> &G)
    {
        if (G.size() != gains.size())
            throw std::invalid_argument("LQRTracker::setGains: one gain per trajectory and node");
        check(scpp_hip_lqr_set_gains(ctx, &G[0][0][0]), "scpp_hip_lqr_set_gains");
        gains = G;
        if (feedforward_on)
            setFeedforward(false); // the terms went with the gains they belonged to
        feedforward.clear();
    }

    // SC_tracking.cpp:48-75 for every trajectory at once, on the device: `samples` flights per trajectory, flight f from x_start[f] along
    // trajectory f / samples (samples = 1: one flight per trajectory); max_steps = 0: the longest flight time / time_step + 2
    void track(const std::vector<Model::state_vector_t> &x_start, const Model::state_vector_t &x_final, lqr_track_result_t &out,
               double time_step = 0.01, int n_record = 0, int write_steps = 30, int substeps = 20, int samples = 1, int max_steps = 0)
    {
        if (samples < 1 || x_start.size() % size_t(samples) != 0)
            throw std::invalid_argument("LQRTracker::track: the starts are no multiple of samples");
        const int B = int(x_start.size());
        double t_max = 0.;
        for (const auto &td : tds)
            t_max = std::max(t_max, td.t);
        if (max_steps < 1)
            max_steps = int(std::ceil(t_max / time_step)) + 2;
        check(scpp_hip_lqr_track_samples(ctx, &x_start[0][0], x_final.data(), B / samples, samples, time_step, substeps, max_steps, n_record, write_steps,
                                         &out.n_finite),
              "scpp_hip_lqr_track_samples");
        const size_t nB = size_t(B);
        out.x.resize(nB);
        out.u.resize(nB);
        for (auto *v : {&out.t, &out.initial_error, &out.final_error, &out.max_deviation})
            v->assign(nB, 0.);
        out.steps.assign(nB, 0);
        out.status.assign(nB, 0);
        check(scpp_hip_lqr_track_download(ctx, &out.x[0][0], &out.u[0][0], out.t.data(), out.steps.data(), out.status.data(),
                                          out.initial_error.data(), out.final_error.data(), out.max_deviation.data()),
              "scpp_hip_lqr_track_download");
        out.n_sat.assign(nB, 0);
        out.max_clip.assign(nB, 0.);
        check(scpp_hip_lqr_track_download_saturation(ctx, out.n_sat.data(), out.max_clip.data()), "scpp_hip_lqr_track_download_saturation");
        out.X_sim.clear();
        out.U_sim.clear();
        out.t_sim.clear();
        if (n_record < 1)
            return;
        int nr = 0, cap = 0;
        check(scpp_hip_lqr_track_record_size(ctx, &nr, &cap), "scpp_hip_lqr_track_record_size");
        std::vector<double> X(size_t(nr) * cap * NX), U(size_t(nr) * cap * NU), t(size_t(nr) * cap);
        std::vector<int32_t> n(size_t(nr), 0);
        check(scpp_hip_lqr_track_record(ctx, X.data(), U.data(), t.data(), n.data()), "scpp_hip_lqr_track_record");
        out.X_sim.resize(size_t(nr));
        out.U_sim.resize(size_t(nr));
        out.t_sim.resize(size_t(nr));
        for (size_t b = 0; b < size_t(nr); b++)
            for (size_t j = 0; j < size_t(n[b]); j++)
            {
                Model::state_vector_t xs;
                Model::input_vector_t us;
                std::copy(&X[(b * cap + j) * NX], &X[(b * cap + j) * NX] + NX, xs.begin());
                std::copy(&U[(b * cap + j) * NU], &U[(b * cap + j) * NU] + NU, us.begin());
                out.X_sim[b].push_back(xs);
                out.U_sim[b].push_back(us);
                out.t_sim[b].push_back(t[b * cap + j]);
            }
    }

    // linear covariance analysis of every trajectory at once, on the device, under the gains held; changes neither gains nor flights
    void covariance(const lqr_covariance_options_t &o, lqr_covariance_result_t &out)
    {
        const size_t B = tds.size(), K = tds[0].n_X();
        if (o.sigma0.size() != NX * NX && o.sigma0.size() != B * NX * NX)
            throw std::invalid_argument("LQRTracker::covariance: sigma0 is one NX x NX matrix, or one per trajectory");
        if (!o.disturbance.empty() && o.disturbance.size() != NX)
            throw std::invalid_argument("LQRTracker::covariance: disturbance needs one entry per state");
        check(scpp_hip_lqr_set_covariance_inputs(ctx, o.sigma0.data(), int(o.sigma0.size() / (NX * NX)),
                                                 o.disturbance.empty() ? nullptr : o.disturbance.data()),
              "scpp_hip_lqr_set_covariance_inputs");
        if (o.hold_node)
            check(scpp_hip_lqr_propagate_covariance_discrete(ctx, o.steps, o.keep ? 1 : 0, &out.n_ok), "scpp_hip_lqr_propagate_covariance_discrete");
        else
            check(scpp_hip_lqr_propagate_covariance(ctx, o.steps, o.keep ? 1 : 0, &out.n_ok), "scpp_hip_lqr_propagate_covariance");
        out.state_std.assign(B * K * NX, 0.);
        out.input_cov.assign(B * K * NU * NU, 0.);
        out.final_cov.assign(B * NX * NX, 0.);
        out.status.assign(B, 0);
        out.cov.assign(o.keep ? B * K * NX * NX : 0, 0.);
        check(scpp_hip_lqr_download_covariance(ctx, out.state_std.data(), out.input_cov.data(), out.final_cov.data(), out.status.data(),
                                               o.keep ? out.cov.data() : nullptr),
              "scpp_hip_lqr_download_covariance");
    }

    // covariance() of the continuous loop (o.hold_node is refused: the held loop's mean is not built) together with the mean deviation, in one
    // sweep per trajectory.  mean0: empty (0), one [NX] row for every trajectory or [B][NX].  feedforward < 0 (the default): the drive of the
    // mean includes -B k_t exactly when the tracker holds the terms of an affine sweep; 0 / 1: without / with them.
    void moments(const lqr_covariance_options_t &o, const std::vector<double> &mean0, lqr_moments_result_t &out, int feedforward = -1)
    {
        const size_t B = tds.size(), K = tds[0].n_X();
        if (o.hold_node)
            throw std::invalid_argument("LQRTracker::moments: the mean of the loop that holds its correction is not built");
        if (o.sigma0.size() != NX * NX && o.sigma0.size() != B * NX * NX)
            throw std::invalid_argument("LQRTracker::moments: sigma0 is one NX x NX matrix, or one per trajectory");
        if (!o.disturbance.empty() && o.disturbance.size() != NX)
            throw std::invalid_argument("LQRTracker::moments: disturbance needs one entry per state");
        if (!mean0.empty() && mean0.size() != NX && mean0.size() != B * NX)
            throw std::invalid_argument("LQRTracker::moments: mean0 is one row of NX entries, or one per trajectory");
        const bool ff = feedforward < 0 ? !this->feedforward.empty() : feedforward != 0;
        if (ff && this->feedforward.empty())
            throw std::invalid_argument("LQRTracker::moments: no feedforward terms held (lqr_gain_options_t::affine)");
        check(scpp_hip_lqr_set_covariance_inputs(ctx, o.sigma0.data(), int(o.sigma0.size() / (NX * NX)),
                                                 o.disturbance.empty() ? nullptr : o.disturbance.data()),
              "scpp_hip_lqr_set_covariance_inputs");
        check(scpp_hip_lqr_propagate_moments(ctx, o.steps, o.keep ? 1 : 0, ff ? 1 : 0, mean0.empty() ? nullptr : mean0.data(),
                                             mean0.empty() ? 1 : int(mean0.size() / NX), &out.n_ok),
              "scpp_hip_lqr_propagate_moments");
        out.state_std.assign(B * K * NX, 0.);
        out.input_cov.assign(B * K * NU * NU, 0.);
        out.final_cov.assign(B * NX * NX, 0.);
        out.status.assign(B, 0);
        out.cov.assign(o.keep ? B * K * NX * NX : 0, 0.);
        out.mean.assign(B * K * NX, 0.);
        out.input_mean.assign(B * K * NU, 0.);
        check(scpp_hip_lqr_download_covariance(ctx, out.state_std.data(), out.input_cov.data(), out.final_cov.data(), out.status.data(),
                                               o.keep ? out.cov.data() : nullptr),
              "scpp_hip_lqr_download_covariance");
        check(scpp_hip_lqr_download_moments(ctx, out.mean.data(), out.input_mean.data()), "scpp_hip_lqr_download_moments");
    }

    static constexpr int FILTER_MIN_STEPS = 5, FILTER_MAX_STEPS = 200;

    // the filter sweep's step rule: the smallest count >= 5 with h rho <= 1/8, h = dt_max / steps (a count that the rule meets to 1e-12
    // relative is taken as meeting it); *rho_out = max_m (H sigma0 H')_mm / v_m over every sigma0 given.  Returned whatever its size.
    static int filterSteps(const std::vector<double> &sigma0, const std::vector<double> &H, const std::vector<double> &v, double dt_max,
                           double *rho_out = nullptr)
    {
        const size_t ny = v.size();
        double rho = 0.;
        for (size_t b = 0; b < sigma0.size() / (NX * NX); b++)
            for (size_t m = 0; m < ny; m++)
            {
                double hsh = 0.;
                for (size_t i = 0; i < NX; i++)
                    for (size_t j = 0; j < NX; j++)
                        hsh += H[m * NX + i] * sigma0[(b * NX + i) * NX + j] * H[m * NX + j];
                rho = std::max(rho, hsh / v[m]);
            }
        if (rho_out)
            *rho_out = rho;
        const double need = std::ceil(8. * rho * dt_max * (1. - 1e-12));
        if (!std::isfinite(need))
            return FILTER_MAX_STEPS + 1;
        return std::max(FILTER_MIN_STEPS, int(std::min(need, 2147483647.))); // the count it would take, whatever its size
    }

    // LQG analysis of every trajectory at once, on the device; changes neither gains, covariance results nor flights
    void filter(const lqr_filter_options_t &o, lqr_filter_result_t &out)
    {
        const size_t B = tds.size(), K = tds[0].n_X();
        if (o.sigma0.size() != NX * NX && o.sigma0.size() != B * NX * NX)
            throw std::invalid_argument("LQRTracker::filter: sigma0 is one NX x NX matrix, or one per trajectory");
        if (!o.disturbance.empty() && o.disturbance.size() != NX)
            throw std::invalid_argument("LQRTracker::filter: disturbance needs one entry per state");
        std::vector<double> H = o.H, v = o.measurement_noise;
        if (H.empty() || v.empty())
        {
            // whichever is not given comes from LQR.info
            std::vector<double> Hf, vf;
            loadMeasurement(Hf, vf);
            if (H.empty())
                H = Hf;
            if (v.empty())
                v = vf;
        }
        if (v.empty() || H.size() != v.size() * NX)
            throw std::invalid_argument("LQRTracker::filter: no measurement: give H [ny][NX] and measurement_noise [ny], or LQR.info a measurement_std vector");
        const bool loop = o.closed_loop < 0 ? !gains.empty() : o.closed_loop != 0;
        int steps = o.steps;
        if (steps <= 0)
        {
            double dt_max = 0., rho = 0.;
            for (const trajectory_data_t &td : tds)
                dt_max = std::max(dt_max, td.t / double(K - 1));
            steps = filterSteps(o.sigma0, H, v, dt_max, &rho);
            if (steps > FILTER_MAX_STEPS)
                throw std::invalid_argument("LQRTracker::filter: the initial transient has the rate rho = max (H sigma0 H')_mm / v_m = " + std::to_string(rho) +
                                            " per second, which needs " + std::to_string(steps) + " steps per segment for h rho <= 1/8; more than " +
                                            std::to_string(FILTER_MAX_STEPS) +
                                            " is refused.  Give steps explicitly, or use a larger measurement_noise or a smaller sigma0.");
        }
        const int ny = int(v.size());
        check(scpp_hip_lqr_set_covariance_inputs(ctx, o.sigma0.data(), int(o.sigma0.size() / (NX * NX)),
                                                 o.disturbance.empty() ? nullptr : o.disturbance.data()),
              "scpp_hip_lqr_set_covariance_inputs");
        check(scpp_hip_lqr_set_measurement(ctx, H.data(), ny, v.data()), "scpp_hip_lqr_set_measurement");
        check(scpp_hip_lqr_filter(ctx, steps, loop ? 1 : 0, o.keep ? 1 : 0, &out.n_ok), "scpp_hip_lqr_filter");
        out.ny = ny;
        out.steps = steps;
        out.closed_loop = loop;
        out.L.assign(B * K * NX * size_t(ny), 0.);
        out.error_std.assign(B * K * NX, 0.);
        out.final_error_cov.assign(B * NX * NX, 0.);
        out.status.assign(B, 0);
        out.error_cov.assign(o.keep ? B * K * NX * NX : 0, 0.);
        out.state_std.assign(loop ? B * K * NX : 0, 0.);
        out.input_cov.assign(loop ? B * K * NU * NU : 0, 0.);
        out.final_state_cov.assign(loop ? B * NX * NX : 0, 0.);
        out.estimate_cov.assign(loop && o.keep ? B * K * NX * NX : 0, 0.);
        auto ptr = [](std::vector<double> &a) { return a.empty() ? nullptr : a.data(); };
        check(scpp_hip_lqr_download_filter(ctx, out.L.data(), out.error_std.data(), out.final_error_cov.data(), out.status.data(), ptr(out.error_cov),
                                           ptr(out.state_std), ptr(out.input_cov), ptr(out.final_state_cov), ptr(out.estimate_cov)),
              "scpp_hip_lqr_download_filter");
    }

    // H [ny][NX] and v [ny] from the optional measurement_std vector of LQR.info (one entry per state: the square root of the noise intensity of a
    // sensor that reads that state, 0: not measured): H selects the non-zero entries, v_m = std_m^2; both empty without the vector
    static void loadMeasurement(std::vector<double> &H, std::vector<double> &v)
    {
        H.clear();
        v.clear();
        const std::vector<double> sd = loadOptionalVector("measurement_std");
        for (size_t j = 0; j < sd.size(); j++)
            if (sd[j] != 0.)
            {
                H.resize(H.size() + NX, 0.);
                H[H.size() - NX + j] = 1.;
                v.push_back(sd[j] * sd[j]);
            }
    }

    // the optional vector `name` of LQR.info (initial_std, disturbance_std: one entry per state); empty without the file or the entry
    static std::vector<double> loadOptionalVector(const std::string &name)
    {
        const std::string file = Model::getParameterFolder() + "/LQR.info";
        if (!std::filesystem::exists(file))
            return {};
        ParameterServer param(file);
        if (!param.has(name))
            return {};
        std::vector<double> v(NX);
        param.loadMatrix(name, v.data(), int(NX));
        return v;
    }

    std::array<double, NX> Q{};
    std::array<double, NU> R{};
    std::vector<feedback_matrix_t> gains; // [B][K]
    std::vector<int32_t> status, iterations; // iterations: sign iterations, or RKF78 steps behind the node (finite horizon, discrete)
    std::vector<double> riccati;             // [B][K][NX][NX], finite horizon with keep_riccati only
    std::vector<double> discrete_P, discrete_Phi, discrete_Gamma; // [B][K][NX][NX], [B][K-1][NX][NX], [B][K-1][NX][NU]: discrete with keep_discrete only
    std::vector<double> feedforward;                 // [B][K][NU] = k_k: affine only
    std::vector<double> affine_P, affine_p, affine_s; // [B][K][NX][NX], [B][K][NX], [B][K]: affine with keep_affine only
    lqr_gain_options_t opts;

private:
    static void check(int rc, const char *what)
    {
        if (rc != SCPP_OK)
            throw std::runtime_error(std::string(what) + " failed with code " + std::to_string(rc));
    }
    Model::ptr_t model;
    std::vector<trajectory_data_t> tds;
    scpp_hip_lqr_ctx *ctx = nullptr;
    int n_ok = 0;
    bool feedforward_on = false;
};

} // namespace scpp

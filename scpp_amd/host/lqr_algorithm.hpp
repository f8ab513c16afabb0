// C++17 host front end: the reference's LQRAlgorithm (scpp_core/include/LQRAlgorithm.hpp, src/LQRAlgorithm.cpp:6-75) -- one constant gain,
// linearised at the model's operating point -- over include/scpp_hip_lqr.h.  The gain comes from the same device kernel as the tracker's
// (a two-node constant "trajectory" at the operating point); only models that declare getOperatingPoint compile here (the reference: Rocket2d).
#pragma once
#include <optional>

#include "lqr_tracker.hpp"

namespace scpp
{

class LQRAlgorithm
{
public:
    static constexpr size_t NX = Model::state_dim, NU = Model::input_dim;
    explicit LQRAlgorithm(Model::ptr_t model_, int device_ = 0) : model(std::move(model_)), device(device_) { loadParameters(); }

    // LQRAlgorithm.cpp:11-25
    void initialize()
    {
        if (!(state_weights_set && input_weights_set))
            throw std::runtime_error("LQRAlgorithm: weights not set");
        model->getOperatingPoint(x_eq, u_eq);
        trajectory_data_t td;
        td.initialize(2, true);
        td.X[0] = td.X[1] = x_eq;
        td.U[0] = td.U[1] = u_eq;
        td.t = 1.;
        const std::pair<std::array<double, NX>, std::array<double, NU>> weights{Q, R};
        LQRTracker node(model, td, device, &weights);
        if (node.status[0] != 0)
            throw std::runtime_error("LQRAlgorithm: the gain at the operating point failed with status " + std::to_string(node.status[0]));
        K = node.gain(0, 0);
        initialized = true;
    }
    // LQRAlgorithm.cpp:27-33
    void solve()
    {
        if (!initialized)
            throw std::runtime_error("LQRAlgorithm::initialize() has not been called");
        Model::input_vector_t v;
        for (size_t r = 0; r < NU; r++)
        {
            double acc = 0.;
            for (size_t c = 0; c < NX; c++)
                acc += K[r][c] * (x_init[c] - x_final[c]);
            v[r] = -acc + u_eq[r];
        }
        u = v;
    }
    void setInitialState(const Model::state_vector_t &x) { x_init = x; }
    void setFinalState(const Model::state_vector_t &x) { x_final = x; }
    void getSolution(Model::input_vector_t &out) const
    {
        if (!u)
            throw std::runtime_error("LQRAlgorithm::solve() has not been called");
        out = *u;
    }
    // LQRAlgorithm.cpp:45-57
    void setStateWeights(const Model::state_vector_t &weights)
    {
        Q = weights;
        state_weights_set = true;
    }
    void setInputWeights(const Model::input_vector_t &weights)
    {
        R = weights;
        input_weights_set = true;
    }
    // LQRAlgorithm.cpp:65-75 (the file is required here, as in the reference; the tracker alone falls back to Q = I, R = I)
    void loadParameters()
    {
        ParameterServer param(Model::getParameterFolder() + "/LQR.info");
        Model::state_vector_t q;
        Model::input_vector_t r;
        param.loadMatrix("state_weights", q.data(), int(NX));
        param.loadMatrix("input_weights", r.data(), int(NU));
        setStateWeights(q);
        setInputWeights(r);
    }

    // the clip of LQR_sim.cpp:55-66 for the loops simulate() flies: (T_min, T_max, angle_max in radians); off by default, and solve()
    // stays the unlimited control law
    void setInputLimits(const std::array<double, 3> &lim) { input_limits = lim; }
    void setInputLimitsFromModel()
    {
        std::array<double, 3> lim{};
        model->inputLimits(lim.data());
        input_limits = lim;
    }
    void clearInputLimits() { input_limits.reset(); }

    // LQR_sim.cpp:43-82 for every start at once, on the device: u = sat(-K (x - x_final) + u_eq) until |x - x_final| < stop_tol or sim_time,
    // `samples` starts per regulator (they all share the one gain, so samples only shapes the fan: x_start.size() must be a multiple)
    void simulate(const std::vector<Model::state_vector_t> &x_start, lqr_track_result_t &out, int samples = 1, double sim_time = 5., double time_step = 0.010,
                  double stop_tol = 0.02, int n_record = 0, int write_steps = 30)
    {
        if (!initialized)
            throw std::runtime_error("LQRAlgorithm::initialize() has not been called");
        if (samples < 1 || x_start.empty() || x_start.size() % size_t(samples) != 0)
            throw std::invalid_argument("LQRAlgorithm::simulate: the starts are no multiple of samples");
        trajectory_data_t td;
        td.initialize(2, true);
        td.X[0] = td.X[1] = x_final;
        td.U[0] = td.U[1] = u_eq;
        td.t = sim_time;
        const std::pair<std::array<double, NX>, std::array<double, NU>> weights{Q, R};
        LQRTracker loop(model, std::vector<trajectory_data_t>(x_start.size() / size_t(samples), td), device, &weights);
        loop.setGains(std::vector<LQRTracker::feedback_matrix_t>(loop.gains.size(), K));
        loop.setStopTolerance(stop_tol);
        if (input_limits)
            loop.setInputLimits(std::vector<double>(input_limits->begin(), input_limits->end()));
        loop.track(x_start, x_final, out, time_step, n_record, write_steps, 20, samples);
    }

    LQRTracker::feedback_matrix_t K{};
    Model::state_vector_t x_eq{};
    Model::input_vector_t u_eq{};

private:
    Model::ptr_t model;
    int device;
    std::array<double, NX> Q{};
    std::array<double, NU> R{};
    bool state_weights_set = false, input_weights_set = false, initialized = false;
    Model::state_vector_t x_init{}, x_final{};
    std::optional<Model::input_vector_t> u;
    std::optional<std::array<double, 3>> input_limits;
};

} // namespace scpp

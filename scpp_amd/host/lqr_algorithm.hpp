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
};

} // namespace scpp

// sc_tracking: the reference's SC_tracking executable (scpp/src/SC_tracking.cpp:17-124) on the device engine, batched.
//   no arguments        : one trajectory from the shipped configuration, solved by SCAlgorithm, one LQR gain per node, the nonlinear plant
//                         flown along it from x_init                                              (what the reference does)
//   --batch N [--seed S]: N randomised initial states: N trajectories, N x K gains, N flights from those initial states
//   --config DIR --out DIR --K n --device d --time-step s
//   --gains frozen|riccati|discrete|affine : frozen (default): one frozen-time infinite-horizon gain per node (the reference's); riccati: finite-horizon gains,
//                         the differential Riccati equation swept backwards along each trajectory; --riccati-steps n RKF78 steps per segment (5)
//                         discrete: sampled-data gains, the discrete Riccati recursion over the segments' transition matrices
//                         (scpp_hip_lqr_compute_gains_discrete); --discrete-steps n RKF78 steps per segment (5)
//                         affine: the finite-horizon law for a nominal that misses its own nodes (scpp_hip_lqr_compute_gains_affine): the riccati
//                         gains and a feedforward term against the nominal's defect, which the loop applies; --affine-steps n RKF78 steps
//                         per segment (5); --no-feedforward flies the same gains without the term (the flights of --gains riccati).
//                         Writes feedforward.txt (one node per row) of instance 0 next to X.txt
//   --hold step|node    : step (default): the feedback term changes on every plant step; node: it is latched at each node and held over the
//                         segment (scpp_hip_lqr_set_feedback_hold), the loop --gains discrete designs for
//   --covariance        : also the closed-loop covariance sweep along every trajectory under those gains (scpp_hip_lqr_propagate_covariance):
//                         S(0) = diag(initial_std)^2 and W = diag(disturbance_std)^2 from the optional vectors initial_std / disturbance_std of
//                         LQR.info (absent: 0); --covariance-steps n RKF78 steps per segment (5).  Writes state_std.txt (one node per row) and
//                         input_cov.txt (one node per row, the nu x nu matrix row-major) of instance 0 next to X.txt
//   --covariance-hold step|node : which loop --covariance describes.  step (default): the continuous loop; node: the loop that latches its
//                         correction at each node and holds it over the segment (scpp_hip_lqr_propagate_covariance_discrete), the loop
//                         --hold node flies.  Used only with --covariance; the same two files
//   --mean              : also where the loop's centre goes (scpp_hip_lqr_propagate_moments): dm/dt = A_cl m + d from m(0) = 0, d the defect of
//                         the nominal minus, under --gains affine without --no-feedforward, B k_t.  Used only together with --covariance and
//                         the continuous loop: with --covariance-hold node it is refused before anything is solved (the held loop's mean is
//                         not built).  --mean-steps n RKF78 steps per segment (default: those of --covariance-steps).  Writes mean.txt and
//                         input_mean.txt (one node per row; the mean correction -G m - k on top of u_ref) of instance 0 next to X.txt
//   --saturate          : input limits inside the closed loop (scpp_hip_lqr_set_input_limits), from the model's parameters T_min, T_max,
//                         gimbal_max.  Writes n_sat.txt (plant steps on which the input was clipped) and max_clip.txt (largest |u_cmd - u|),
//                         one flight per row, next to X.txt
//                         (--saturate and --samples also write x_end.txt: the final state of every flight, one per row)
//   --samples N         : N flights per trajectory (scpp_hip_lqr_track_samples): flight 0 of trajectory b from the initial state the trajectory
//                         was solved for, flights 1 .. N-1 from states drawn by the same randomisation (instances batch + b (N - 1) + s - 1 of
//                         --seed); the trajectories and gains are neither copied nor recomputed
//   --disturbance       : process noise on the plant (scpp_hip_lqr_set_disturbance): w = disturbance_std^2 from LQR.info, the generator keyed
//                         by --seed.  Without the vector in LQR.info it is refused before anything is solved.  Also writes x_end.txt
//   --filter            : also the LQG analysis along every trajectory (scpp_hip_lqr_filter): the Kalman-Bucy filter of the sensors that
//                         measurement_std of LQR.info describes (one entry per state, 0: not measured) and the covariance of the loop closed
//                         on its estimate, under those gains; sigma0 and W as for --covariance.  --filter-steps n RKF78 steps per segment
//                         (default: the smallest count >= 5 with h rho <= 1/8, refused above 200).  Without the vector in LQR.info it is
//                         refused before anything is solved.  Writes error_std.txt, filter_gain.txt (one node per row, the nx x ny matrix
//                         row-major), lqg_state_std.txt and lqg_input_cov.txt of instance 0 next to X.txt
// Writes <out>/output/<Model>/SC_tracking/<time>/0/{X,U,t}.txt of instance 0 (every 30th step, like write_steps of the reference) and prints
// gains/s, tracked plant steps/s and the distribution of the final error.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lqr_tracker.hpp"
#include "output.hpp"

namespace fs = std::filesystem;

static double seconds()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char **argv)
{
    std::string config = "../scpp_amd/config", out = "..";
    int batch = 0, K = 0, device = 0;
    scpp::lqr_gain_options_t gain_opts;
    bool covariance = false, saturate = false, hold_node = false, covariance_hold_node = false, no_feedforward = false, mean = false, disturbance = false;
    int covariance_steps = 5, samples = 1, mean_steps = 0, filter_steps = 0;
    bool filter = false;
    double time_step = 0.01;
    unsigned long long seed = 20260927ull;
    for (int i = 1; i < argc; i++)
    {
        auto next = [&]() -> const char * {
            if (i + 1 >= argc)
            {
                std::fprintf(stderr, "missing value for %s\n", argv[i]);
                std::exit(2);
            }
            return argv[++i];
        };
        if (!std::strcmp(argv[i], "--batch"))
            batch = std::atoi(next());
        else if (!std::strcmp(argv[i], "--seed"))
            seed = std::strtoull(next(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--config"))
            config = next();
        else if (!std::strcmp(argv[i], "--out"))
            out = next();
        else if (!std::strcmp(argv[i], "--K"))
            K = std::atoi(next());
        else if (!std::strcmp(argv[i], "--device"))
            device = std::atoi(next());
        else if (!std::strcmp(argv[i], "--time-step"))
            time_step = std::atof(next());
        else if (!std::strcmp(argv[i], "--gains"))
        {
            const std::string which = next();
            if (which != "frozen" && which != "riccati" && which != "discrete" && which != "affine")
            {
                std::fprintf(stderr, "--gains %s: frozen, riccati, discrete or affine\n", which.c_str());
                return 2;
            }
            gain_opts.finite_horizon = which == "riccati";
            gain_opts.discrete = which == "discrete";
            gain_opts.affine = which == "affine";
        }
        else if (!std::strcmp(argv[i], "--affine-steps"))
            gain_opts.affine_steps = std::atoi(next());
        else if (!std::strcmp(argv[i], "--no-feedforward"))
            no_feedforward = true;
        else if (!std::strcmp(argv[i], "--discrete-steps"))
            gain_opts.discrete_steps = std::atoi(next());
        else if (!std::strcmp(argv[i], "--hold"))
        {
            const std::string which = next();
            if (which != "step" && which != "node")
            {
                std::fprintf(stderr, "--hold %s: step or node\n", which.c_str());
                return 2;
            }
            hold_node = which == "node";
        }
        else if (!std::strcmp(argv[i], "--riccati-steps"))
            gain_opts.riccati_steps = std::atoi(next());
        else if (!std::strcmp(argv[i], "--covariance"))
            covariance = true;
        else if (!std::strcmp(argv[i], "--covariance-steps"))
            covariance_steps = std::atoi(next());
        else if (!std::strcmp(argv[i], "--covariance-hold"))
        {
            const std::string which = next();
            if (which != "step" && which != "node")
            {
                std::fprintf(stderr, "--covariance-hold %s: step or node\n", which.c_str());
                return 2;
            }
            covariance_hold_node = which == "node";
        }
        else if (!std::strcmp(argv[i], "--mean"))
            mean = true;
        else if (!std::strcmp(argv[i], "--mean-steps"))
            mean_steps = std::atoi(next());
        else if (!std::strcmp(argv[i], "--filter"))
            filter = true;
        else if (!std::strcmp(argv[i], "--filter-steps"))
            filter_steps = std::atoi(next());
        else if (!std::strcmp(argv[i], "--saturate"))
            saturate = true;
        else if (!std::strcmp(argv[i], "--disturbance"))
            disturbance = true;
        else if (!std::strcmp(argv[i], "--samples"))
        {
            samples = std::atoi(next());
            if (samples < 1)
            {
                std::fprintf(stderr, "--samples %d: at least 1\n", samples);
                return 2;
            }
        }
        else
        {
            std::fprintf(stderr, "unknown argument %s\n", argv[i]);
            return 2;
        }
    }
    if (mean && !covariance)
    {
        std::fprintf(stderr, "--mean: used only together with --covariance\n");
        return 2;
    }
    if (mean && covariance_hold_node)
    {
        std::fprintf(stderr, "--mean with --covariance-hold node: the mean of the loop that holds its correction is not built\n");
        return 2;
    }
    try
    {
        Model::setParameterFolder(config);
        auto model = std::make_shared<Model>();
        model->loadParameters();
        std::vector<double> noise_w;
        if (disturbance)
        {
            noise_w = scpp::LQRTracker::loadOptionalVector("disturbance_std");
            if (noise_w.empty())
            {
                std::fprintf(stderr, "--disturbance: %s/LQR.info has no disturbance_std vector\n", Model::getParameterFolder().c_str());
                return 2;
            }
            for (double &v : noise_w)
                v *= v;
        }
        std::vector<double> meas_H, meas_v;
        if (filter)
        {
            scpp::LQRTracker::loadMeasurement(meas_H, meas_v);
            if (meas_v.empty())
            {
                std::fprintf(stderr, "--filter: %s/LQR.info has no measurement_std vector (or none of its entries is non-zero)\n",
                             Model::getParameterFolder().c_str());
                return 2;
            }
        }

        std::vector<Model::state_vector_t> x_inits;
        if (batch <= 0)
            x_inits.push_back(model->p.x_init);
        for (int b = 0; b < batch; b++)
        {
            Model inst = *model;
            inst.p.randomizeInitialState(seed, uint64_t(b));
            x_inits.push_back(inst.p.x_init);
        }
        const size_t N = x_inits.size();

        scpp::SCAlgorithm solver(model, int(N), device, K);
        solver.initialize();
        scpp::batch_result_t r;
        double t0 = seconds();
        solver.solveBatch(x_inits, r);
        const double t_solve = seconds() - t0;
        long conv = 0;
        for (size_t b = 0; b < N; b++)
            conv += r.converged[b];
        std::printf("SC batch %zu: converged %ld in %.3f s\n", N, conv, t_solve);

        // calculate LQR gains
        t0 = seconds();
        scpp::LQRTracker tracker(model, r.td, device, nullptr, gain_opts);
        const double t_gains = seconds() - t0;
        const size_t nodes = N * r.td[0].n_X();
        if (gain_opts.finite_horizon)
            std::printf("Gains: riccati (finite horizon, %d RKF78 steps per segment, %zu Riccati right-hand sides)\n", gain_opts.riccati_steps,
                        N * (r.td[0].n_X() - 1) * size_t(gain_opts.riccati_steps) * 13);
        else if (gain_opts.affine)
            std::printf("Gains: affine (finite horizon with feedforward, %d RKF78 steps per segment, %zu Riccati right-hand sides on [e; 1])\n",
                        gain_opts.affine_steps, N * (r.td[0].n_X() - 1) * size_t(gain_opts.affine_steps) * 13);
        else if (gain_opts.discrete)
            std::printf("Gains: discrete (sampled data, %d RKF78 steps per segment, %zu transition right-hand sides)\n", gain_opts.discrete_steps,
                        N * (r.td[0].n_X() - 1) * size_t(gain_opts.discrete_steps) * 13);
        else
            std::printf("Gains: frozen (one infinite-horizon gain per node)\n");
        std::printf("Time, LQR gains: %.2f ms for %zu nodes (%d converged): %.0f gains/s (with context set-up and transfers)\n", 1e3 * t_gains, nodes,
                    tracker.nodesConverged(), double(nodes) / t_gains);

        // closed-loop covariance along every trajectory
        scpp::lqr_covariance_result_t cov;
        scpp::lqr_moments_result_t mom;
        if (covariance)
        {
            constexpr size_t NX = Model::state_dim;
            scpp::lqr_covariance_options_t co;
            co.steps = covariance_steps;
            co.hold_node = covariance_hold_node;
            const std::vector<double> sd0 = scpp::LQRTracker::loadOptionalVector("initial_std");
            co.disturbance = scpp::LQRTracker::loadOptionalVector("disturbance_std");
            co.sigma0.assign(NX * NX, 0.);
            for (size_t j = 0; j < sd0.size(); j++)
                co.sigma0[j * NX + j] = sd0[j] * sd0[j];
            for (double &v : co.disturbance)
                v *= v;
            t0 = seconds();
            tracker.covariance(co, cov);
            const double t_cov = seconds() - t0;
            const size_t rhs = N * (r.td[0].n_X() - 1) * size_t(covariance_steps) * 13;
            std::printf("Covariance: %d RKF78 steps per segment, %zu right-hand sides in %.2f ms (%d of %zu trajectories with status 0)\n", covariance_steps,
                        rhs, 1e3 * t_cov, cov.n_ok, N);
            if (covariance_hold_node)
                std::printf("Covariance hold: node (the sweep of the loop that holds its correction over a segment)\n");
            if (mean)
            {
                const bool ff = gain_opts.affine && !no_feedforward;
                co.steps = mean_steps > 0 ? mean_steps : covariance_steps;
                t0 = seconds();
                tracker.moments(co, {}, mom, ff ? 1 : 0);
                std::printf("Mean: %d RKF78 steps per segment, covariance and mean in %.2f ms, feedforward term %s (%d of %zu trajectories with status 0)\n",
                            co.steps, 1e3 * (seconds() - t0), ff ? "in" : "not in", mom.n_ok, N);
            }
        }

        // the filter of the sensors LQR.info describes, and the loop closed on its estimate
        scpp::lqr_filter_result_t filt;
        if (filter)
        {
            constexpr size_t NX = Model::state_dim;
            scpp::lqr_filter_options_t fo;
            fo.steps = filter_steps;
            fo.H = meas_H;
            fo.measurement_noise = meas_v;
            const std::vector<double> sd0 = scpp::LQRTracker::loadOptionalVector("initial_std");
            fo.disturbance = scpp::LQRTracker::loadOptionalVector("disturbance_std");
            fo.sigma0.assign(NX * NX, 0.);
            for (size_t j = 0; j < sd0.size(); j++)
                fo.sigma0[j * NX + j] = sd0[j] * sd0[j];
            for (double &v : fo.disturbance)
                v *= v;
            t0 = seconds();
            tracker.filter(fo, filt);
            const double t_filt = seconds() - t0;
            std::printf("Filter: %d measurements, %d RKF78 steps per segment, %zu right-hand sides in %.2f ms (%d of %zu trajectories with status 0)\n",
                        filt.ny, filt.steps, N * (r.td[0].n_X() - 1) * size_t(filt.steps) * 13, 1e3 * t_filt, filt.n_ok, N);
        }

        // the starts: `samples` per trajectory, the first of each the state its trajectory was solved for
        std::vector<Model::state_vector_t> x_starts;
        for (size_t b = 0; b < N; b++)
            for (int s = 0; s < samples; s++)
            {
                Model inst = *model;
                if (s > 0)
                    inst.p.randomizeInitialState(seed, uint64_t(batch > 0 ? batch : 0) + uint64_t(b) * uint64_t(samples - 1) + uint64_t(s - 1));
                x_starts.push_back(s > 0 ? inst.p.x_init : x_inits[b]);
            }
        const size_t F = x_starts.size();
        if (saturate)
            tracker.setInputLimitsFromModel();
        tracker.setFeedbackHold(hold_node);
        if (gain_opts.affine && no_feedforward)
            tracker.setFeedforward(false);
        if (disturbance)
            tracker.setDisturbance(noise_w, seed, 0);

        // start simulation
        scpp::lqr_track_result_t sim;
        t0 = seconds();
        tracker.track(x_starts, model->p.x_final, sim, time_step, 1, 30, 20, samples);
        const double t_run = seconds() - t0;
        long steps = 0;
        std::vector<double> rel;
        for (size_t b = 0; b < F; b++)
        {
            steps += sim.steps[b];
            if (sim.status[b] != SCPP_LQR_NONFINITE && sim.initial_error[b] > 0.)
                rel.push_back(100. * sim.final_error[b] / sim.initial_error[b]);
        }
        std::sort(rel.begin(), rel.end());
        std::printf("Simulating %zu trajectories.\nFinished after %d steps (instance 0), %ld plant steps in %.2f ms: %.0f steps/s; %d of %zu flights finite\n", N,
                    sim.steps[0] + 1, steps, 1e3 * t_run, double(steps) / t_run, sim.n_finite, F);
        std::printf("Hold: %s\n", hold_node ? "node (the feedback term is latched at each node and held over the segment)"
                                            : "step (the feedback term changes on every plant step)");
        if (gain_opts.affine)
            std::printf("Feedforward: %s\n", tracker.feedforwardOn() ? "on (u_cmd = u_ref - K_t (x - x_ref) - k_t)" : "off (--no-feedforward: the riccati loop)");
        if (samples > 1)
            std::printf("Sample fan: %d flights per trajectory, %zu flights\n", samples, F);
        if (disturbance)
            std::printf("Disturbance: process noise W = diag(disturbance_std)^2 held over each plant step, seed %llu\n", seed);
        if (saturate)
        {
            size_t clipped = 0;
            double worst = 0.;
            for (size_t f = 0; f < F; f++)
            {
                clipped += sim.n_sat[f] > 0;
                worst = std::max(worst, sim.max_clip[f]);
            }
            std::printf("Input limits: %zu of %zu flights clipped on at least one step, largest clip %.6g\n", clipped, F, worst);
        }
        if (!rel.empty())
            std::printf("Final error: %.4f%% (instance 0); over the batch min %.4f%% median %.4f%% max %.4f%%\n",
                        100. * sim.final_error[0] / sim.initial_error[0], rel.front(), rel[rel.size() / 2], rel.back());

        // write solution to files
        const fs::path outputPath = fs::path(out) / "output" / Model::getModelName() / "SC_tracking" / scpp::getTimeString() / "0";
        scpp::makeDir(outputPath);
        scpp::writeRows(outputPath / "X.txt", sim.X_sim.at(0));
        scpp::writeRows(outputPath / "U.txt", sim.U_sim.at(0));
        {
            std::ofstream f(outputPath / "t.txt");
            for (double t : sim.t_sim.at(0))
                f << t << "\n";
        }
        if (gain_opts.affine)
        {
            // k_k of instance 0, one node per row, round-trip precision
            constexpr size_t NU = Model::input_dim;
            std::ofstream ff(outputPath / "feedforward.txt");
            ff.precision(17);
            for (size_t k = 0; k < r.td[0].n_X(); k++)
                for (size_t j = 0; j < NU; j++)
                    ff << tracker.feedforward[k * NU + j] << (j + 1 < NU ? ", " : "\n");
        }
        if (saturate || samples > 1 || disturbance)
        {
            // the final state of every flight, one per row, round-trip precision
            std::ofstream fx(outputPath / "x_end.txt");
            fx.precision(17);
            for (size_t f = 0; f < F; f++)
                for (size_t j = 0; j < sim.x[f].size(); j++)
                    fx << sim.x[f][j] << (j + 1 < sim.x[f].size() ? ", " : "\n");
        }
        if (saturate)
        {
            std::ofstream fn(outputPath / "n_sat.txt"), fc(outputPath / "max_clip.txt");
            fc.precision(17);
            for (size_t f = 0; f < F; f++)
            {
                fn << sim.n_sat[f] << "\n";
                fc << sim.max_clip[f] << "\n";
            }
        }
        if (covariance)
        {
            constexpr size_t NX = Model::state_dim, NU = Model::input_dim;
            const size_t Kn = r.td[0].n_X();
            std::vector<std::vector<double>> sd(Kn), ic(Kn);
            for (size_t k = 0; k < Kn; k++)
            {
                sd[k].assign(&cov.state_std[k * NX], &cov.state_std[k * NX] + NX);
                ic[k].assign(&cov.input_cov[k * NU * NU], &cov.input_cov[k * NU * NU] + NU * NU);
            }
            scpp::writeRows(outputPath / "state_std.txt", sd);
            scpp::writeRows(outputPath / "input_cov.txt", ic);
            if (mean)
            {
                // m(t_k) and the mean correction of instance 0, one node per row, round-trip precision
                std::ofstream fm(outputPath / "mean.txt"), fu(outputPath / "input_mean.txt");
                fm.precision(17);
                fu.precision(17);
                for (size_t k = 0; k < Kn; k++)
                {
                    for (size_t j = 0; j < NX; j++)
                        fm << mom.mean[k * NX + j] << (j + 1 < NX ? ", " : "\n");
                    for (size_t j = 0; j < NU; j++)
                        fu << mom.input_mean[k * NU + j] << (j + 1 < NU ? ", " : "\n");
                }
            }
        }
        if (filter)
        {
            // instance 0, one node per row, round-trip precision
            constexpr size_t NX = Model::state_dim, NU = Model::input_dim;
            const size_t Kn = r.td[0].n_X(), nL = NX * size_t(filt.ny);
            auto rows = [&](const char *name, const std::vector<double> &a, size_t n) {
                std::ofstream f(outputPath / name);
                f.precision(17);
                for (size_t k = 0; k < Kn; k++)
                    for (size_t j = 0; j < n; j++)
                        f << a[k * n + j] << (j + 1 < n ? ", " : "\n");
            };
            rows("error_std.txt", filt.error_std, NX);
            rows("filter_gain.txt", filt.L, nL);
            rows("lqg_state_std.txt", filt.state_std, NX);
            rows("lqg_input_cov.txt", filt.input_cov, NU * NU);
        }
        std::printf("output: %s\n", outputPath.string().c_str());
    }
    catch (const std::exception &e)
    {
        std::fprintf(stderr, "sc_tracking: %s\n", e.what());
        return 1;
    }
    return 0;
}

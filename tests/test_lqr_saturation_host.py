"""host/sc_tracking --saturate --samples 3 against the CPU emulation libraries: the files it writes (n_sat.txt, max_clip.txt, x_end.txt, one
flight per row) equal the arrays of the Python front end for the same configuration, limits from the model's parameters and the same
dispersed starts."""
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "scpp_amd", "host")

pytestmark = pytest.mark.xdist_group("host_cpp")  # one build directory (scpp_amd/host): keep the module on the worker of tests/test_host_cpp.py


def test_sc_tracking_saturation_files_equal_the_python_front_end(emu_lib, tmp_path):
    import __graft_entry__ as g
    import scpp_amd

    lqr_emu = g.build_lqr_emu()
    subprocess.check_call(["make", "-s", "-C", HOST, "sc_tracking_emu"])
    K, B, S = 10, 2, 3
    cfg = os.path.join(ROOT, "scpp_amd", "config")
    cmd = [os.path.join(HOST, "sc_tracking_emu"), "--K", str(K), "--batch", str(B), "--config", cfg, "--out", str(tmp_path)]
    r = subprocess.run(cmd + ["--saturate", "--samples", str(S)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert f"Sample fan: {S} flights per trajectory, {B * S} flights" in r.stdout and "Input limits: " in r.stdout
    run = glob.glob(str(tmp_path / "output" / "RocketQuat" / "SC_tracking" / "*" / "0"))[0]
    assert sorted(os.listdir(run)) == ["U.txt", "X.txt", "max_clip.txt", "n_sat.txt", "t.txt", "x_end.txt"]
    n_sat = np.loadtxt(os.path.join(run, "n_sat.txt"), dtype=np.int64, ndmin=1)
    max_clip = np.loadtxt(os.path.join(run, "max_clip.txt"), ndmin=1)
    x_end = np.loadtxt(os.path.join(run, "x_end.txt"), delimiter=",", ndmin=2)
    assert n_sat.shape == (B * S,) and max_clip.shape == (B * S,) and x_end.shape == (B * S, 14)

    model = scpp_amd.RocketQuat(cfg).loadParameters()
    x0 = model.randomized_initial_states(B)
    alg = scpp_amd.SCAlgorithm(model, K=K, batch_max=B, library=emu_lib).initialize()
    alg.solve(x0)
    trk = scpp_amd.LQRTracker.from_algorithm(alg, library=lqr_emu)
    # flight 0 of trajectory b: the state it was solved for; flights 1 .. S-1: instances B + b (S - 1) + s - 1 of the same randomisation
    xs = np.stack([x0[b] if s == 0 else model.randomized_initial_states(1, first=B + b * (S - 1) + s - 1)[0] for b in range(B) for s in range(S)])
    trk.setInputLimits("model")
    out = trk.track(xs, samples=S)
    trk.setInputLimits(None)
    off = trk.track(xs, samples=S)
    trk.close()
    assert (out["status"] == 0).all()
    assert (n_sat == out["n_sat"]).all() and (n_sat > 0).any() and (off["n_sat"] == 0).all()
    assert np.allclose(max_clip, out["max_clip"], rtol=1e-12, atol=0.0)
    assert np.allclose(x_end, out["x"], rtol=1e-12, atol=1e-12 * np.abs(out["x"]).max(axis=0))
    assert not np.allclose(out["x"], off["x"], rtol=1e-6)  # the limits acted on what was compared

    # without the flags nothing new is written and nothing new is printed
    out2 = tmp_path / "plain"
    r = subprocess.run(cmd[:-1] + [str(out2)], capture_output=True, text=True)
    assert r.returncode == 0 and "Input limits" not in r.stdout and "Sample fan" not in r.stdout
    run2 = glob.glob(str(out2 / "output" / "RocketQuat" / "SC_tracking" / "*" / "0"))[0]
    assert sorted(os.listdir(run2)) == ["U.txt", "X.txt", "t.txt"]


PROGRAM = r"""
#include <cstdio>
#include "lqr_algorithm.hpp"
int main(int, char **argv)
{
    Model::setParameterFolder(argv[1]);
    auto m = std::make_shared<Model>();
    m->loadParameters();
    scpp::LQRAlgorithm a(m);
    a.initialize();
    a.setFinalState(m->p.x_final);
    std::vector<Model::state_vector_t> xs(4, m->p.x_init);
    for (size_t f = 0; f < xs.size(); f++)
        xs[f][0] += 0.5 * double(f);
    for (int limited = 0; limited < 2; limited++)
    {
        if (limited)
            a.setInputLimitsFromModel();
        scpp::lqr_track_result_t o;
        a.simulate(xs, o, 2, 0.5);
        for (size_t f = 0; f < xs.size(); f++)
        {
            std::printf("%d %d %d %.17g", limited, o.steps[f], o.n_sat[f], o.max_clip[f]);
            for (double v : o.x[f])
                std::printf(" %.17g", v);
            std::printf("\n");
        }
    }
    return 0;
}
"""


def test_lqr_algorithm_simulate_with_limits_equals_lqrsim(emu_lib, tmp_path):
    """host/lqr_algorithm.hpp (Rocket2D; no shipped executable includes it, so it is compiled here against the emulation libraries):
    LQRAlgorithm::simulate, four starts as a fan of two per regulator, with and without setInputLimitsFromModel, against the Python LQRSim
    with setInputLimits("model") on the same starts: steps and n_sat equal, max_clip and the final states to 1e-12."""
    import __graft_entry__ as g
    import scpp_amd

    lqr_emu = g.build_lqr_emu()
    emu = os.path.dirname(lqr_emu)
    src, exe = tmp_path / "lqr_sim.cpp", tmp_path / "lqr_sim"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-DSCPP_ACTIVE_MODEL_ROCKET2D", "-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                           str(src), "-o", str(exe), "-L" + emu, "-l:" + os.path.basename(emu_lib), "-l:" + os.path.basename(lqr_emu), "-Wl,-rpath," + emu])
    cfg = os.path.join(ROOT, "scpp_amd", "config")
    r = subprocess.run([str(exe), cfg], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    rows = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()])
    assert rows.shape == (8, 4 + 6)

    m = scpp_amd.Rocket2D(cfg).loadParameters()
    alg = scpp_amd.LQRAlgorithm(m, library=lqr_emu).initialize()
    xs = np.tile(np.asarray(m.p.x_init, dtype=np.float64), (4, 1))
    xs[:, 0] += 0.5 * np.arange(4)
    for limited in (0, 1):
        alg.setInputLimits("model" if limited else None)
        o = scpp_amd.LQRSim(alg, sim_time=0.5).run(xs)
        c = rows[rows[:, 0] == limited]
        assert (c[:, 1] == o["steps"]).all() and (c[:, 2] == o["n_sat"]).all()
        assert np.allclose(c[:, 3], o["max_clip"], rtol=1e-12, atol=0.0)
        assert np.allclose(c[:, 4:], o["x"], rtol=1e-12, atol=1e-12 * np.abs(o["x"]).max())
        assert (o["n_sat"] > 0).all() if limited else (o["n_sat"] == 0).all()

"""host/sc_tracking --disturbance --seed 7 against the CPU emulation libraries: the files it writes equal the arrays of the Python front end for
the same configuration (w = disturbance_std^2 of LQR.info, the generator keyed by the seed); without the flag it writes what it wrote before;
the flag without a disturbance_std vector is refused before anything is solved."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "scpp_amd", "host")

pytestmark = pytest.mark.xdist_group("host_cpp")  # one build directory (scpp_amd/host): keep the module on the worker of tests/test_host_cpp.py


def test_sc_tracking_disturbance_files_equal_the_python_front_end(emu_lib, tmp_path):
    import __graft_entry__ as g
    import scpp_amd

    lqr_emu = g.build_lqr_emu()
    subprocess.check_call(["make", "-s", "-C", HOST, "sc_tracking_emu"])
    K, B, seed = 10, 2, 7
    shipped = os.path.join(ROOT, "scpp_amd", "config")
    exe = os.path.join(HOST, "sc_tracking_emu")

    # the shipped LQR.info has no disturbance_std: refused, with a message, before anything is solved
    r = subprocess.run([exe, "--K", str(K), "--batch", str(B), "--config", shipped, "--out", str(tmp_path / "refused"), "--disturbance"],
                       capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode != 0 and "disturbance_std" in r.stderr and "SC batch" not in r.stdout
    assert not (tmp_path / "refused").exists()

    # a configuration of its own: the shipped one plus a disturbance_std vector (0 on the mass)
    cfg = str(tmp_path / "config")
    shutil.copytree(shipped, cfg)
    std = np.array([0.0] + [0.05] * 3 + [0.2] * 3 + [1e-3] * 4 + [2e-3] * 3)
    with open(os.path.join(cfg, "RocketQuat", "LQR.info"), "a") as f:
        f.write("disturbance_std { scaling 1. " + " ".join(f"({i}) {v!r}" for i, v in enumerate(std.tolist())) + " }\n")
    cmd = [exe, "--K", str(K), "--batch", str(B), "--seed", str(seed), "--config", cfg]
    r = subprocess.run(cmd + ["--out", str(tmp_path), "--disturbance"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and f"seed {seed}" in r.stdout and "Disturbance: " in r.stdout
    run = glob.glob(str(tmp_path / "output" / "RocketQuat" / "SC_tracking" / "*" / "0"))[0]
    assert sorted(os.listdir(run)) == ["U.txt", "X.txt", "t.txt", "x_end.txt"]
    x_end = np.loadtxt(os.path.join(run, "x_end.txt"), delimiter=",", ndmin=2)
    X_rec = np.loadtxt(os.path.join(run, "X.txt"), delimiter=",", ndmin=2)
    assert x_end.shape == (B, 14)

    model = scpp_amd.RocketQuat(cfg).loadParameters()
    x0 = model.randomized_initial_states(B, seed=seed)
    alg = scpp_amd.SCAlgorithm(model, K=K, batch_max=B, library=emu_lib).initialize()
    alg.solve(x0)
    trk = scpp_amd.LQRTracker.from_algorithm(alg, library=lqr_emu)
    _, dstd = scpp_amd.lqr.load_lqr_covariance_inputs(model)
    assert (dstd == std).all()
    on = trk.track(x0, disturbance=dstd ** 2, seed=seed, n_record=1, write_steps=30)
    off = trk.track(x0, n_record=1, write_steps=30)
    trk.close()
    assert (on["status"] == 0).all()
    assert np.allclose(x_end, on["x"], rtol=1e-12, atol=1e-12 * np.abs(on["x"]).max(axis=0))
    n = int(on["record"]["n"][0])
    assert X_rec.shape == (n, 14) and np.allclose(X_rec, on["record"]["X"][0, :n], rtol=1e-5, atol=1e-5 * np.abs(X_rec).max())  # 6 digits in X.txt
    assert not np.allclose(on["x"], off["x"], rtol=1e-6)  # the noise acted on what was compared

    # without the flag nothing new is written or printed, and the flights are the undisturbed ones
    r = subprocess.run(cmd + ["--out", str(tmp_path / "plain")], capture_output=True, text=True)
    assert r.returncode == 0 and "Disturbance" not in r.stdout
    run2 = glob.glob(str(tmp_path / "plain" / "output" / "RocketQuat" / "SC_tracking" / "*" / "0"))[0]
    assert sorted(os.listdir(run2)) == ["U.txt", "X.txt", "t.txt"]
    X_plain = np.loadtxt(os.path.join(run2, "X.txt"), delimiter=",", ndmin=2)
    n0 = int(off["record"]["n"][0])
    assert X_plain.shape == (n0, 14) and np.allclose(X_plain, off["record"]["X"][0, :n0], rtol=1e-5, atol=1e-5 * np.abs(X_plain).max())

"""host/sc_tracking --covariance against the CPU emulation libraries: the files it writes (state_std.txt, input_cov.txt of instance 0, the
reference's CSV format with 6 significant digits) equal the arrays of the Python front end for the same configuration."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "scpp_amd", "host")

pytestmark = pytest.mark.xdist_group("host_cpp")  # one build directory (scpp_amd/host): keep the module on the worker of tests/test_host_cpp.py


def test_sc_tracking_covariance_files_equal_the_python_front_end(emu_lib, tmp_path):
    import __graft_entry__ as g
    import scpp_amd

    lqr_emu = g.build_lqr_emu()
    subprocess.check_call(["make", "-s", "-C", HOST, "sc_tracking_emu"])
    cfg = tmp_path / "config"
    shutil.copytree(os.path.join(ROOT, "scpp_amd", "config"), cfg)
    sd0 = [5.0, 2.0, 2.0, 2.0, 0.5, 0.5, 0.5, 0.01, 0.01, 0.01, 0.01, 0.02, 0.02, 0.02]
    dist = [0.0, 0.0, 0.0, 0.0, 0.1, 0.1, 0.1, 0.0, 0.0, 0.0, 0.0, 0.01, 0.01, 0.01]
    with open(cfg / "RocketQuat" / "LQR.info", "a") as f:
        f.write("\ninitial_std\n{\n" + "".join(f"    ({i}) {v}\n" for i, v in enumerate(sd0)) + "}\n")
        f.write("disturbance_std\n{\n" + "".join(f"    ({i}) {v}\n" for i, v in enumerate(dist)) + "}\n")
    K, steps = 10, 3
    cmd = [os.path.join(HOST, "sc_tracking_emu"), "--K", str(K), "--config", str(cfg), "--out", str(tmp_path)]
    r = subprocess.run(cmd + ["--covariance", "--covariance-steps", str(steps)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert f"Covariance: {steps} RKF78 steps per segment, {(K - 1) * steps * 13} right-hand sides" in r.stdout and "(1 of 1 trajectories with status 0)" in r.stdout
    run = glob.glob(str(tmp_path / "output" / "RocketQuat" / "SC_tracking" / "*" / "0"))[0]
    sd = np.loadtxt(os.path.join(run, "state_std.txt"), delimiter=",", ndmin=2)
    ic = np.loadtxt(os.path.join(run, "input_cov.txt"), delimiter=",", ndmin=2)
    assert sd.shape == (K, 14) and ic.shape == (K, 16)

    model = scpp_amd.RocketQuat(str(cfg)).loadParameters()
    alg = scpp_amd.SCAlgorithm(model, K=K, library=emu_lib).initialize()
    alg.solve()
    trk = scpp_amd.LQRTracker.from_algorithm(alg, library=lqr_emu)
    s0, w = scpp_amd.load_lqr_covariance_inputs(model)
    assert s0.tolist() == sd0 and w.tolist() == dist
    out = trk.covariance(np.diag(s0 * s0), w * w, steps=steps)
    trk.close()
    assert out["status"].tolist() == [0]
    assert np.allclose(sd, out["state_std"][0], rtol=2e-5, atol=2e-5 * np.abs(out["state_std"][0]).max(axis=0))
    icp = out["input_cov"][0].reshape(K, 16)
    assert np.allclose(ic, icp, rtol=2e-5, atol=2e-5 * np.abs(icp).max(axis=0))
    assert (sd[0] == np.array(sd0)).all() and sd[-1].max() > 0

    # without the flag nothing new is written and nothing new is printed
    out2 = tmp_path / "plain"
    r = subprocess.run(cmd[:-1] + [str(out2)], capture_output=True, text=True)
    assert r.returncode == 0 and "Covariance" not in r.stdout
    run2 = glob.glob(str(out2 / "output" / "RocketQuat" / "SC_tracking" / "*" / "0"))[0]
    assert sorted(os.listdir(run2)) == ["U.txt", "X.txt", "t.txt"]

"""host/sc_tracking --covariance --covariance-hold node against the CPU emulation libraries: the files it writes (state_std.txt,
input_cov.txt of instance 0, the reference's CSV format with 6 significant digits) equal the arrays of the Python front end's
covariance(hold="node") for the same configuration; without --covariance-hold it writes what it wrote before; another word is refused."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "scpp_amd", "host")

pytestmark = pytest.mark.xdist_group("host_cpp")  # one build directory (scpp_amd/host): keep the module on the worker of tests/test_host_cpp.py

SD0 = [5.0, 2.0, 2.0, 2.0, 0.5, 0.5, 0.5, 0.01, 0.01, 0.01, 0.01, 0.02, 0.02, 0.02]
DIST = [0.0, 0.0, 0.0, 0.0, 0.1, 0.1, 0.1, 0.0, 0.0, 0.0, 0.0, 0.01, 0.01, 0.01]


def files_of(out):
    run = glob.glob(str(out / "output" / "RocketQuat" / "SC_tracking" / "*" / "0"))[0]
    return (np.loadtxt(os.path.join(run, "state_std.txt"), delimiter=",", ndmin=2), np.loadtxt(os.path.join(run, "input_cov.txt"), delimiter=",", ndmin=2),
            sorted(os.listdir(run)))


def close(a, b):
    return np.allclose(a, b, rtol=2e-5, atol=2e-5 * np.abs(b).max(axis=0))


def test_sc_tracking_covariance_hold_node_files_equal_the_python_front_end(emu_lib, tmp_path):
    import __graft_entry__ as g
    import scpp_amd

    lqr_emu = g.build_lqr_emu()
    subprocess.check_call(["make", "-s", "-C", HOST, "sc_tracking_emu"])
    cfg = tmp_path / "config"
    shutil.copytree(os.path.join(ROOT, "scpp_amd", "config"), cfg)
    with open(cfg / "RocketQuat" / "LQR.info", "a") as f:
        f.write("\ninitial_std\n{\n" + "".join(f"    ({i}) {v}\n" for i, v in enumerate(SD0)) + "}\n")
        f.write("disturbance_std\n{\n" + "".join(f"    ({i}) {v}\n" for i, v in enumerate(DIST)) + "}\n")
    K, steps = 10, 3
    base = [os.path.join(HOST, "sc_tracking_emu"), "--K", str(K), "--config", str(cfg), "--gains", "discrete", "--discrete-steps", str(steps),
            "--hold", "node", "--covariance", "--covariance-steps", str(steps)]
    r = subprocess.run(base + ["--covariance-hold", "node", "--out", str(tmp_path / "node")], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert f"Covariance: {steps} RKF78 steps per segment" in r.stdout and "(1 of 1 trajectories with status 0)" in r.stdout
    assert "Covariance hold: node" in r.stdout and "Hold: node" in r.stdout
    sd, ic, names = files_of(tmp_path / "node")
    assert sd.shape == (K, 14) and ic.shape == (K, 16) and names == ["U.txt", "X.txt", "input_cov.txt", "state_std.txt", "t.txt"]

    model = scpp_amd.RocketQuat(str(cfg)).loadParameters()
    alg = scpp_amd.SCAlgorithm(model, K=K, library=emu_lib).initialize()
    alg.solve()
    trk = scpp_amd.LQRTracker.from_algorithm(alg, library=lqr_emu, horizon="discrete", discrete_steps=steps)
    s0, w = scpp_amd.load_lqr_covariance_inputs(model)
    node = trk.covariance(np.diag(s0 * s0), w * w, steps=steps, hold="node")
    step = trk.covariance(np.diag(s0 * s0), w * w, steps=steps)
    trk.close()
    assert node["status"].tolist() == [0] and step["status"].tolist() == [0]
    assert close(sd, node["state_std"][0]) and close(ic, node["input_cov"][0].reshape(K, 16))
    assert (sd[0] == np.array(SD0)).all() and sd[-1].max() > 0
    assert not close(sd, step["state_std"][0])  # the two loops differ by more than the files' six digits

    # without --covariance-hold, and with --covariance-hold step: what the command wrote before, the continuous loop's sweep
    for extra, where in (([], "plain"), (["--covariance-hold", "step"], "step")):
        r = subprocess.run(base + extra + ["--out", str(tmp_path / where)], capture_output=True, text=True)
        assert r.returncode == 0 and "Covariance hold" not in r.stdout and f"Covariance: {steps} RKF78 steps per segment" in r.stdout
        sd2, ic2, names2 = files_of(tmp_path / where)
        assert names2 == names and close(sd2, step["state_std"][0]) and close(ic2, step["input_cov"][0].reshape(K, 16))

    # another word is refused with a message, before anything is solved
    r = subprocess.run(base + ["--covariance-hold", "bogus", "--out", str(tmp_path / "bogus")], capture_output=True, text=True)
    assert r.returncode != 0 and "--covariance-hold bogus: step or node" in r.stderr and not (tmp_path / "bogus").exists()

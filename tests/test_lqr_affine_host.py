"""host/sc_tracking --gains affine against the CPU emulation libraries: it names the law and the feedforward setting in its summary and writes
feedforward.txt of instance 0 (17 significant digits), equal to the Python front end's terms for the same configuration; --no-feedforward
reproduces the flight files of --gains riccati at the same step count; the refused words stay refused."""
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "scpp_amd", "host")

pytestmark = pytest.mark.xdist_group("host_cpp")  # one build directory (scpp_amd/host): keep the module on the worker of tests/test_host_cpp.py


def run_dir(out):
    return glob.glob(str(out / "output" / "RocketQuat" / "SC_tracking" / "*" / "0"))[0]


def test_sc_tracking_affine_files_equal_the_python_front_end(emu_lib, tmp_path):
    import __graft_entry__ as g
    import scpp_amd

    lqr_emu = g.build_lqr_emu()
    subprocess.check_call(["make", "-s", "-C", HOST, "sc_tracking_emu"])
    K, steps = 10, 3
    cfg = os.path.join(ROOT, "scpp_amd", "config")
    base = [os.path.join(HOST, "sc_tracking_emu"), "--K", str(K), "--config", cfg]

    def run(extra, where):
        r = subprocess.run(base + extra + ["--out", str(tmp_path / where)], capture_output=True, text=True)
        print(r.stdout, r.stderr)
        assert r.returncode == 0
        d = run_dir(tmp_path / where)
        return r.stdout, d, {n: open(os.path.join(d, n)).read() for n in ("X.txt", "U.txt", "t.txt")}

    out, d, on = run(["--gains", "affine", "--affine-steps", str(steps)], "affine")
    assert "Gains: affine" in out and f"{steps} RKF78 steps per segment" in out and "Feedforward: on" in out and "Final error:" in out
    assert sorted(os.listdir(d)) == ["U.txt", "X.txt", "feedforward.txt", "t.txt"]
    ff = np.loadtxt(os.path.join(d, "feedforward.txt"), delimiter=",", ndmin=2)

    model = scpp_amd.RocketQuat(cfg).loadParameters()
    alg = scpp_amd.SCAlgorithm(model, K=K, library=emu_lib).initialize()
    alg.solve()
    trk = scpp_amd.LQRTracker.from_algorithm(alg, library=lqr_emu, horizon="affine", affine_steps=steps)
    want = trk.affine()["ff"][0]
    trk.close()
    assert ff.shape == (K, 4) and np.array_equal(ff, want) and np.abs(ff).max() > 0 and (ff[-1] == 0).all()

    out, d2, off = run(["--gains", "affine", "--affine-steps", str(steps), "--no-feedforward"], "off")
    assert "Gains: affine" in out and "Feedforward: off" in out and os.path.exists(os.path.join(d2, "feedforward.txt"))
    out, _, ric = run(["--gains", "riccati", "--riccati-steps", str(steps)], "riccati")
    assert "Gains: riccati" in out and "Feedforward" not in out
    assert off == ric  # the same gains without the term: the same flight, file for file
    assert on["U.txt"] != ric["U.txt"]

    # the refused words stay refused, before anything is solved
    for extra in (["--gains", "other"], ["--hold", "other"]):
        r = subprocess.run(base + extra + ["--out", str(tmp_path / "bogus")], capture_output=True, text=True)
        assert r.returncode == 2 and not (tmp_path / "bogus").exists()

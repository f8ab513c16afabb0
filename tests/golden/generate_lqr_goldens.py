"""Goldens of the LQR tracker tests (tests/test_lqr.py): python tests/golden/generate_lqr_goldens.py  ->  tests/golden/lqr_<model>.npz

numpy / scipy / the oracle only (tests/lqr_reference.py); nothing here touches the kernels under test.

Per model a few DYNAMICALLY EXACT nominal trajectories: a smooth input profile sampled at the nodes and integrated from node to node by
oracle_simulate with the hold the tracker assumes (first-order: the input interpolated between the nodes; zero-order: constant).  Solver
output is deliberately not used: a converged SCvx trajectory misses its own next node by tens of m/s, so tracking it says nothing about the
tracker.  RocketQuat trajectory 0 flies with the thrust along the body axis (w_B = 0 at EVERY node: the reference's 14-state Hamiltonian is
exactly singular there); trajectory 1 starts at w_B = 0 and, its lateral thrust being antisymmetric about the mid-point, returns to it.

The generator asserts, with the restatement alone:
  * every node's sign iteration converges (status 0) and its gain agrees with scipy's solve_continuous_are to 1e-5 of max|K|;
  * the iteration count of a copy whose Jacobians are perturbed by 1 ulp is equal on >= 95 % of the nodes and within +-1 elsewhere
    (the cap the tests put on the device);
  * the restatement's tracked final state moves by less than 1e-9 of max|x| when every plant step is taken as two half steps (stored:
    the bar of the device-loop test rests on it);
  * for the stored weights and dispersed starts the tracked flight ends within 1/4 of the open-loop (G = 0) final error, for every start.
Stored: X, U, t, par, weights, scipy gains, restatement gains / iteration counts, the restatement-vs-scipy gap per node, the starts, the
open-loop and closed-loop final errors and the undisturbed excursion of the restatement.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lqr_reference as ref  # noqa: E402
import oracle_lib  # noqa: E402
import scpp_amd  # noqa: E402

N_STARTS = 8
# MASS: the models with a mass state burn m' = -alpha_m |T|, so every m/s of vertical velocity a controller removes leaves about
# alpha_m m = 9 kg in the final |x - x_final| that no gain can take back (mass is not controllable independently of v_z).  The dispersions
# of those models are therefore mostly lateral, where a correction changes |T| to second order only.
TIME_STEP = 0.01


def integrate(model, par, x0, U, t, foh):
    K = U.shape[0] if foh else U.shape[0] + 1
    X = np.zeros((K, x0.size))
    X[0] = x0
    dt = t / (K - 1)
    for k in range(K - 1):
        X[k + 1] = oracle_lib.simulate(model, par, dt, U[k], U[k + 1] if foh else U[k], X[k])
    return X


def rocket2d_cases():
    m = scpp_amd.Rocket2D().loadParameters()
    par = m.flow_params()
    hover = -par[3] * par[0]
    K, t = 30, 12.0
    s = np.linspace(0.0, 1.0, K)
    cases = []
    for j, (x0, amp, ph) in enumerate([(np.array([-30.0, 300.0, 6.0, -45.0, -0.08, 0.0]), 0.02, 0.0),
                                       (np.array([20.0, 250.0, -4.0, -38.0, 0.05, 0.0]), -0.015, 0.7)]):
        U = np.stack([amp * np.sin(2 * np.pi * s + ph), hover * (1.25 + 0.1 * np.cos(2 * np.pi * s + j))], axis=1)
        cases.append(dict(U=U, x0=x0, t=t, foh=True))
    Uz = np.stack([0.02 * np.sin(2 * np.pi * s[:-1]), hover * (1.2 + 0.1 * np.cos(2 * np.pi * s[:-1]))], axis=1)
    cases.append(dict(U=Uz, x0=np.array([-30.0, 300.0, 6.0, -45.0, -0.08, 0.0]), t=t, foh=False))
    q = np.ones(6)
    r = np.array([1e4, 1e-6])
    disp = np.array([8.0, 8.0, 2.0, 2.0, 0.04, 0.01])
    return oracle_lib.ROCKET2D, par, cases, q, r, disp


def lander3dof_cases():
    m = scpp_amd.Lander3dof().loadParameters()
    par = m.flow_params(nondimensionalize=False)
    K, t = 50, 12.0
    s = np.linspace(0.0, 1.0, K)
    w0 = 24000.0 * 9.81
    cases = []
    for j, x0 in enumerate([np.array([24000.0, 150.0, 120.0, 600.0, -25.0, -20.0, -70.0]), np.array([23500.0, -90.0, 60.0, 450.0, 14.0, -9.0, -55.0])]):
        sg = 1.0 if j == 0 else -1.0
        U = np.stack([sg * 0.12 * w0 * np.cos(np.pi * s), 0.08 * w0 * np.sin(2 * np.pi * s + j), w0 * (1.3 + 0.1 * np.sin(2 * np.pi * s))], axis=1)
        cases.append(dict(U=U, x0=x0, t=t, foh=True))
    cases.append(dict(U=cases[0]["U"][:-1].copy(), x0=cases[0]["x0"], t=t, foh=False))
    q = np.ones(7)
    r = np.full(3, 1e-6)
    disp = np.array([0.0, 15.0, 15.0, 3.0, 3.0, 3.0, 0.3])  # (see MASS below)
    return oracle_lib.LANDER3DOF, par, cases, q, r, disp


def rocketquat_cases():
    m = scpp_amd.RocketQuat().loadParameters()
    par = m.flow_params(nondimensionalize=False)
    K, t = 50, 12.0
    s = np.linspace(0.0, 1.0, K)
    w0 = 24000.0 * 9.81
    q0 = np.array(scpp_amd.models.euler_to_quaternion_xyz([0.10, -0.08, 0.0]))
    x0 = np.concatenate([[24000.0], [120.0, 90.0, 600.0], [-20.0, -15.0, -70.0], q0, [0.0, 0.0, 0.0]])
    cases = []
    # 0: thrust along the body axis: no torque, w_B = 0 exactly at every node
    U = np.stack([np.zeros(K), np.zeros(K), w0 * (1.3 + 0.1 * np.sin(2 * np.pi * s)), np.zeros(K)], axis=1)
    cases.append(dict(U=U, x0=x0, t=t, foh=True))
    # 1: lateral thrust antisymmetric about the mid-point (U[k] = -U[K-1-k]): w_B starts at 0 and returns to it
    lat = 0.01 * w0 * np.sin(2 * np.pi * s) * (1.0 + 0.5 * np.cos(2 * np.pi * s))
    lat = 0.5 * (lat - lat[::-1])
    U = np.stack([lat, -0.6 * lat, w0 * (1.3 + 0.1 * np.cos(2 * np.pi * s)), np.zeros(K)], axis=1)
    cases.append(dict(U=U, x0=x0, t=t, foh=True))
    # zero-order hold (K - 1 inputs): the tangent path with node K-1 linearised at U[K-2]; starts at w_B = 0
    cases.append(dict(U=U[:-1].copy(), x0=x0, t=t, foh=False))
    q = np.ones(14)
    r = np.array([1e-6, 1e-6, 1e-6, 1e-6])
    disp = np.array([0.0, 15.0, 15.0, 3.0, 3.0, 3.0, 0.3, 0.03, 0.03, 0.03, 0.03, 0.01, 0.01, 0.01])  # (see MASS below)
    return oracle_lib.ROCKETQUAT, par, cases, q, r, disp


def starts(model, x0, disp, rng):
    """N_STARTS dispersed starts around x0 (per state a random sign times 0.6 .. 1 of disp, so that no start happens to sit on the nominal);
    a quaternion is re-normalised"""
    out = np.zeros((N_STARTS, x0.size))
    for i in range(N_STARTS):
        x = x0 + disp * rng.choice([-1.0, 1.0], x0.size) * rng.uniform(0.6, 1.0, x0.size)
        if model == oracle_lib.ROCKETQUAT:
            x[7:11] /= np.linalg.norm(x[7:11])
        out[i] = x
    return out


def ulp_perturb(rng):
    def f(A, B):
        return A * (1.0 + np.finfo(float).eps * rng.choice([-1.0, 1.0], A.shape)), B * (1.0 + np.finfo(float).eps * rng.choice([-1.0, 1.0], B.shape))

    return f


def generate(name, spec, seed):
    model, par, cases, q, r, disp = spec
    rng = np.random.default_rng(seed)
    out = dict(par=par, q=q, r=r, time_step=np.array(TIME_STEP))
    for hold in ("foh", "zoh"):
        sel = [c for c in cases if c["foh"] == (hold == "foh")]
        if not sel:
            continue
        X = np.stack([integrate(model, par, c["x0"], c["U"], c["t"], c["foh"]) for c in sel])
        U = np.stack([c["U"] for c in sel])
        t = np.array([c["t"] for c in sel])
        n, K = X.shape[0], X.shape[1]
        Gs, Gr = np.zeros((n, K, U.shape[2], X.shape[2])), np.zeros((n, K, U.shape[2], X.shape[2]))
        it, gap = np.zeros((n, K), dtype=np.int32), np.zeros((n, K))
        same = within = 0
        for b in range(n):
            Gr[b], it[b], st = ref.tracker_gains(model, X[b], U[b], par, q, r)
            assert (st == 0).all(), (name, hold, b, st)
            _, it2, st2 = ref.tracker_gains(model, X[b], U[b], par, q, r, perturb=ulp_perturb(rng))
            assert (st2 == 0).all()
            same += int((it2 == it[b]).sum())
            within += int((np.abs(it2 - it[b]) <= 1).sum())
            for k in range(K):
                Gs[b, k] = ref.scipy_gain(model, X[b, k], U[b, ref.input_index(k, K, U.shape[1])], par, q, r)
                gap[b, k] = np.abs(Gr[b, k] - Gs[b, k]).max() / np.abs(Gs[b, k]).max()
        assert gap.max() < 1e-5, (name, hold, gap.max())
        assert same >= 0.95 * n * K and within == n * K, (name, hold, same, within, n * K)
        print(f"{name} {hold}: {n} x {K} nodes, iterations {it.min()}..{it.max()}, restatement vs scipy gap max {gap.max():.2e}, "
              f"1-ulp copy: {same}/{n * K} equal counts")
        # tracking margins (trajectory 0 of the hold), scipy gains
        xs = starts(model, X[0, 0], disp, rng)
        xf = X[0, -1]
        zero = np.zeros_like(Gs[0])
        e_open, e_closed = np.zeros(N_STARTS), np.zeros(N_STARTS)
        for i in range(N_STARTS):
            e_open[i] = ref.track(model, par, X[0], U[0], zero, t[0], xs[i], xf, TIME_STEP)["err1"]
            e_closed[i] = ref.track(model, par, X[0], U[0], Gs[0], t[0], xs[i], xf, TIME_STEP)["err1"]
        # how far the restatement's own result moves under the one integration variant available (every plant step as two oracle_simulate
        # calls of half the time step): the tests' 1e-9 max|x| bar on the device loop stands only while this is below it
        shift = 0.0
        for i in range(4):
            a, b2 = (ref.track(model, par, X[0], U[0], Gs[0], t[0], xs[i], xf, TIME_STEP, halves=h) for h in (1, 2))
            assert a["steps"] == b2["steps"]
            shift = max(shift, float(np.abs(a["x"] - b2["x"]).max() / np.abs(a["x"]).max()))
        assert shift < 1e-9, (name, hold, shift)
        print(f"   half-step variant moves the restatement's final x by {shift:.2e} of max|x|")
        und = ref.track(model, par, X[0], U[0], Gs[0], t[0], X[0, 0], xf, TIME_STEP)
        print(f"   open loop {np.round(e_open, 2)}\n   tracked   {np.round(e_closed, 3)}\n   undisturbed: max |x - x_ref| {und['max_dev']:.3e}, final {und['err1']:.3e}")
        assert (e_closed <= 0.25 * e_open).all(), (name, hold, e_closed / e_open)
        out.update({f"{hold}_X": X, f"{hold}_U": U, f"{hold}_t": t, f"{hold}_G_scipy": Gs, f"{hold}_G_ref": Gr, f"{hold}_it_ref": it,
                    f"{hold}_gap": gap, f"{hold}_starts": xs, f"{hold}_err_open": e_open, f"{hold}_err_closed": e_closed,
                    f"{hold}_undisturbed_max_dev": np.array(und["max_dev"]), f"{hold}_half_step_shift": np.array(shift)})
    path = os.path.join(HERE, f"lqr_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    which = sys.argv[1:] or ["rocket2d", "lander3dof", "rocketquat"]
    specs = dict(rocket2d=(rocket2d_cases, 1), lander3dof=(lander3dof_cases, 2), rocketquat=(rocketquat_cases, 3))
    for w in which:
        generate(w, specs[w][0](), specs[w][1])

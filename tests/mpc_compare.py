"""Shared checker of the linear MPC solve (csrc/mpc_kernel.h) against the condensed twin (oracle/mpc.hpp, kind 1), per input column.

Thrust is in newtons (1e4 .. 4.2e5) and the gimbal angle in radians (<= 0.26): one bar over both columns at once lets a gimbal error
of 0.4 % of its range through.  Here every quantity has its own scale (gimbal_max, T_max, the twin's two epigraph costs) and its own bar,
and the bar is MEASURED ON THE TWIN ALONE: the rounding floor of a row is the largest change of the twin's answer when x_init is scaled by
1 + 1e-15 N(0, 1) (FLOOR_DRAWS draws, fixed seed), the bar is BAR_FACTOR x that floor and never below BAR_MIN of the scale.  Why 100: the
kernel differs from the twin in the rounding of every operation (FMA contraction, summation trees, shared reciprocals), not only in its
input.  A row whose bar would exceed BAR_MAX is too ill-determined to compare (a flat face of the cost); it keeps its status and iteration
assertions and the caller caps how many rows may be left out."""
import os
import shutil

import numpy as np

HORIZONS = (3, 4, 5, 6, 7, 8)
FLOOR_DRAWS, FLOOR_SEED = 4, 20261018
BAR_FACTOR, BAR_MIN, BAR_MAX = 100.0, 1e-12, 1e-5
COLUMNS = ("gimbal", "thrust", "input_cost", "error_cost")
K_LINE = "K                           7"
WEIGHT_LINE = "input_weights              { scaling 0.1 (0) 1. (1) 1. }"
# thrust a thousand times cheaper than in the shipped file: the optimum brakes (thrust at T_max on some stages, strictly interior on
# others) instead of idling at T_min
BRAKING_WEIGHT_LINE = "input_weights              { scaling 0.1 (0) 1. (1) 1e-3 }"


def write_config(root, src_folder, K, braking=False):
    """a configuration root (root/Rocket2D/{model,MPC}.info) with the project's own files, K replaced and, for the braking variant, the
    input weights; scpp_amd.Rocket2D(root) and oracle.MPC(root) read the same folder"""
    cfg = os.path.join(str(root), "Rocket2D")
    os.makedirs(cfg, exist_ok=True)
    for f in ("model.info", "MPC.info"):
        shutil.copy(os.path.join(src_folder, f), os.path.join(cfg, f))
    with open(os.path.join(cfg, "MPC.info")) as fh:
        txt = fh.read()
    assert txt.count(K_LINE) == 1 and txt.count(WEIGHT_LINE) == 1
    txt = txt.replace(K_LINE, K_LINE[:-1] + str(K))
    if braking:
        txt = txt.replace(WEIGHT_LINE, BRAKING_WEIGHT_LINE)
    with open(os.path.join(cfg, "MPC.info"), "w") as fh:
        fh.write(txt)
    return str(root)


def _quantities(r, scale):
    """the four compared quantities of one twin solve, each over its scale: per-column worst stage of U, and the two costs"""
    return r["U"] / scale, np.array([r["input_cost"], r["error_cost"]])


def twin_reference(o, x0, xf, p):
    """The twin's answer for every row and, measured on the twin alone, floor [B][4], bar [B][4] and the rows kept for the comparison.
    x0, xf [B][6]; p the model's parameters.  The dictionary is shared between tests and backends: nobody writes to it."""
    B = x0.shape[0]
    xf = np.broadcast_to(np.asarray(xf, dtype=np.float64), x0.shape)
    scale = np.array([p.gimbal_max, p.T_max])
    rng = np.random.default_rng(FLOOR_SEED)
    rows = [o.solve(x0[b], xf[b], kind=1) for b in range(B)]
    ref = dict(
        status=np.array([r["status"] for r in rows]), iters=np.array([r["iters"] for r in rows]),
        U=np.array([r["U"] for r in rows]), X=np.array([r["X"] for r in rows]),
        cost=np.array([[r["input_cost"], r["error_cost"]] for r in rows]),
        term=np.array([[r["pres"], r["dres"], r["gap"], r["gap"] / max(abs(r["pcost"]), 1e-300)] for r in rows]),
        x0=x0.copy(), xf=xf.copy(), scale=scale)
    floor = np.zeros((B, 4))
    moved = 0  # perturbed solves whose status or iteration count differs from the unperturbed one
    for b in range(B):
        if rows[b]["status"] < 0:
            floor[b] = np.nan
            continue
        u, c = _quantities(rows[b], scale)
        for _ in range(FLOOR_DRAWS):
            q = o.solve(x0[b] * (1.0 + 1e-15 * rng.standard_normal(6)), xf[b], kind=1)
            moved += q["status"] != rows[b]["status"] or q["iters"] != rows[b]["iters"]
            if q["status"] < 0:
                floor[b] = np.inf
                continue
            uq, cq = _quantities(q, scale)
            floor[b, :2] = np.maximum(floor[b, :2], np.abs(uq - u).max(axis=0))
            floor[b, 2:] = np.maximum(floor[b, 2:], np.abs(cq - c) / c)
    ref["floor"], ref["moved"] = floor, moved
    ref["bar"] = np.maximum(BAR_FACTOR * floor, BAR_MIN)
    ref["solved"] = ref["status"] >= 0
    with np.errstate(invalid="ignore"):
        ref["kept"] = ref["solved"] & (ref["bar"] <= BAR_MAX).all(axis=1)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def rollout(A, Bm, z, x0, U):
    """X [B][K][6] of x+ = A x + B u + z under U [B][K-1][2]"""
    X = [np.asarray(x0, dtype=np.float64)]
    for k in range(U.shape[1]):
        X.append(X[-1] @ A.T + U[:, k] @ Bm.T + z)
    return np.stack(X, axis=1)


def check_against_twin(out, ref, alg, label, max_left_out, rows=None):
    """out: MPCAlgorithm.getSolution() of the rows of ref (rows: a mask of the rows to look at, default all).  Status and iteration count
    equal the twin's on every row the twin solves; U per column, both costs, X (against the roll-out of the returned U and against the
    twin's X) on the kept rows; the epigraph costs against the norms they bound on every solved row.  Prints floor, bar and measured gap
    per quantity; returns the gaps [B][4]."""
    rows = np.ones(len(ref["status"]), dtype=bool) if rows is None else np.asarray(rows, dtype=bool)
    solved, kept, bar, scale = ref["solved"] & rows, ref["kept"] & rows, ref["bar"], ref["scale"]
    assert np.array_equal(out["status"][solved], ref["status"][solved]), (label, out["status"], ref["status"])
    assert np.array_equal(out["iters"][solved], ref["iters"][solved]), (label, out["iters"], ref["iters"])
    assert (out["status"][rows & ~ref["solved"]] < 0).all()
    left_out = int((solved & ~kept).sum())
    assert left_out <= max_left_out, (label, left_out, np.nanmax(bar, axis=0))
    gap = np.zeros(bar.shape)
    gap[:, :2] = np.abs(out["U"] - ref["U"]).max(axis=1) / scale
    with np.errstate(invalid="ignore", divide="ignore"):
        gap[:, 2:] = np.abs(out["cost"] - ref["cost"]) / ref["cost"]
    if kept.any():
        for j, name in enumerate(COLUMNS):
            print(f"{label} {name:10s} rows {int(kept.sum()):3d}/{len(kept)} iters {ref['iters'][kept].min()}..{ref['iters'][kept].max()} "
                  f"floor {ref['floor'][kept, j].max():.1e} bar {bar[kept, j].min():.1e}..{bar[kept, j].max():.1e} "
                  f"gap {gap[kept, j].max():.1e} gap/bar {(gap[kept, j] / bar[kept, j]).max():.2f}")
        worst = gap[kept] / bar[kept]
        assert (gap[kept] <= bar[kept]).all(), (label, "gap over bar by", worst.max(), "row, column", np.argwhere(worst > 1.0).tolist())
    # ---- the states: what the kernel returns is the roll-out of the inputs it returns (condensed sums against the step-by-step recursion,
    # a few dozen FP64 products of magnitude <= |X|: 1e-9 of the largest state is four orders above their rounding)
    X, U = out["X"][solved], out["U"][solved]
    if solved.any():
        xs = max(1.0, np.abs(ref["X"][solved]).max())
        assert np.abs(X - rollout(alg.A, alg.B, alg.z, ref["x0"][solved], U)).max() <= 1e-9 * xs, label
    # ... and the twin's, within what the input bars allow: |dx+| <= |A| |dx| + |B| bar_u
    aA, aB = np.abs(alg.A), np.abs(alg.B)
    for b in np.flatnonzero(kept):
        e = np.zeros(6)
        for k in range(out["U"].shape[1]):
            e = aA @ e + aB @ (bar[b, :2] * scale)
            assert (np.abs(out["X"][b, k + 1] - ref["X"][b, k + 1]) <= e + 1e-9 * xs).all(), (label, b, k)
    # ---- the epigraph variables are tight at the optimum: 1e-6 of the row's cost (the bar of test_gpu_mpc_large_batch_properties), 1e-4 after
    # the reduced-accuracy exit (its feasibility tolerance, as in tests/test_oracle_mpc.py)
    if solved.any():
        ic = np.linalg.norm((alg.input_weights * U).reshape(len(U), -1), axis=1)
        ec = np.linalg.norm(alg.state_weights_terminal * (X[:, -1] - ref["xf"][solved]), axis=1)
        tol = np.where(ref["status"][solved] == 0, 1e-6, 1e-4) * ref["cost"][solved].sum(axis=1)
        c = out["cost"][solved]
        assert (np.abs(c[:, 0] - ic) <= tol).all() and (np.abs(c[:, 1] - ec) <= tol).all(), (label, np.abs(c[:, 0] - ic).max(), np.abs(c[:, 1] - ec).max())
    return gap


def check_constraints(out, rows, p, tol=1e-6):
    """every returned plan satisfies the reference problem's box, glide-slope and rate constraints (rocket2d.cpp:62-83): the assertions
    of test_gpu_mpc_large_batch_properties"""
    X, U = out["X"][rows], out["U"][rows]
    assert (np.abs(U[:, :, 0]) <= p.gimbal_max * (1 + tol)).all()
    assert (U[:, :, 1] >= p.T_min * (1 - tol)).all() and (U[:, :, 1] <= p.T_max * (1 + tol)).all()
    assert (np.abs(X[:, :, 4]) <= p.theta_max + 1e-7).all() and (np.abs(X[:, :, 5]) <= p.w_B_max + 1e-7).all()
    assert (np.abs(X[:, 1:, 0]) <= p.tan_gamma_gs * X[:, 1:, 1] + 1e-5).all()

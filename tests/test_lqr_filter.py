"""Filter sweep (scpp_hip_lqr_set_measurement / _filter / _download_filter, scpp_amd/csrc/lqr/lqr_filter_kernel.h): every test with the
`lqr_lib` fixture runs the SAME assertions on the CPU emulation of the kernel sources (`emu`) and, marked gpu, on the device library (`hip`).

Checkers (tests/lqr_filter_reference.py, no code shared with the kernels): the exact answer (DOP853, rtol 1e-12, stored by
tests/golden/generate_lqr_filter_goldens.py), the twin (numpy fixed-step RKF78 of the same definition on the oracle's Jacobians, run here)
and the 2 nx x 2 nx joint system of (e, eps).  Inputs: tests/golden/lqr_<model>.npz, lqr_riccati_<model>.npz, lqr_covariance_<model>.npz
(sigma0, w), all read only, and lqr_filter_<model>.npz (H, v, the exact answers and the measured gaps).

Bars, all read from the fixture: device vs twin 10 x gap_round (the twin against a copy of itself with Jacobians perturbed by 1 ulp);
device vs exact gap_scheme + that.  Units: lqr_filter_reference.gaps (scaled_gap for the matrices)."""
import ctypes
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import lqr_filter_reference as fr
from lqr_filter_reference import CASES as GOLDEN_CASES, QUANTITIES, gaps

MODELS = {"rocketquat": 0, "rocket2d": 1, "lander3dof": 2}
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
E_ARG, E_STATE = -1, -4
OUT = dict(Sg="error_cov", Xh="estimate_cov", L="L", I="input_cov")
ARRAYS = ("L", "error_std", "final_error_cov", "error_cov", "state_std", "input_cov", "final_state_cov", "estimate_cov")


@pytest.fixture(scope="module", params=BACKENDS)
def backend(request):
    import __graft_entry__ as g

    g.build_oracle()
    if request.param == "emu":
        return request.param, g.build_lqr_emu()
    lib = os.environ.get("SCPP_LQR_LIBRARY") or g.LQR_LIB
    if not os.path.exists(lib):
        g.build_lqr()
    return request.param, lib


@pytest.fixture(scope="module")
def lqr_lib(backend):
    return backend[1]


def goldens(name):
    """(trajectories and frozen-time gains, finite-horizon gains, covariance fixture, filter fixture)"""
    return tuple(np.load(os.path.join(GOLDEN, f"lqr_{pre}{name}.npz")) for pre in ("", "riccati_", "covariance_", "filter_"))


def unpack(tri, nx):
    iu = np.triu_indices(nx)
    S = np.zeros(tri.shape[:-1] + (nx, nx))
    S[..., iu[0], iu[1]] = tri
    S[..., iu[1], iu[0]] = tri
    return S


def context(lib, name, d, hold, X=None, U=None, t=None, G=None):
    from scpp_amd import _lib

    X = d[f"{hold}_X"] if X is None else X
    U = d[f"{hold}_U"] if U is None else U
    t = d[f"{hold}_t"] if t is None else t
    c = _lib.LqrContext(MODELS[name], X.shape[1], X.shape[0], hold == "foh", 0, lib)
    c.set_weights(d["q"], d["r"])
    c.set_flow_params(d["par"])
    c.set_trajectories(X, U, t)
    if G is not None:
        c.set_gains(G)
    return c


def sweep(c, S0, w, H, v, steps, loop=True, keep=True):
    c.set_covariance_inputs(S0, w)
    c.set_measurement(H, v)
    n_ok = c.filter(steps, loop, keep)
    o = c.download_filter(loop, keep)
    o["n_ok"] = n_ok
    return o


def run(lib, name, d, hold, G, S0, w, H, v, steps, loop=True, keep=True, **kw):
    c = context(lib, name, d, hold, G=G, **kw)
    o = sweep(c, S0, w, H, v, steps, loop, keep)
    c.close()
    return o


def as_result(o, b):
    """trajectory b of a downloaded sweep in the reference's names"""
    return {k: o[v][b] for k, v in OUT.items()}


def check_against(o, b, ref, H, v, bars, what):
    g = gaps(as_result(o, b), ref, H, v)
    sd = np.sqrt(np.diagonal(ref["Sg"] + ref["Xh"], axis1=1, axis2=2))
    g["sd"] = float((np.abs(o["state_std"][b] - sd) / sd.max(axis=0)[None, :]).max())
    print(f"{what}: " + ", ".join(f"{q} {g[q]:.2e} (bar {bars[q]:.2e})" for q in QUANTITIES))
    for q in QUANTITIES:
        assert g[q] <= bars[q], (what, q, g[q], bars[q])


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold,law,wc", GOLDEN_CASES)
@pytest.mark.parametrize("name", list(MODELS))
def test_filter_against_twin_and_exact(lqr_lib, name, hold, law, wc):
    """Sg, L, Xh, state_std and G Xh G' of every node vs the twin (bar 10 x gap_round) and vs the exact answer (bar gap_scheme + that); status
    0, n_ok = B, the final arrays are those of the kept last node.  The generator asserts gap_scheme <= 1e-10 and that a twin with ONE tableau
    entry's sign flipped misses the second bar on Sg by a factor >= 100."""
    d, rg, cg, fg = goldens(name)
    steps, H, v = int(fg["steps"]), fg["H"], fg["v"]
    X, U, t = d[f"{hold}_X"], d[f"{hold}_U"], d[f"{hold}_t"]
    G = d[f"{hold}_G_ref"] if law == "frozen" else rg[f"{hold}_G_exact"]
    w = cg["w"] if wc == "w1" else None
    B, nx = X.shape[0], X.shape[2]
    tag = f"{hold}_{law}_{wc}"
    o = run(lqr_lib, name, d, hold, G, cg["sigma0"], w, H, v, steps)
    assert all(np.isfinite(o[k]).all() for k in ARRAYS)
    for b in range(B):
        tw = fr.twin(MODELS[name], d["par"], X[b], U[b], float(t[b]), G[b], cg["sigma0"], w, H, v, steps=steps)
        Sg, Xh = unpack(fg[f"{tag}_Sg_exact"][b], nx), unpack(fg[f"{tag}_Xh_exact"][b], nx)
        ex = dict(Sg=Sg, Xh=Xh, L=fr.gain(Sg, H, v), I=fg[f"{tag}_I_exact"][b])
        rb = {q: 10.0 * float(fg[f"{tag}_gap_round_{q}"][b]) for q in QUANTITIES}
        check_against(o, b, tw, H, v, rb, f"{name} {tag} {b} vs twin")
        check_against(o, b, ex, H, v, {q: float(fg[f"{tag}_gap_scheme_{q}"][b]) + rb[q] for q in QUANTITIES}, f"{name} {tag} {b} vs exact")
        assert float(fg[f"{tag}_gap_scheme_Sg"][b]) <= 1e-10
    assert (o["status"] == 0).all() and o["n_ok"] == B
    assert (o["final_error_cov"] == o["error_cov"][:, -1]).all()
    assert (o["final_state_cov"] == o["error_cov"][:, -1] + o["estimate_cov"][:, -1]).all()


@pytest.mark.parametrize("name", list(MODELS))
def test_joint_system_has_the_covariance_the_sweep_claims(name):
    """CPU only, the reference alone: Cov(e) of the 2 nx x 2 nx joint Lyapunov equation of (e, eps) equals Sg + Xh of `exact` to 1e-9 of its
    largest entry (one case here; every fixture trajectory in the generator, whose stored figures are read)"""
    d, rg, cg, fg = goldens(name)
    for hold, law, wc in GOLDEN_CASES:
        assert (fg[f"{hold}_{law}_{wc}_joint_gap"] <= 1e-9).all()
    X, U, t, G = d["zoh_X"][0], d["zoh_U"][0], float(d["zoh_t"][0]), rg["zoh_G_exact"][0]
    nx = X.shape[1]
    J = fr.joint_exact(MODELS[name], d["par"], X, U, t, G, cg["sigma0"], cg["w"], fg["H"], fg["v"])
    P = unpack(fg["zoh_riccati_w1_Sg_exact"][0], nx) + unpack(fg["zoh_riccati_w1_Xh_exact"][0], nx)
    gap = fr.rel_gap(J, P)
    print(f"{name}: joint system vs Sg + Xh {gap:.2e}")
    assert gap <= 1e-9


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,key", [("lander3dof", "dense"), ("rocket2d", "ny1"), ("rocket2d", "nyI"), ("rocket2d", "ny16")])
def test_other_measurements_against_the_twin(lqr_lib, name, key):
    """a dense 5 x 7 H (no symmetry a transposed operand could hide behind), ny = 1 (the first chunk alone), ny = nx (H = I) and ny = 16 (the
    last row of the last chunk; repeated rows with different v): every output vs the twin, bar 10 x gap_round"""
    d, rg, cg, fg = goldens(name)
    H, v, steps = fg[f"{key}_H"], fg[f"{key}_v"], int(fg["steps"])
    X, U, t, G = d["foh_X"], d["foh_U"], d["foh_t"], rg["foh_G_exact"]
    o = run(lqr_lib, name, d, "foh", G, cg["sigma0"], cg["w"], H, v, steps)
    assert (o["status"] == 0).all() and o["L"].shape[-1] == H.shape[0]
    for b in range(X.shape[0]):
        tw = fr.twin(MODELS[name], d["par"], X[b], U[b], float(t[b]), G[b], cg["sigma0"], cg["w"], H, v, steps=steps)
        check_against(o, b, tw, H, v, {q: 10.0 * float(fg[f"{key}_gap_round_{q}"][b]) for q in QUANTITIES}, f"{name} {key} {b} vs twin")


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hold", [("rocketquat", "foh"), ("rocket2d", "zoh"), ("lander3dof", "foh")])
def test_structure(lqr_lib, name, hold):
    """bitwise: Sg and Xh symmetric; Sg, L and error_std identical with closed_loop on and off; node 0 is (sigma0, 0); with H = 0 (ny = 1) Sg
    equals covariance() under zero gains, L = 0 and Xh = 0; error_std and state_std are the square roots of the kept diagonals; L equals
    Sg H' V^-1 of the kept Sg within 4 ulp of the row's largest term"""
    d, rg, cg, fg = goldens(name)
    steps, H, v = int(fg["steps"]), fg["H"], fg["v"]
    G, S0, w = rg[f"{hold}_G_exact"], cg["sigma0"], cg["w"]
    nx = S0.shape[0]
    c = context(lqr_lib, name, d, hold, G=G)
    o = sweep(c, S0, w, H, v, steps)
    f = sweep(c, S0, w, H, v, steps, loop=False)
    Sg, Xh = o["error_cov"], o["estimate_cov"]
    assert (Sg == Sg.transpose(0, 1, 3, 2)).all() and (Xh == Xh.transpose(0, 1, 3, 2)).all()
    assert set(f) == {"L", "error_std", "final_error_cov", "status", "error_cov", "n_ok"}
    for k in ("L", "error_std", "final_error_cov", "status", "error_cov"):
        assert (f[k] == o[k]).all(), k
    assert (Sg[:, 0] == S0).all() and (Xh[:, 0] == 0).all() and np.abs(Xh[:, -1]).max() > 0
    dg, dp = np.diagonal(Sg, axis1=2, axis2=3), np.diagonal(Sg + Xh, axis1=2, axis2=3)
    assert (dg >= 0).all() and (dp >= 0).all()
    assert (o["error_std"] == np.sqrt(dg)).all() and (o["state_std"] == np.sqrt(dp)).all()
    terms = np.abs(Sg[:, :, :, None, :] * H[None, None, None, :, :]).max(axis=-1) / v  # [B][K][nx][ny]: the largest term of each sum
    Lr = np.einsum("bkij,mj->bkim", Sg, H) / v
    assert (np.abs(o["L"] - Lr) <= 4 * np.finfo(float).eps * terms).all()
    # H = 0: the open loop, and nothing to estimate with
    c.set_gains(np.zeros_like(G))
    z = sweep(c, S0, w, np.zeros((1, nx)), [1.0], steps)
    c.set_covariance_inputs(S0, w)
    c.propagate_covariance(steps, True)
    cv = c.download_covariance(True)
    c.close()
    assert (z["error_cov"] == cv["cov"]).all() and (z["error_std"] == cv["state_std"]).all() and (z["final_error_cov"] == cv["final_cov"]).all()
    assert (z["L"] == 0).all() and (z["estimate_cov"] == 0).all() and (z["input_cov"] == 0).all() and (z["state_std"] == cv["state_std"]).all()
    assert (z["status"] == 0).all() and not (z["error_cov"][:, -1] == Sg[:, -1]).all()


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------
class DeviceBuffers:
    """copies of `arrays` the library can read as device memory, owned by the test: on the emulator the numpy arrays themselves, on the device
    hipMalloc + hipMemcpy of the HIP runtime the LQR library is linked against, reached through the library's own handle"""

    def __init__(self, backend_name, lib, arrays):
        from scpp_amd import _lib

        self.host = [np.array(a, dtype=np.float64, order="C") for a in arrays]
        self.rt, self.ptrs = None, []
        if backend_name == "emu":
            self.ptrs = [a.ctypes.data for a in self.host]
            return
        C = ctypes
        self.rt = _lib.load_lqr_library(lib)
        self.rt.hipMalloc.argtypes, self.rt.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
        self.rt.hipMemcpy.argtypes, self.rt.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
        self.rt.hipFree.argtypes, self.rt.hipFree.restype = [C.c_void_p], C.c_int
        for a in self.host:
            p = C.c_void_p()
            assert self.rt.hipMalloc(C.byref(p), a.nbytes) == 0 and p.value
            self.ptrs.append(p.value)
            assert self.rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice

    def free(self):
        if self.rt is not None:
            for p in self.ptrs:
                assert self.rt.hipFree(p) == 0
        self.ptrs = []


def short(d, rg, hold, Ks):
    """the first Ks nodes of every golden trajectory as trajectories of their own (flight time scaled to the same dt), with the golden gains"""
    X, U, t, G = d[f"{hold}_X"], d[f"{hold}_U"], d[f"{hold}_t"], rg[f"{hold}_G_exact"]
    nU = Ks if hold == "foh" else Ks - 1
    return (np.ascontiguousarray(X[:, :Ks]), np.ascontiguousarray(U[:, :nU]), t * (Ks - 1) / (X.shape[1] - 1), np.ascontiguousarray(G[:, :Ks]))


def twin_floor(model, par, X, U, T, G, S0, w, H, v, steps, seed):
    """the twin of one short trajectory and its rounding floor, measured here as the generator measures it (the largest of 5 draws, and
    never below one ulp: after one or two steps a draw can leave a quantity untouched, and no computed quantity can be held to less)"""
    rng = np.random.default_rng(seed)
    tw = fr.twin(model, par, X, U, T, G, S0, w, H, v, steps=steps)
    floor = {q: fr.EPS for q in QUANTITIES}
    for _ in range(5):
        for q, val in gaps(fr.perturbed_twin(model, par, X, U, T, G, S0, w, H, v, steps, rng), tw, H, v).items():
            floor[q] = max(floor[q], val)
    return tw, floor


@pytest.mark.parametrize("name,hold,Ks,steps", [("rocket2d", "foh", 2, 1), ("rocketquat", "zoh", 3, 1), ("lander3dof", "zoh", 2, 5), ("rocket2d", "zoh", 3, 2)])
def test_short_horizons(lqr_lib, name, hold, Ks, steps):
    """K = 2 and K = 3 cut from the goldens, down to one step per segment: every output vs the twin, bar 10 x the floor measured here"""
    d, rg, cg, fg = goldens(name)
    X, U, t, G = short(d, rg, hold, Ks)
    H, v = fg["H"], fg["v"]
    o = run(lqr_lib, name, d, hold, G, cg["sigma0"], cg["w"], H, v, steps, X=X, U=U, t=t)
    assert (o["status"] == 0).all() and o["n_ok"] == X.shape[0]
    for b in range(X.shape[0]):
        tw, floor = twin_floor(MODELS[name], d["par"], X[b], U[b], float(t[b]), G[b], cg["sigma0"], cg["w"], H, v, steps, 7 + b)
        check_against(o, b, tw, H, v, {q: 10.0 * floor[q] for q in QUANTITIES}, f"{name} {hold} K={Ks} steps={steps} {b} vs twin")


def test_zero_order_hold_buffer_with_more_rows_than_inputs(backend):
    """U in a device buffer [B][K + 2][nu] of which K - 1 rows per trajectory are inputs and the rest NaN, handed over by
    scpp_hip_lqr_set_trajectories_device: bitwise the upload path's result (the kernel strides U by u_rows and reads no row past nU)"""
    kind, lib = backend
    d, rg, cg, fg = goldens("rocket2d")
    X, U, t, G = short(d, rg, "zoh", 4)
    B, K, nu = X.shape[0], X.shape[1], U.shape[2]
    ref = run(lib, "rocket2d", d, "zoh", G, cg["sigma0"], cg["w"], fg["H"], fg["v"], 2, X=X, U=U, t=t)
    Up = np.full((B, K + 2, nu), np.nan)
    Up[:, :K - 1] = U
    bufs = DeviceBuffers(kind, lib, [X, Up, t])
    c = context(lib, "rocket2d", d, "zoh", X=X, U=U, t=t)
    c.set_trajectories_device(*bufs.ptrs, B, K + 2)
    c.set_gains(G)
    o = sweep(c, cg["sigma0"], cg["w"], fg["H"], fg["v"], 2)
    c.close()
    bufs.free()
    assert (o["status"] == 0).all()
    for k in ARRAYS:
        assert (o[k] == ref[k]).all(), k


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------
def test_batch_independence(lqr_lib):
    """B = 5 with differing T and per-trajectory sigma0, a NaN state in trajectory 2: trajectories 0, 1, 3, 4 are bitwise what each gives
    alone; trajectory 2 has SCPP_LQR_NONFINITE and zeros everywhere"""
    d, rg, cg, fg = goldens("rocket2d")
    idx = [0, 1, 0, 1, 0]
    X, U, G = d["foh_X"][idx].copy(), d["foh_U"][idx], rg["foh_G_exact"][idx]
    t = d["foh_t"][idx] * np.array([1.0, 0.9, 1.0, 1.1, 0.8])
    S0 = np.stack([cg["sigma0"] * s for s in (1.0, 0.5, 1.0, 0.25, 2.0)])
    X[2, 7, 3] = np.nan
    H, v, w = fg["H"], 2.0 * fg["v"], cg["w"]
    o = run(lqr_lib, "rocket2d", d, "foh", G, S0, w, H, v, 5, X=X, U=U, t=t)
    assert o["status"].tolist() == [0, 0, -2, 0, 0] and o["n_ok"] == 4
    for b in range(5):
        if b == 2:
            assert all((o[k][b] == 0).all() for k in ARRAYS)
            continue
        a = run(lqr_lib, "rocket2d", d, "foh", G[b:b + 1], S0[b], w, H, v, 5, X=X[b:b + 1], U=U[b:b + 1], t=t[b:b + 1])
        for k in ARRAYS:
            assert np.isfinite(o[k][b]).all() and (o[k][b] == a[k][0]).all(), (b, k)
    assert not (o["error_cov"][0] == o["error_cov"][4]).all()


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------------
def test_overflow_is_reported_from_its_segment_on(lqr_lib):
    """v = 1e-300.  Trajectory 1 starts from the golden sigma0: Sg H' V^-1 H Sg overflows inside the first segment; node 0 is intact (Sg =
    sigma0, a finite L), node 1 and every later one and the final matrices are zeros, SCPP_LQR_NONFINITE, nothing non-finite is written.
    Trajectory 0 starts from sigma0 scaled (by a power of two) so that h rho <= 1/8 even under that v, with W = 0: it is unaffected -- status
    0, finite, and bitwise what it gives alone."""
    d, rg, cg, fg = goldens("rocket2d")
    X, U, t, G = d["foh_X"], d["foh_U"], d["foh_t"], rg["foh_G_exact"]
    H, S0, K = fg["H"], cg["sigma0"], X.shape[1]
    v = np.full(H.shape[0], 1e-300)
    h = float(t.max()) / (K - 1) / 5
    s = 2.0 ** np.floor(np.log2(1e-300 / (8.0 * h * np.einsum("mi,ij,mj->m", H, S0, H).max())))
    S2 = np.stack([s * S0, S0])
    assert fr.auto_steps(S2[0], H, v, 5 * h)[0] == 5
    o = run(lqr_lib, "rocket2d", d, "foh", G, S2, None, H, v, 5)
    alone = run(lqr_lib, "rocket2d", d, "foh", G[:1], S2[0], None, H, v, 5, X=X[:1], U=U[:1], t=t[:1])
    assert o["status"].tolist() == [0, -2] and o["n_ok"] == 1
    for k in ARRAYS:
        assert np.isfinite(o[k]).all(), k
        assert (o[k][0] == alone[k][0]).all(), k
        assert (o[k][1][1:] == 0).all() if o[k].ndim > 3 or k.endswith("_std") else (o[k][1] == 0).all(), k
    assert np.abs(o["error_cov"][0, -1]).max() > 0 and (o["error_cov"][1, 0] == S0).all() and np.abs(o["L"][1, 0]).max() > 1e290
    assert (o["error_std"][1, 0] > 0).all() and (o["state_std"][1, 0] == o["error_std"][1, 0]).all()


# ---- 7 -------------------------------------------------------------------------------------------------------------------------------------
def test_constant_system_reaches_the_algebraic_riccati_solution(lqr_lib):
    """Two-node constant trajectory at Rocket2D's operating point, the fixture's H and v, W = diag(w) > 0, horizon and step count from the
    generator: the final Sg vs scipy.linalg.solve_continuous_are(A', H', W, V).  The twin on the CPU is within stat_gap (stored by the
    generator, <= 1e-8); the device is held to the twin's bar, 1e-8"""
    import scipy.linalg

    import oracle_lib
    import scpp_amd
    from scpp_amd import _lib

    d, _, cg, fg = goldens("rocket2d")
    T, steps, gap = float(fg["stat_horizon"]), int(fg["stat_steps"]), float(fg["stat_gap"])
    H, v, w = fg["H"], fg["v"], cg["w"]
    m = scpp_amd.Rocket2D().loadParameters()
    x_eq, u_eq = (np.asarray(a, dtype=np.float64) for a in m.getOperatingPoint())
    c = _lib.LqrContext(1, 2, 1, True, 0, lqr_lib)
    c.set_flow_params(d["par"])
    c.set_trajectories(np.tile(x_eq, (1, 2, 1)), np.tile(u_eq, (1, 2, 1)), [T])
    o = sweep(c, cg["sigma0"], w, H, v, steps, loop=False, keep=False)
    c.close()
    _, A, _ = oracle_lib.flow(1, x_eq, u_eq, d["par"])
    Sa = scipy.linalg.solve_continuous_are(A.T, H.T, np.diag(w), np.diag(v))
    g = fr.rel_gap(o["final_error_cov"][0], Sa)
    print(f"stationary limit, horizon {T} s, {steps} steps: Sg(T) vs the algebraic Riccati solution {g:.2e} (twin {gap:.2e})")
    assert o["status"][0] == 0 and gap <= 1e-8
    assert g <= 1e-8


# ---- 8 -------------------------------------------------------------------------------------------------------------------------------------
def test_abi_errors(lqr_lib):
    from scpp_amd import _lib

    L = _lib.load_lqr_library(lqr_lib)
    d, rg, cg, fg = goldens("rocket2d")
    X, U, t = d["foh_X"], d["foh_U"], d["foh_t"]
    S0, w = np.ascontiguousarray(cg["sigma0"]), np.ascontiguousarray(cg["w"])
    H, v = np.ascontiguousarray(fg["H"]), np.ascontiguousarray(fg["v"])
    p = _lib._p
    n = ctypes.c_int()
    st = np.zeros(2, dtype=np.int32)
    c = _lib.LqrContext(1, 30, 2, True, 0, lqr_lib)

    def download(**kw):
        names = ("L", "error_std", "final_error_cov", "status", "error_cov", "state_std", "input_cov", "final_state_cov", "estimate_cov")
        return L.scpp_hip_lqr_download_filter(c.h, *[p(kw.get(k)) for k in names])

    with pytest.raises(_lib.ScppHipError):  # the binding before any measurement: the ABI's SCPP_E_STATE, as for every other download
        c.download_filter()
    assert L.scpp_hip_lqr_set_measurement(None, p(H), 3, p(v)) == E_ARG and L.scpp_hip_lqr_filter(None, 5, 0, 0, None) == E_ARG
    assert L.scpp_hip_lqr_download_filter(None, *[None] * 9) == E_ARG
    assert L.scpp_hip_lqr_set_measurement(c.h, p(H), 3, p(v)) == 0
    assert L.scpp_hip_lqr_filter(c.h, 5, 0, 0, ctypes.byref(n)) == E_STATE  # no trajectories
    c.set_trajectories(X, U, t)
    c.set_flow_params(d["par"])
    assert L.scpp_hip_lqr_filter(c.h, 5, 0, 0, ctypes.byref(n)) == E_STATE  # no covariance inputs
    c.set_covariance_inputs(S0, w)
    assert L.scpp_hip_lqr_set_measurement(c.h, None, 0, None) == 0
    assert L.scpp_hip_lqr_filter(c.h, 5, 0, 0, ctypes.byref(n)) == E_STATE  # the measurement was cleared
    for ny in (0, 17, -1):
        assert L.scpp_hip_lqr_set_measurement(c.h, p(np.zeros((17, 6))), ny, p(np.ones(17))) == E_ARG
    assert L.scpp_hip_lqr_set_measurement(c.h, p(H), 3, None) == E_ARG
    for bad in (np.nan, np.inf):
        Hb = H.copy()
        Hb[2, 4] = bad
        assert L.scpp_hip_lqr_set_measurement(c.h, p(Hb), 3, p(v)) == E_ARG
    for bad in (0.0, -1.0, np.nan, np.inf):
        vb = v.copy()
        vb[2] = bad
        assert L.scpp_hip_lqr_set_measurement(c.h, p(H), 3, p(vb)) == E_ARG
    assert L.scpp_hip_lqr_filter(c.h, 5, 0, 0, ctypes.byref(n)) == E_STATE  # the refused calls set nothing
    assert L.scpp_hip_lqr_set_measurement(c.h, p(H), 3, p(v)) == 0
    assert download(status=st) == E_STATE  # before a sweep
    for steps in (0, -2):
        assert L.scpp_hip_lqr_filter(c.h, steps, 0, 0, ctypes.byref(n)) == E_ARG
    assert L.scpp_hip_lqr_filter(c.h, 5, 1, 0, ctypes.byref(n)) == E_STATE  # closed_loop without gains
    assert L.scpp_hip_lqr_filter(c.h, 5, 0, 0, ctypes.byref(n)) == 0 and n.value == 2  # the filter alone needs none
    out = dict(L=np.zeros((2, 30, 6, 3)), error_std=np.zeros((2, 30, 6)), final_error_cov=np.zeros((2, 6, 6)), status=st)
    assert download(**out) == 0 and out["error_std"].min() > 0
    assert download() == 0  # any pointer may be NULL
    assert download(error_cov=np.zeros((2, 30, 6, 6))) == E_STATE  # swept without keep
    for k, shape in (("state_std", (2, 30, 6)), ("input_cov", (2, 30, 2, 2)), ("final_state_cov", (2, 6, 6)), ("estimate_cov", (2, 30, 6, 6))):
        assert download(**{k: np.zeros(shape)}) == E_STATE  # swept without closed_loop
    assert L.scpp_hip_lqr_filter(c.h, 5, 0, 1, None) == 0
    ec = np.zeros((2, 30, 6, 6))
    assert download(error_cov=ec) == 0 and (ec[:, 0] == S0).all()
    assert download(estimate_cov=np.zeros((2, 30, 6, 6))) == E_STATE
    c.compute_gains()
    assert L.scpp_hip_lqr_filter(c.h, 5, 1, 0, ctypes.byref(n)) == 0 and n.value == 2
    assert download(state_std=np.zeros((2, 30, 6)), input_cov=np.zeros((2, 30, 2, 2)), final_state_cov=np.zeros((2, 6, 6))) == 0
    assert download(estimate_cov=np.zeros((2, 30, 6, 6))) == E_STATE and download(error_cov=ec) == E_STATE  # closed_loop without keep
    # covariance inputs for another number of trajectories: refused at the sweep
    c3 = _lib.LqrContext(1, 30, 3, True, 0, lqr_lib)
    c3.set_flow_params(d["par"])
    c3.set_trajectories(X, U, t)
    c3.set_covariance_inputs(np.stack([S0, S0]), w)
    c3.set_measurement(H, v)
    c3.set_trajectories(np.tile(X[:1], (3, 1, 1)), np.tile(U[:1], (3, 1, 1)), np.tile(t[:1], 3))
    assert L.scpp_hip_lqr_filter(c3.h, 5, 0, 0, None) == E_STATE
    c3.close()
    c.close()


def test_what_invalidates_the_result(lqr_lib):
    """set_trajectories, set_flow_params, set_covariance_inputs and set_measurement always; whatever changes the gains only after a sweep
    with closed_loop"""
    from scpp_amd import _lib

    L = _lib.load_lqr_library(lqr_lib)
    d, rg, cg, fg = goldens("rocket2d")
    c = context(lqr_lib, "rocket2d", d, "foh")
    c.compute_gains()
    G = c.download_gains()["gains"]
    st = np.zeros(2, dtype=np.int32)

    def have():
        return L.scpp_hip_lqr_download_filter(c.h, None, None, None, _lib._p(st), None, None, None, None, None)

    always = [lambda: c.set_trajectories(d["foh_X"], d["foh_U"], d["foh_t"]), lambda: c.set_flow_params(d["par"]),
              lambda: c.set_covariance_inputs(cg["sigma0"], cg["w"]), lambda: c.set_measurement(fg["H"], fg["v"]), lambda: c.set_measurement(None)]
    gains = [lambda: c.set_gains(G), c.compute_gains, lambda: c.compute_gains_riccati(3), lambda: c.compute_gains_affine(3),
             lambda: c.compute_gains_discrete(3), lambda: c.set_weights(2 * d["q"], d["r"])]
    for loop in (True, False):
        for change in always + gains:
            c.set_weights(d["q"], d["r"])
            c.compute_gains()
            sweep(c, cg["sigma0"], cg["w"], fg["H"], fg["v"], 2, loop=loop, keep=False)
            assert have() == 0
            change()
            assert have() == (E_STATE if loop or change in always else 0), (loop, change)
    c.close()


def test_sweep_leaves_the_rest_of_the_context_alone(lqr_lib):
    """gains and their status, a previous covariance() and moments() result and a flight's outputs are bitwise the same with and without a
    filter sweep in between, and so is a flight after it"""
    d, _, cg, fg = goldens("rocketquat")
    X, U, t = d["foh_X"][0], d["foh_U"][0], float(d["foh_t"][0])
    xs = d["foh_starts"][:4]
    B = xs.shape[0]

    def fly(with_sweep):
        c = context(lqr_lib, "rocketquat", d, "foh", X=np.tile(X, (B, 1, 1)), U=np.tile(U, (B, 1, 1)), t=np.full(B, t))
        c.compute_gains()
        c.track(xs, X[-1], float(d["time_step"]), 20, 300)
        c.set_covariance_inputs(cg["sigma0"], cg["w"])
        c.propagate_moments(2, True)
        if with_sweep:
            c.set_measurement(fg["H"], fg["v"])
            assert c.filter(2, True, True) == B
        res = [c.download_gains(), c.track_download(), c.download_covariance(True), c.download_moments()]
        c.track(xs, X[-1], float(d["time_step"]), 20, 400)
        res.append(c.track_download())
        c.close()
        return res

    for u, v in zip(fly(False), fly(True)):
        for k in u:
            assert (u[k] == v[k]).all(), k


def test_gains_incomplete_is_reported(lqr_lib):
    """Q = I, R = I on Rocket2D at 5 steps: the explicit Riccati sweep fails every node but the last (zero gains, status -2 there).  The loop
    tile runs on those zeros and says so: SCPP_LQR_GAINS_INCOMPLETE; the filter alone does not read gains: status 0, the same Sg bitwise;
    with the same gains handed in by the user there is no gain status and the result is bitwise the same with status 0"""
    from scpp_amd import _lib

    d, _, cg, fg = goldens("rocket2d")
    c = context(lqr_lib, "rocket2d", d, "foh")
    c.set_weights(np.ones(6), np.ones(2))
    assert c.compute_gains_riccati(5) == 2
    g = c.download_gains()
    assert (g["status"][:, :-1] == -2).all()
    o = sweep(c, cg["sigma0"], cg["w"], fg["H"], fg["v"], 5)
    assert (o["status"] == _lib.LQR_GAINS_INCOMPLETE).all() and o["n_ok"] == 0 and np.isfinite(o["estimate_cov"]).all()
    f = sweep(c, cg["sigma0"], cg["w"], fg["H"], fg["v"], 5, loop=False)
    assert (f["status"] == 0).all() and f["n_ok"] == 2 and (f["error_cov"] == o["error_cov"]).all()
    c.set_gains(g["gains"])
    o2 = sweep(c, cg["sigma0"], cg["w"], fg["H"], fg["v"], 5)
    c.close()
    assert (o2["status"] == 0).all() and all((o2[k] == o[k]).all() for k in ARRAYS)


# ---- 9 -------------------------------------------------------------------------------------------------------------------------------------
def test_front_end_tracker(lqr_lib, tmp_path):
    """scpp_amd.LQRTracker.filter == the C ABI's arrays; H and v from LQR.info's optional measurement_std, absent from the shipped files;
    closed_loop=None means exactly when the tracker has gains; steps=None picks the documented count and refuses above 200"""
    import scpp_amd

    d, _, cg, fg = goldens("rocket2d")
    X, U, t = d["foh_X"], d["foh_U"], d["foh_t"]
    S0, w, H, v = cg["sigma0"], cg["w"], fg["H"], fg["v"]
    for m in (scpp_amd.Rocket2D(), scpp_amd.RocketQuat(), scpp_amd.Lander3dof()):
        assert scpp_amd.load_lqr_measurement(m.loadParameters()) == (None, None)
    cfg = tmp_path / "config"
    shutil.copytree(os.path.join(ROOT, "scpp_amd", "config"), cfg)
    sd = np.zeros(6)
    sd[[0, 1, 4]] = np.sqrt(v)
    with open(cfg / "Rocket2D" / "LQR.info", "a") as f:
        f.write("\nmeasurement_std\n{\n" + "".join(f"    ({i}) {s!r}\n" for i, s in enumerate(sd.tolist())) + "}\n")
    m = scpp_amd.Rocket2D(str(cfg)).loadParameters()
    Hf, vf = scpp_amd.load_lqr_measurement(m)
    assert (Hf == H).all() and (vf == np.sqrt(v) ** 2).all()
    trk = scpp_amd.LQRTracker(m, X, U, t, library=lqr_lib, horizon="finite")
    c = context(lqr_lib, "rocket2d", d, "foh")
    c.set_weights(trk.Q, trk.R)
    c.compute_gains_riccati(5)
    abi = sweep(c, S0, w, Hf, vf, 5)
    gains = trk.gains.copy()
    out = trk.filter(S0, w, keep=True)
    assert set(out) == set(ARRAYS) | {"status", "n_ok", "steps"} and out["n_ok"] == 2
    assert out["steps"] == 5 == scpp_amd.filter_steps(S0, Hf, vf, float(t.max()) / 29)[0]
    for k in ARRAYS + ("status",):
        assert (out[k] == abi[k]).all(), k
    lean = trk.filter(S0, w, H=H, measurement_noise=4.0 * v, steps=3, closed_loop=False)
    assert set(lean) == {"L", "error_std", "final_error_cov", "status", "n_ok", "steps"} and lean["steps"] == 3
    assert (trk.gains == gains).all()
    # the step rule: the smallest count >= 5 with h rho <= 1/8, from the largest rho and dt of the batch
    dt = float(t.max()) / 29
    rho = float((np.einsum("mi,ij,mj->m", H, S0, H) / v).max())
    assert abs(scpp_amd.filter_steps(S0, H, v, dt)[1] - rho) <= 1e-15 * rho
    for scale, want in ((1.0, 5), (0.5, 5), (2.0, 10), (3.3, 17), (40.0, 200)):
        assert trk.filter(scale * S0, w, H=H, measurement_noise=v, closed_loop=False)["steps"] == want == max(5, int(np.ceil(8 * scale * rho * dt - 1e-9)))
    assert trk.filter(np.stack([S0, 3.3 * S0]), w, H=H, measurement_noise=v, closed_loop=False)["steps"] == 17
    with pytest.raises(ValueError, match=r"rho.*201 steps.*steps explicitly.*measurement_noise.*sigma0"):
        trk.filter(40.2 * S0, w, H=H, measurement_noise=v)
    assert trk.filter(40.2 * S0, w, H=H, measurement_noise=v, steps=6, closed_loop=False)["steps"] == 6  # an explicit count is taken as given
    trk.close()
    c.close()
    no_gains = scpp_amd.LQRTracker(m, X, U, t, library=lqr_lib, compute=False)
    assert "state_std" not in no_gains.filter(S0, w)
    no_gains.close()
    with pytest.raises(ValueError, match="measurement_std"):
        t2 = scpp_amd.LQRTracker(scpp_amd.Rocket2D().loadParameters(), X, U, t, library=lqr_lib, compute=False)
        try:
            t2.filter(S0, w)
        finally:
            t2.close()


@pytest.mark.gpu
def test_rate_tool_filter_leg_accounts_for_every_trajectory(hip_lib):
    """tools/lqr_rate.py --filter 1 at batch 64 (the solver's trajectories, so the device only): every trajectory of both variants is accounted
    for by its status and nothing non-finite leaves the device.  No pass / fail on time."""
    import json
    import sys

    import __graft_entry__ as g

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lqr_rate

    lqr = os.environ.get("SCPP_LQR_LIBRARY") or (g.LQR_LIB if os.path.exists(g.LQR_LIB) else g.build_lqr())
    r = lqr_rate.measure(64, repeat=1, library=hip_lib, lqr_library=lqr, filter=1)
    print(json.dumps({k: v for k, v in r.items() if k.startswith("filter_")}, indent=1))
    assert r["filter_trajectories"] == 64 and r["filter_rhs"] == 64 * 49 * 13 and r["filter_steps_per_segment"] == 1
    for key in ("filter_alone", "filter_loop"):
        assert r[f"{key}_status_ok"] + r[f"{key}_status_gains_incomplete"] + r[f"{key}_status_nonfinite"] == 64
        assert r[f"{key}_status_other"] == 0 and r[f"{key}_nonfinite_values"] == 0
        assert r[f"{key}_wall_s"] > 0 and len(r[f"{key}_final_position_std_p5_p50_p95"]) == 3
    assert r["filter_alone_status_gains_incomplete"] == 0  # the filter alone reads no gains

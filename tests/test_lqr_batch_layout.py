"""Per-trajectory addressing of the four LQR kernels (scpp_amd/csrc/lqr/: frozen-time gains, tracking, Riccati sweep, covariance sweep): every test
runs the SAME assertions on the CPU emulation of the kernel sources (`emu`) and, marked gpu, on the device library (`hip`).

The other LQR tests feed the kernels homogeneous batches: one parameter row, one sigma0, golden trajectories that differ only in X / U / t,
K = 30 or 50 with B K even, U rows == inputs used.  There every per-trajectory address but the X / U / G base is the same whether its stride is
right, zero or garbage.  Here every trajectory of a batch has its own nodes, flight time, parameter row and initial covariance, the shapes are
the smallest at which the indexing can go wrong (K = 2, 3, 5; steps = 1, 2, 3; B K odd; 65 flights = one block of 64 and one of 1), and U comes
through the device-pointer entry with a row stride larger than the rows used.

Checkers (none shares code with the kernels): lqr_riccati_reference.twin, lqr_covariance_reference.twin, lqr_reference.tracker_gains /
scipy_gain / track, each evaluated with the trajectory's OWN row.  Inputs: tests/golden/lqr_<model>.npz only (read only).

Bars: bitwise equality wherever two device computations must agree; device vs twin 10 x the twin's rounding floor (the project's rule; the floor
is measured here, the twin against a copy with Jacobians perturbed by 1 ulp, the largest over the trajectories of the case and three seeds --
a single draw at K = 5 is noisy); frozen-time gains vs scipy 10 x the restatement's own gap on the same nodes; flights 1e-9 (the bar of
test_lqr.py::test_tracking_kernel_alone).  Each value test also asserts, with the references alone, that reading row 0 instead of row b would
miss its bar by orders of magnitude."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import lqr_covariance_reference as cr
import lqr_reference as ref
import lqr_riccati_reference as rr

MODELS = {"rocketquat": 0, "rocket2d": 1, "lander3dof": 2}
NAMES = ["rocketquat", "rocket2d", "lander3dof"]
HOLDS = ["foh", "zoh"]
SHAPES = [(2, 1), (3, 3), (5, 2)]  # (K, steps)
BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
EPS = float(np.finfo(float).eps)
E_ARG, E_STATE = -1, -4
COV_KEYS = ("cov", "state_std", "input_cov", "final_cov", "status")


@pytest.fixture(scope="module", params=BACKENDS)
def backend(request):
    """(name, LQR library) of the emulation build or of the device build"""
    import __graft_entry__ as g

    g.build_oracle()
    if request.param == "emu":
        return "emu", g.build_lqr_emu()
    lib = os.environ.get("SCPP_LQR_LIBRARY") or g.LQR_LIB
    if not os.path.exists(lib):
        g.build_lqr()
    return "hip", lib


@pytest.fixture(scope="module")
def lqr_lib(backend):
    return backend[1]


def golden(name):
    return np.load(os.path.join(GOLDEN, f"lqr_{name}.npz"))


# ---- the heterogeneous batch ---------------------------------------------------------------------------------------------------------------
_batches = {}


def hetero(name, hold, K, B=3):
    """B trajectories cut from golden trajectory 0 of (name, hold), no two alike in anything a kernel reads per trajectory: trajectory b takes
    the golden nodes arange(K) * ((K_golden - 1) // K) + b and the matching input rows (index clipped to the last golden row; K rows first-order
    hold, K - 1 zero-order hold), flies t_golden (K - 1) / (K_golden - 1) (1 + 0.1 b), has the parameter row par_golden (1 + 0.03 b) and the
    initial covariance L L', L = 0.1 randn (seed per b), symmetrised to the bit.  w is one disturbance intensity for the batch.  Not dynamically
    feasible, and need not be: both sweeps are linear time-varying equations along interpolated points.  Cached; nobody writes to it."""
    key = (name, hold, K, B)
    if key not in _batches:
        d = golden(name)
        Xg, Ug, tg = d[f"{hold}_X"][0], d[f"{hold}_U"][0], float(d[f"{hold}_t"][0])
        Kg, nx = Xg.shape
        nU = K if hold == "foh" else K - 1
        stride = (Kg - 1) // K
        X = np.stack([Xg[np.arange(K) * stride + b] for b in range(B)])
        U = np.stack([Ug[np.minimum(np.arange(nU) * stride + b, Ug.shape[0] - 1)] for b in range(B)])
        t = tg * (K - 1) / (Kg - 1) * (1.0 + 0.1 * np.arange(B))
        par = d["par"][None, :] * (1.0 + 0.03 * np.arange(B))[:, None]
        S0 = np.zeros((B, nx, nx))
        for b in range(B):
            L = 0.1 * np.random.default_rng(4100 + b).standard_normal((nx, nx))
            S = L @ L.T
            S0[b] = 0.5 * (S + S.T)
        assert (S0 == S0.transpose(0, 2, 1)).all()
        w = 1e-3 * (1.0 + np.arange(nx) / nx)
        out = dict(X=X, U=U, t=t, par=par, S0=S0, w=w, q=d["q"], r=d["r"], time_step=float(d["time_step"]))
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _batches[key] = out
    return _batches[key]


def new_context(lib, name, hold, K, B, h, rows=None):
    """a context of batch_max B with the weights of the batch and the parameter rows `rows` of it (default: all B)"""
    from scpp_amd import _lib

    c = _lib.LqrContext(MODELS[name], K, B, hold == "foh", 0, lib)
    c.set_weights(h["q"], h["r"])
    c.set_flow_params(h["par"] if rows is None else h["par"][rows])
    return c


def everything(c, S0, w, steps):
    """frozen-time gains, Riccati gains with P, the covariance under the Riccati gains: all a context computes for the trajectories it holds"""
    n_frozen = c.compute_gains()
    frozen = c.download_gains()
    n_ric = c.compute_gains_riccati(steps, True)
    ric = c.download_gains()
    ric["P"] = c.download_riccati()
    c.set_covariance_inputs(S0, w)
    n_cov = c.propagate_covariance(steps, True)
    cov = c.download_covariance(True)
    return dict(frozen=frozen, riccati=ric, cov=cov, n=(n_frozen, n_ric, n_cov))


_runs = {}


def batch_run(lib, name, hold, K, steps):
    """everything() of the heterogeneous batch of three, computed once per (library, case) and shared by the tests; left unchanged"""
    key = (lib, name, hold, K, steps)
    if key not in _runs:
        h = hetero(name, hold, K)
        c = new_context(lib, name, hold, K, 3, h)
        c.set_trajectories(h["X"], h["U"], h["t"])
        _runs[key] = everything(c, h["S0"], h["w"], steps)
        c.close()
    return _runs[key]


def same(a, b):
    return a.shape == b.shape and bool((a == b).all())


def ulp_perturb(rng):
    def f(A, Bm):
        return A * (1.0 + EPS * rng.choice([-1.0, 1.0], A.shape)), Bm * (1.0 + EPS * rng.choice([-1.0, 1.0], Bm.shape))

    return f


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,steps", SHAPES)
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_batch_equals_alone_bitwise(lqr_lib, name, hold, K, steps):
    """Trajectory b of the heterogeneous batch of three == the same trajectory alone in a batch_max = 1 context that is given par[b] as its
    single row (par_stride 0 there, np here) and sigma0[b] (s0_stride 0 there, nx nx here): frozen-time gains, Riccati gains, P, status,
    counts, cov, state_std, input_cov, final_cov, all bitwise.  With K odd, b = 1 moves every node to the other half-wave of the gain kernel,
    and B K = 9 or 15 leaves the last wavefront's second half idle."""
    h = hetero(name, hold, K)
    batch = batch_run(lqr_lib, name, hold, K, steps)
    assert batch["n"] == (3 * K, 3 * K, 3), batch["n"]
    for b in range(3):
        c = new_context(lqr_lib, name, hold, K, 1, h, rows=slice(b, b + 1))
        c.set_trajectories(h["X"][b:b + 1], h["U"][b:b + 1], h["t"][b:b + 1])
        one = everything(c, h["S0"][b], h["w"], steps)
        c.close()
        assert one["n"] == (K, K, 1), (b, one["n"])
        for law, keys in (("frozen", ("gains", "status", "iters")), ("riccati", ("gains", "status", "iters", "P")), ("cov", COV_KEYS)):
            for k in keys:
                assert same(one[law][k][0], batch[law][k][b]), (b, law, k)
    # the trajectories do differ: a kernel that read trajectory 0 for every b would have failed above
    for law, k in (("frozen", "gains"), ("riccati", "P"), ("cov", "final_cov")):
        assert not same(batch[law][k][0], batch[law][k][1]) and not same(batch[law][k][0], batch[law][k][2]), (law, k)


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_each_trajectory_against_the_twin_at_its_own_row(lqr_lib, name, hold):
    """K = 5, steps = 2, the batch of test 1.  P and K of trajectory b vs rr.twin at par[b] (rel_gap), cov and input_cov vs cr.twin at par[b]
    under the device's own gains of b with sigma0[b] (scaled_gap); bar 10 x the twin's rounding floor, measured here as
    test_lqr_riccati.py::test_structure and the generators do (the twin against a copy with Jacobians perturbed by 1 ulp -- for G S G' the
    copy's node product also takes a gain perturbed by 1 ulp, generate_lqr_covariance_goldens.py), the largest over the three trajectories and
    three seeds.  Frozen-time gains vs scipy_gain at par[b], node by node relative to the node's max|K_scipy|; bar 10 x the largest gap
    tracker_gains shows against scipy on the same nodes.  Every status 0.
    With the references alone: for b >= 1 the twin with row 0's par (P) or row 0's sigma0 (cov) misses the bar by a factor >= 1e4."""
    K, steps, B = 5, 2, 3
    m = MODELS[name]
    h = hetero(name, hold, K)
    o = batch_run(lqr_lib, name, hold, K, steps)
    X, U, t, par, S0, w, q, r = (h[k] for k in ("X", "U", "t", "par", "S0", "w", "q", "r"))
    assert (o["frozen"]["status"] == 0).all() and (o["riccati"]["status"] == 0).all() and (o["cov"]["status"] == 0).all()
    assert (o["riccati"]["iters"] == (K - 1 - np.arange(K)) * steps).all()
    G = o["riccati"]["gains"]
    twins = []
    fl = dict(P=0.0, K=0.0, S=0.0, I=0.0)
    for b in range(B):
        Pt, Gt = rr.twin(m, par[b], X[b], U[b], float(t[b]), q, r, steps=steps)
        St, It = cr.twin(m, par[b], X[b], U[b], float(t[b]), G[b], S0[b], w, steps=steps)
        twins.append((Pt, Gt, St, It))
        for seed in range(3):
            rng = np.random.default_rng(1000 + 10 * b + seed)
            Pp, Gp = rr.twin(m, par[b], X[b], U[b], float(t[b]), q, r, steps=steps, perturb=ulp_perturb(rng))
            Sp, _ = cr.twin(m, par[b], X[b], U[b], float(t[b]), G[b], S0[b], w, steps=steps, perturb=ulp_perturb(rng))
            Ip = cr.input_cov(G[b] * (1.0 + EPS * rng.choice([-1.0, 1.0], G[b].shape)), Sp)
            fl["P"], fl["K"] = max(fl["P"], rr.rel_gap(Pp, Pt)), max(fl["K"], rr.rel_gap(Gp, Gt))
            fl["S"], fl["I"] = max(fl["S"], cr.scaled_gap(Sp, St)), max(fl["I"], cr.scaled_gap(Ip, It))
    assert all(v > 0.0 for v in fl.values()), fl
    worst = 0.0
    for b in range(B):
        Pt, Gt, St, It = twins[b]
        gap = dict(P=rr.rel_gap(o["riccati"]["P"][b], Pt), K=rr.rel_gap(G[b], Gt),
                   S=cr.scaled_gap(o["cov"]["cov"][b], St), I=cr.scaled_gap(o["cov"]["input_cov"][b], It))
        print(f"{name} {hold} {b}: vs twin " + ", ".join(f"{k} {gap[k]:.2e} (bar {10 * fl[k]:.2e}, {gap[k] / fl[k]:.2f} floors)" for k in gap))
        worst = max(worst, max(gap[k] / fl[k] for k in gap))
        for k in gap:
            assert gap[k] <= 10.0 * fl[k], (b, k, gap[k], fl[k])
        if b:
            P0, _ = rr.twin(m, par[0], X[b], U[b], float(t[b]), q, r, steps=steps)
            S00, _ = cr.twin(m, par[b], X[b], U[b], float(t[b]), G[b], S0[0], w, steps=steps)
            wp, ws = rr.rel_gap(P0, Pt), cr.scaled_gap(S00, St)
            print(f"{name} {hold} {b}: the twin with row 0's par moves P by {wp:.2e} ({wp / (10 * fl['P']):.1e} bars), with row 0's sigma0 moves S by "
                  f"{ws:.2e} ({ws / (10 * fl['S']):.1e} bars)")
            assert wp >= 1e4 * 10.0 * fl["P"] and ws >= 1e4 * 10.0 * fl["S"], (b, wp, ws, fl)
    print(f"{name} {hold}: worst device-vs-twin ratio {worst:.2f} floors (bar 10)")
    # frozen-time gains, node by node
    Fg = o["frozen"]["gains"]
    gaps, own = np.zeros((B, K)), np.zeros((B, K))
    for b in range(B):
        Gr, _, st = ref.tracker_gains(m, X[b], U[b], par[b], q, r)
        assert (st == 0).all()
        for k in range(K):
            Ks = ref.scipy_gain(m, X[b, k], U[b, ref.input_index(k, K, U.shape[1])], par[b], q, r)
            gaps[b, k] = np.abs(Fg[b, k] - Ks).max() / np.abs(Ks).max()
            own[b, k] = np.abs(Gr[k] - Ks).max() / np.abs(Ks).max()
    bar = 10.0 * float(own.max())
    print(f"{name} {hold}: frozen-time gains vs scipy at the trajectory's own row {gaps.max():.2e} (bar {bar:.2e})")
    assert gaps.max() <= bar, (gaps.max(), bar)


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------
class DeviceBuffers:
    """Copies of `arrays` the library can read as device memory, owned by the test and not by the context.  Emulator: the numpy arrays
    themselves.  Device: hipMalloc + hipMemcpy of the HIP runtime the LQR library itself is linked against, reached through the library's own
    handle (dlsym searches a library's dependencies), so the memory belongs to the runtime that launches the kernels.  Not torch tensors: the
    torch wheel brings a HIP runtime of its own, and in a process in which the project's libraries have initialised theirs first -- every GPU
    test before this one does -- torch finds no GPU (measured on the MI355X: "No HIP GPUs are available").  hipMemcpy from pageable host
    memory returns after the copy, so the buffers are complete before the first call on the context's stream."""

    def __init__(self, backend_name, lib, arrays):
        import ctypes as C

        from scpp_amd import _lib

        self.host = [np.array(a, dtype=np.float64, order="C") for a in arrays]
        self.rt, self.ptrs = None, []
        if backend_name == "emu":
            self.ptrs = [a.ctypes.data for a in self.host]
            return
        self.rt = _lib.load_lqr_library(lib)
        self.rt.hipMalloc.argtypes, self.rt.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
        self.rt.hipMemcpy.argtypes, self.rt.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
        self.rt.hipFree.argtypes, self.rt.hipFree.restype = [C.c_void_p], C.c_int
        for a in self.host:
            d = C.c_void_p()
            assert self.rt.hipMalloc(C.byref(d), a.nbytes) == 0 and d.value
            self.ptrs.append(d.value)
            assert self.rt.hipMemcpy(d, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice

    def free(self):
        """after the context that read them is closed (closing synchronises its stream)"""
        if self.rt is not None:
            for d in self.ptrs:
                assert self.rt.hipFree(d) == 0
        self.ptrs = []


@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_u_row_stride_through_the_device_pointer_entry(backend, name, hold):
    """B = 3, K = 5: U sits in a buffer [B][K + 2][nu] of which the first nU rows of each trajectory are inputs (nU = K or K - 1) and the rest
    is 7.5 in one run and NaN in the other; X and t in buffers of their own; handed over by scpp_hip_lqr_set_trajectories_device with
    u_rows = K + 2 (the buffers: DeviceBuffers).  Frozen-time gains, Riccati gains and P, every covariance output and a 40-step flight are bitwise those of the upload
    path (U [B][nU][nu]) -- so each kernel strides U by u_rows, reads no row past nU, and its non-finite scan stops at nU rows (NaN padding
    retires no trajectory).  u_rows = nU - 1 is refused."""
    bname, lib = backend
    K, steps, B = 5, 2, 3
    h = hetero(name, hold, K)
    X, U, t = h["X"], h["U"], h["t"]
    nU, nu = U.shape[1], U.shape[2]
    rng = np.random.default_rng(77)
    xs = X[:, 0] * (1.0 + 0.01 * rng.standard_normal(X[:, 0].shape))

    def run(setter):
        c = new_context(lib, name, hold, K, B, h)
        setter(c)
        o = everything(c, h["S0"], h["w"], steps)
        o["n_finite"] = c.track(xs, X[0, -1], 0.01, 20, 40)
        o["flight"] = c.track_download()
        return o, c

    up, c = run(lambda c: c.set_trajectories(X, U, t))
    c.close()
    assert up["n"] == (B * K, B * K, B) and up["n_finite"] == B
    for fill in (7.5, np.nan):
        Upad = np.full((B, K + 2, nu), fill)
        Upad[:, :nU] = U
        bufs = DeviceBuffers(bname, lib, [X, Upad, t])
        pX, pU, pt = bufs.ptrs
        dev, c = run(lambda c: c.set_trajectories_device(pX, pU, pt, B, K + 2))
        assert c.lib.scpp_hip_lqr_set_trajectories_device(c.h, pX, pU, pt, B, nU - 1) == E_ARG
        c.close()
        bufs.free()
        assert dev["n"] == up["n"] and dev["n_finite"] == up["n_finite"], (fill, dev["n"], dev["n_finite"])
        assert (dev["riccati"]["status"] == 0).all() and (dev["cov"]["status"] == 0).all() and (dev["flight"]["status"] == up["flight"]["status"]).all()
        for law, keys in (("frozen", ("gains", "status", "iters")), ("riccati", ("gains", "status", "iters", "P")), ("cov", COV_KEYS),
                          ("flight", tuple(up["flight"]))):
            for k in keys:
                assert same(dev[law][k], up[law][k]), (fill, law, k)
    assert (up["flight"]["steps"] == 40).all()


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rocket2d", "rocketquat"])
def test_ragged_tracking_batch(lqr_lib, name):
    """65 flights (one full block of 64 threads and a block of one), zero-order hold, K = 5: flight b follows trajectory b % 3 of the
    heterogeneous batch with X, U and t scaled by 1 + 1e-3 (b // 3), parameter row par (1 + 1e-3 b), the Riccati gains the batch computed
    (2 steps), from node 0 with 1 % Gaussian dispersion; time_step 0.01, 20 substeps.  Flights 0, 1, 63, 64 are bitwise what a batch_max = 1
    context computes and flies with that row alone, and within 1e-9 of lqr_reference.track at par[b] under the downloaded gains of b, with
    equal step counts.  All 65 statuses 0, n_finite 65.  With the reference alone: the flight of b = 63, 64 under row 0's parameters ends
    >= 1e-4 of max|x| away from the right one."""
    K, steps, B = 5, 2, 65
    m = MODELS[name]
    h = hetero(name, "zoh", K)
    s = 1.0 + 1e-3 * (np.arange(B) // 3)
    X = h["X"][np.arange(B) % 3] * s[:, None, None]
    U = h["U"][np.arange(B) % 3] * s[:, None, None]
    t = h["t"][np.arange(B) % 3] * s
    par = h["par"][0][None, :] * (1.0 + 1e-3 * np.arange(B))[:, None]
    xs = X[:, 0] * (1.0 + 0.01 * np.random.default_rng(65).standard_normal(X[:, 0].shape))
    x_final = h["X"][0, -1]
    max_steps = int(np.ceil(t.max() / 0.01)) + 2
    hb = dict(h, par=par)
    c = new_context(lqr_lib, name, "zoh", K, B, hb)
    c.set_trajectories(X, U, t)
    assert c.compute_gains_riccati(steps) == B * K
    G = c.download_gains()["gains"]
    assert c.track(xs, x_final, 0.01, 20, max_steps) == B
    fl = c.track_download()
    c.close()
    assert (fl["status"] == 0).all() and all(np.isfinite(v).all() for v in fl.values())
    assert len(set(fl["steps"].tolist())) > 3  # flight times differ: the loops of a block retire at different steps
    for b in (0, 1, 63, 64):
        c1 = new_context(lqr_lib, name, "zoh", K, 1, hb, rows=slice(b, b + 1))
        c1.set_trajectories(X[b:b + 1], U[b:b + 1], t[b:b + 1])
        assert c1.compute_gains_riccati(steps) == K
        assert same(c1.download_gains()["gains"][0], G[b]), b
        assert c1.track(xs[b:b + 1], x_final, 0.01, 20, max_steps) == 1
        f1 = c1.track_download()
        c1.close()
        for k in f1:
            assert same(f1[k][0], fl[k][b]), (b, k)
        e = ref.track(m, par[b], X[b], U[b], G[b], float(t[b]), xs[b], x_final, 0.01)
        dx = np.abs(fl["x"][b] - e["x"]).max() / np.abs(e["x"]).max()
        du = np.abs(fl["u"][b] - e["u"]).max() / np.abs(e["u"]).max()
        print(f"{name} flight {b}: {fl['steps'][b]} steps, device loop vs restatement at its own row x {dx:.2e} u {du:.2e} (bar 1e-9)")
        assert fl["steps"][b] == e["steps"] and abs(fl["t"][b] - e["t"]) <= 1e-12
        assert dx <= 1e-9 and du <= 1e-9, (b, dx, du)
        if b >= 63:
            e0 = ref.track(m, par[0], X[b], U[b], G[b], float(t[b]), xs[b], x_final, 0.01)
            wrong = np.abs(e0["x"] - e["x"]).max() / np.abs(e["x"]).max()
            print(f"{name} flight {b}: the restatement under row 0's parameters ends {wrong:.2e} of max|x| away")
            assert wrong >= 1e-4, (b, wrong)


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_optional_outputs_change_nothing_else(lqr_lib, name, hold):
    """keep_p = 0 (Pout == nullptr) leaves gains, status and counts bitwise those of keep_p = 1; keep_cov = 0 (cov == nullptr) leaves
    state_std, input_cov, final_cov and status bitwise those of keep_cov = 1; what was not kept is refused with SCPP_E_STATE.  B = 3 on the
    heterogeneous batch, K = 5, 2 steps; the lean results come from a context that never allocated P or cov."""
    from scpp_amd import _lib

    K, steps, B = 5, 2, 3
    h = hetero(name, hold, K)
    full = batch_run(lqr_lib, name, hold, K, steps)
    c = new_context(lqr_lib, name, hold, K, B, h)
    c.set_trajectories(h["X"], h["U"], h["t"])
    assert c.compute_gains_riccati(steps, False) == B * K
    lean = c.download_gains()
    nx = h["X"].shape[2]
    Pbuf = np.full((B, K, nx, nx), 3.25)
    assert c.lib.scpp_hip_lqr_download_riccati(c.h, _lib._p(Pbuf)) == E_STATE and (Pbuf == 3.25).all()
    for k in ("gains", "status", "iters"):
        assert same(lean[k], full["riccati"][k]), k
    c.set_covariance_inputs(h["S0"], h["w"])
    assert c.propagate_covariance(steps, False) == B
    lc = c.download_covariance(False)
    out = [np.zeros((B, K, nx)), np.zeros((B, K, lean["gains"].shape[2], lean["gains"].shape[2])), np.zeros((B, nx, nx)), np.zeros(B, dtype=np.int32)]
    cov = np.full((B, K, nx, nx), 3.25)
    assert c.lib.scpp_hip_lqr_download_covariance(c.h, *[_lib._p(v) for v in out], _lib._p(cov)) == E_STATE and (cov == 3.25).all()
    c.close()
    assert "cov" not in lc
    for k in ("state_std", "input_cov", "final_cov", "status"):
        assert same(lc[k], full["cov"][k]), k
    assert (lc["status"] == 0).all() and np.abs(lc["final_cov"]).max() > 0

"""The cone layer of the interior-point solver, each function alone: the second-order-cone primitives of csrc/cone_math.h against mpmath
(cone_reference.py: written from the definitions), and the three per-cone stage steps of csrc/ipm_solve.h (coneScaling, coneT, coneDir) as
their primitives plus glue, with their memory footprint and the out-of-range view of SCvx mode (padView).

Every test runs on the wave emulator (`emu`: checks the harness, the reference, the bars and the chains) and on the device (`hip`, marked gpu:
the fused multiply-adds, the hardware division and square root, and the buffer hardware that returns 0 for a load and drops a store beyond
the record block, which the emulator only imitates).  The kernels are those of tests/cone_probe/cone_probe.cpp."""
import ctypes
import functools
import os

import mpmath as mp
import numpy as np
import pytest

import cone_reference as cr

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
DIMS = [2, 3, 4, 17]  # Rocket2D glide slope, the 3- and 4-row application cones, TD = NV + 1 of the trust-region cone
N_ITEMS = 203  # per launch: not a multiple of 64 or of the block size (256); every (delta_s, delta_z, delta_lam) of the grid three times
ZROWS = 13  # the SCvx shape of D = 17: rows 1 .. 13 exactly zero (RocketQuat's NXV)
FN_NT, FN_W, FN_WINV, FN_WINV2, FN_PROD, FN_DIV, FN_STEP = range(7)
FN_NAMES = ["nt_scaling", "applyW", "applyWinv", "applyWinv2", "conicProduct", "conicDivision", "stepInv"]
MODELS = {"RocketQuatSC": 0, "Rocket2dSC": 1, "Lander3dofSC": 2}


class Probe:
    def __init__(self, path, backend):
        self.backend = backend
        self.lib = ctypes.CDLL(path)
        self.lib.cone_probe_layout_names.restype = ctypes.c_char_p

    def call(self, name, *args):
        conv = []
        for a in args:
            if isinstance(a, np.ndarray):
                assert a.flags["C_CONTIGUOUS"]
                conv.append(a.ctypes.data_as(ctypes.c_void_p))
            else:
                conv.append(ctypes.c_int(a))
        f = getattr(self.lib, "cone_probe_" + name)
        f.restype = ctypes.c_int
        rc = f(*conv)
        assert rc == 0, (name, rc)

    def prim(self, fn, rt, a, b, eta=None):
        """(out[n][D], sc[n], flag[n]); what the function does not write is a NaN / -1"""
        a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
        n, d = a.shape
        assert b.shape == a.shape
        eta = np.ones(n) if eta is None else np.ascontiguousarray(eta, dtype=np.float64)
        out, sc, flag = np.full((n, d), np.nan), np.full(n, np.nan), np.full(n, -1, dtype=np.int32)
        self.call("prim", fn, int(rt), d, n, eta, a, b, out, sc, flag)
        return out, sc, flag

    def layout(self, model):
        n = self.lib.cone_probe_layout_count()
        raw = np.zeros(n, dtype=np.int32)
        self.call("layout", MODELS[model], raw)
        names = self.lib.cone_probe_layout_names().decode().split()
        lay = {k: int(raw[q]) for q, k in enumerate(names)}
        rest = raw[len(names):].reshape(2, -1)
        lay["coneOff"] = [int(x) for x in rest[0, : lay["NCONES"]]]
        lay["coneDim"] = [int(x) for x in rest[1, : lay["NCONES"]]]
        return lay


@pytest.fixture(scope="module", params=BACKENDS)
def probe(request):
    """the probe library of the emulation build or of the device build"""
    import __graft_entry__ as g

    if request.param == "emu":
        return Probe(os.environ.get("SCPP_CONE_PROBE_EMU_LIBRARY") or g.build_cone_probe_emu(), "emu")
    lib = os.environ.get("SCPP_CONE_PROBE_LIBRARY") or g.CONE_PROBE_LIB
    if not os.path.exists(lib):
        g.build_cone_probe()
    return Probe(lib, "hip")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------- inputs and their reference, computed once and shared by both backends
SHAPES = [(d, 0) for d in DIMS] + [(17, ZROWS)]


def shape_id(shape):
    return f"D{shape[0]}" + ("-scvx" if shape[1] else "")


@functools.lru_cache(maxsize=None)
def grid(shape):
    """s, z, lam on the grid c (1, (1 - delta) u), delta of s, z and lam independently from {0.5, 1e-2, 1e-5, 1e-8} (item q: digits of q in
    base 4); v and u2 with entries +-10^U(-3, 3); (eta, w): the exact scaling of (s, z), rounded to float64 -- from then on exact inputs"""
    d, zr = shape
    rng = np.random.default_rng(20261101 + 100 * d + zr)
    q = np.arange(N_ITEMS)
    dl = np.array(cr.DELTAS)
    g = {
        "s": cr.cone_points(rng, N_ITEMS, d, dl[q % 4], zr),
        "z": cr.cone_points(rng, N_ITEMS, d, dl[(q // 4) % 4], zr),
        "lam": cr.cone_points(rng, N_ITEMS, d, dl[(q // 16) % 4], zr),
        "v": cr.directions(rng, N_ITEMS, d, zr),
        "u2": cr.directions(rng, N_ITEMS, d, zr),
    }
    nt = [cr.nt_scaling(g["s"][i], g["z"][i]) for i in range(N_ITEMS)]
    g["w_mp"], g["eta_mp"] = [r[0] for r in nt], [r[1] for r in nt]
    g["w"] = np.array([cr.to_f64(r[0]) for r in nt])
    g["eta"] = np.array([float(r[1]) for r in nt])
    return g


def c_bar(fn, d):
    """roundings along the longest chain of each function (counted in the docstring of test_accuracy), at most 2 (D + 8)"""
    c = {FN_DIV: 2 * d + 4, FN_STEP: 2 * (d + 8)}.get(fn, d + 8)
    assert c <= 2 * (d + 8)
    return c


@functools.lru_cache(maxsize=None)
def reference(shape, fn):
    """(exact[n][k] mpf, amplification[n][k] mpf): k = D components (nt_scaling: D + 1, eta last; stepInv: 1)"""
    g = grid(shape)
    ex, amp = [], []
    for i in range(N_ITEMS):
        s, z, lam, v, u2, w, eta = g["s"][i], g["z"][i], g["lam"][i], g["v"][i], g["u2"][i], g["w"][i], g["eta"][i]
        if fn == FN_NT:
            wm, em = g["w_mp"][i], g["eta_mp"][i]
            k = cr.kappa(s) + cr.kappa(z)
            ex.append(list(wm) + [em])
            amp.append([k * max(abs(a) for a in wm)] * len(wm) + [k * em])
        elif fn == FN_W:
            ex.append(cr.apply_w(eta, w, v))
            amp.append(cr.amp_w_terms(eta, w, v))
        elif fn == FN_WINV:
            ex.append(cr.apply_winv(eta, w, v))
            amp.append(cr.amp_w_terms(eta, w, v, inverse=True))
        elif fn == FN_WINV2:
            ex.append(cr.apply_winv2(eta, w, v))
            amp.append(cr.amp_winv2_terms(eta, w, v))
        elif fn == FN_PROD:
            ex.append(cr.conic_product(u2, v))
            amp.append(cr.amp_product_terms(u2, v))
        elif fn == FN_DIV:
            ex.append(cr.conic_division(lam, v))
            amp.append(cr.amp_division_terms(lam, v))
        else:
            ex.append([cr.step_inv(lam, v)])
            amp.append([cr.amp_step(lam, v)])
    return ex, amp


def run_prim(probe, shape, fn, rt=False):
    """the device's output for the grid of `shape` as [n][k] float64, k as in reference()"""
    g = grid(shape)
    if fn == FN_NT:
        out, sc, flag = probe.prim(fn, rt, g["s"], g["z"])
        return np.concatenate([out, sc[:, None]], axis=1), flag
    if fn in (FN_W, FN_WINV, FN_WINV2):
        return probe.prim(fn, rt, g["w"], g["v"], g["eta"])[0], None
    if fn == FN_PROD:
        return probe.prim(fn, rt, g["u2"], g["v"])[0], None
    if fn == FN_DIV:
        return probe.prim(fn, rt, g["lam"], g["v"])[0], None
    return probe.prim(fn, rt, g["lam"], g["v"])[1][:, None], None


# ---------------------------------------------------------------- a. accuracy against mpmath
@pytest.mark.parametrize("fn", range(7), ids=FN_NAMES)
def test_accuracy(probe, fn):
    """|device - exact| <= c(D) u amplification per output component, u = 2^-53, amplification from the inputs alone (cone_reference.py):
    nt_scaling (kappa(s) + kappa(z)) max|w| (times eta / max|w| for eta); applyW, applyWinv, applyWinv2, conicProduct the sum of the absolute
    values of the terms of the header's formula; conicDivision that sum times kappa(lam); stepInv kappa(lam) (|mu_1| + |mu_2|).

    c(D), roundings counted to first order (a fused multiply-add counts once):
    nt_scaling, D + 8.  |s|_J^2 = s0^2 - |s1|^2: D - 1 accumulations, the square, the difference -> relative (D + 1) u kappa(s); its root halves
      that: e_s = ((D + 1) / 2 kappa(s) + 1) u, e_z likewise.  Every sbar_i carries the SAME e_s, so sbar'zbar = (exact) (1 + e_s + e_z) +
      (D + 3) u sum|sbar_i zbar_i| with sum|.| <= (kappa(s) + kappa(z) + 2) / 2, and 1 + sbar'zbar >= 2: gamma is off by (e_s + e_z) / 2 +
      (D + 3) (kappa(s) + kappa(z) + 2) u / 8 + 2 u relative.  w_i = (sbar_i +- zbar_i) / (2 gamma) with a |sbar_i| <= w0: in units of
      u (kappa(s) + kappa(z)) max|w| this is 3 (D + 1) / 4 + (D + 3) / 8 + small <= D + 8.  eta = sqrt(|s|_J / |z|_J): (D + 1) / 4 + small.
    applyW, applyWinv, D + 8.  zeta: D - 1; 1 + w0, the division, f: 3; f w_i + v_i: 1 or 2; the scaling by eta: 1 -> D + 5.
    applyWinv2, D + 8.  tv: D; eta^2 and its reciprocal: 2; -2 w_i tv + v_i: 1 or 2; the scaling: 1 -> D + 5.
    conicProduct, D + 8.  Row 0: D; the other rows: 2 or 3.
    conicDivision, 2 D + 4.  rho = lam0^2 - |lam1|^2: relative (D - 1) u kappa + u <= D u kappa; the numerator of x0: D u of its terms, the
      division 1: x0 is off by (2 D + 1) u kappa of its terms; x_i = (d_i - x0 lam_i) / lam0 adds 3.
    stepInv, 2 (D + 8), the ceiling.  The result is the difference of two chains, rho0 = (lam'J v / ln) / ln and sqrt(sum r_i^2), each of
      which runs through ln (D + 1 roundings, halved by the root, entering twice) and an accumulation of D terms: D + 8 is taken for each.
      (Not a proof; the float64 restatement of the header stays at 2.3.)

    Every bar is also at most 1e-6 of the size of the exact output: no bar here is vacuous.  The size is the largest component of the exact
    vector; for stepInv the larger root in magnitude (the value is one root, the error scales with both); for conicDivision the largest sum
    of terms without its kappa -- x0 = (lam0 d0 - lam1'd1) / rho with lam near a boundary ray cancels whenever d0 ~ +-|d1| (here down to
    1 / 26 of its terms at D = 2), which no evaluation in float64 can undo, so against the cancelled value the bar reads 2.3e-6 on this grid.
    Worst ratios per D are printed."""
    for shape in SHAPES:
        d = shape[0]
        dev, flag = run_prim(probe, shape, fn)
        ex, amp = reference(shape, fn)
        if flag is not None:
            assert (flag == 1).all(), np.flatnonzero(flag != 1)  # the whole grid is interior
        assert np.isfinite(dev).all()
        worst, worst_rel, where = 0., 0., None
        for i in range(N_ITEMS):
            if fn == FN_STEP:
                size = max(abs(m) for m in cr.step_roots(grid(shape)["lam"][i], grid(shape)["v"][i]))
            elif fn == FN_DIV:
                size = max(amp[i]) / cr.kappa(grid(shape)["lam"][i])
            else:
                size = max(abs(a) for a in ex[i][:d])
            for k in range(len(ex[i])):
                sz = abs(ex[i][k]) if (fn == FN_NT and k == d) else size
                bar = cr.U * amp[i][k]
                if bar == 0:  # a structural-zero row: every term is zero, and so is the exact value
                    assert ex[i][k] == 0 and dev[i, k] == 0., (shape, i, k, dev[i, k])
                    continue
                r = float(abs(mp.mpf(float(dev[i, k])) - ex[i][k]) / bar)
                rel = float(c_bar(fn, d) * bar / sz)
                if r > worst:
                    worst, where = r, (i, k)
                worst_rel = max(worst_rel, rel)
        print(f"{probe.backend} {FN_NAMES[fn]} {shape_id(shape)}: worst error {worst:.3f} u amplification at item, component {where} "
              f"(bar {c_bar(fn, d)}); largest bar / size of the exact output {worst_rel:.2e}")
        assert worst <= c_bar(fn, d), (shape, where, worst)
        assert worst_rel <= 1e-6, (shape, worst_rel)


# ---------------------------------------------------------------- b. exact properties
def boundary_point(d):
    """s0^2 - |s1|^2 exactly 0 in float64: (5, 3, 4, 0, ..), or (3, 3) where there is one row only"""
    x = np.zeros(d)
    x[:min(d, 3)] = [5., 3., 4.] if d > 2 else [3., 3.]
    return x


@pytest.mark.parametrize("rt", [False, True], ids=["static", "runtime"])
def test_nt_scaling_rejects(probe, rt):
    """false for s or z on the boundary, outside the cone, or with a NaN in any entry (s0, z0 > 0); w and eta are not read"""
    for d in DIMS:
        good = np.zeros(d)
        good[0], good[d - 1] = 2., 1.
        outside = np.zeros(d)
        outside[0], outside[1] = 1., 2.
        bad = [boundary_point(d), 2. ** -40 * boundary_point(d), outside]  # (a power of two keeps the boundary exact)
        for i in range(d):
            x = good.copy()
            x[i] = np.nan
            bad.append(x)
        s = np.array([b for b in bad] + [good for _ in bad] + [good])
        z = np.array([good for _ in bad] + [b for b in bad] + [good])
        _, _, flag = probe.prim(FN_NT, rt, s, z)
        assert (flag[:-1] == 0).all(), (d, np.flatnonzero(flag[:-1] != 0))
        assert flag[-1] == 1  # (and the interior point between them is accepted)


@pytest.mark.parametrize("fn", [FN_W, FN_WINV, FN_WINV2, FN_PROD, FN_DIV], ids=[FN_NAMES[f] for f in (FN_W, FN_WINV, FN_WINV2, FN_PROD, FN_DIV)])
def test_zero_rows_stay_zero(probe, fn):
    """D = 17 with rows 1 .. 13 of both operands +0.: those rows of the result are +0. bit for bit (not -0., not 1e-300) -- what the comment
    above padView (ipm_solve.h) relies on -- in the compile-time and the runtime-d function"""
    for rt in (False, True):
        dev, _ = run_prim(probe, (17, ZROWS), fn, rt)
        z = bits(dev[:, 1:1 + ZROWS])
        assert (z == 0).all(), (rt, np.argwhere(z != 0)[:8], dev[:, 1:1 + ZROWS][z != 0][:8])
        assert (dev[:, 0] != 0).all() and (dev[:, 1 + ZROWS:] != 0).all()  # (the other rows are alive)


@pytest.mark.parametrize("fn", range(7), ids=FN_NAMES)
def test_runtime_twin_same_bits(probe, fn):
    """each runtime-d function and its compile-time twin: the same bits at all four dimensions (and nt_scaling true across the grid in both)"""
    for shape in SHAPES:
        a, fa = run_prim(probe, shape, fn, False)
        b, fb = run_prim(probe, shape, fn, True)
        assert np.isfinite(a).all()
        assert same_bits(a, b), (shape, np.argwhere(bits(a) != bits(b))[:8])
        if fa is not None:
            assert (fa == 1).all() and (fb == 1).all()


# ---------------------------------------------------------------- the stage steps: records, inputs, chains
STAGE_MODELS = ["RocketQuatSC", "Rocket2dSC", "Lander3dofSC"]
STAGE_K = [3, 50, 64]
COUNT = 5  # instances per launch: not a multiple of the two wavefronts of a block
CONE_FIELDS = ["F_S", "F_Z", "F_DS", "F_DZ", "F_RZ", "F_TZ", "F_LS", "F_DSS", "F_WB"]
QNAN = np.uint64(0x7FF8000000000000)


def payloads(shape):
    """a distinct quiet-NaN payload in every double"""
    return (QNAN | (np.arange(int(np.prod(shape)), dtype=np.uint64) + np.uint64(1))).reshape(shape)


class Stage:
    """COUNT instances of one model and horizon: cone vectors as [COUNT][K][LP0] (cone C at coneOff(C) ..), eta as [COUNT][K][NCONES]"""

    def __init__(self, probe, model, K, zero_rows):
        self.probe, self.model, self.K = probe, model, K
        self.lay = lay = probe.layout(model)
        self.pitch = (K + 1) & ~1
        assert probe.lib.cone_probe_rec_pitch(K) == self.pitch
        self.nxv = lay["NXV"]
        self.zr = self.nxv if zero_rows else 0  # rows 1 .. NXV of the trust-region cone exactly zero
        self.cones = list(zip(range(lay["NCONES"]), lay["coneOff"], lay["coneDim"]))
        assert lay["coneOff"][0] == 0 and lay["coneDim"][0] == 17 and sum(lay["coneDim"]) == lay["LP0"]
        self.base = payloads((COUNT, lay["STREC"], self.pitch))

    def points(self, rng):
        """interior iterates on the grid of the primitives: delta 0.5 or 1e-2, near the boundary (1e-5, 1e-8) in a few lanes"""
        lane = np.arange(self.K)
        out = np.zeros((COUNT, self.K, self.lay["LP0"]))
        for c, off, d in self.cones:
            delta = np.where(lane % 7 == 3, 1e-8, np.where(lane % 5 == 1, 1e-5, np.where(lane % 2 == 0, 0.5, 1e-2)))
            delta = np.broadcast_to(np.roll(delta, c), (COUNT, self.K)).ravel()
            out[:, :, off:off + d] = cr.cone_points(rng, COUNT * self.K, d, delta, self.zr if c == 0 else 0).reshape(COUNT, self.K, d)
        return out

    def vectors(self, rng):
        out = np.zeros((COUNT, self.K, self.lay["LP0"]))
        for c, off, d in self.cones:
            out[:, :, off:off + d] = cr.directions(rng, COUNT * self.K, d, self.zr if c == 0 else 0).reshape(COUNT, self.K, d)
        return out

    def record(self, fields, eta=None, payload_rows=False):
        """the record block: payloads everywhere, the given cone-vector fields (and eta) at lanes < K; payload_rows: rows 1 .. NXV of the
        trust-region cone keep their payloads in those fields too (the SCvx run, which must not read them)"""
        rec = self.base.copy()
        for name, val in fields.items():
            f = self.lay[name]
            rec[:, f:f + self.lay["LP0"], :self.K] = bits(val).transpose(0, 2, 1)
            if payload_rows:
                rec[:, f + 1:f + 1 + self.nxv] = self.base[:, f + 1:f + 1 + self.nxv]
        if eta is not None:
            f = self.lay["F_ETA"]
            rec[:, f:f + self.lay["NCONES"], :self.K] = bits(eta).transpose(0, 2, 1)
        return rec

    def field(self, rec, name):
        """[COUNT][K][LP0] float64 view of a cone-vector field of a record block"""
        f = self.lay[name]
        return np.ascontiguousarray(rec[:, f:f + self.lay["LP0"], :self.K].transpose(0, 2, 1)).view(np.float64)

    def eta(self, rec):
        f = self.lay["F_ETA"]
        return np.ascontiguousarray(rec[:, f:f + self.lay["NCONES"], :self.K].transpose(0, 2, 1)).view(np.float64)

    def written(self, names, eta=False, scvx=False, skip=()):
        """mask [COUNT][STREC][pitch] of the documented outputs: the cone rows of the named fields (and F_ETA) at lanes < K; scvx: without
        rows 1 .. NXV of the trust-region cone; skip: (instance, lane, cone) whose outputs are not stored"""
        m = np.zeros(self.base.shape, dtype=bool)
        for name in names:
            f = self.lay[name]
            m[:, f:f + self.lay["LP0"], :self.K] = True
            if scvx:
                m[:, f + 1:f + 1 + self.nxv] = False
            for q, k, c in skip:
                m[q, f + self.lay["coneOff"][c]:f + self.lay["coneOff"][c] + self.lay["coneDim"][c], k] = False
        if eta:
            f = self.lay["F_ETA"]
            m[:, f:f + self.lay["NCONES"], :self.K] = True
            for q, k, c in skip:
                m[q, f + c, k] = False
        return m

    # ---- the three steps through the probe: (record after, returned values)
    def scaling(self, rec, scvx):
        rec = np.ascontiguousarray(rec.copy())
        ret = np.full((COUNT, 64), -1, dtype=np.int32)
        self.probe.call("scaling", MODELS[self.model], self.K, int(scvx), COUNT, rec, ret)
        return rec, ret

    def t(self, rec, scvx, pas, om, sigmu):
        rec = np.ascontiguousarray(rec.copy())
        tout = np.full((COUNT, self.K, self.lay["LP0"]), np.nan)
        self.probe.call("t", MODELS[self.model], self.K, int(scvx), COUNT, pas, om, sigmu, rec, tout)
        return rec, tout

    def dir(self, rec, scvx, store_final, om, Ld, ainv0):
        rec = np.ascontiguousarray(rec.copy())
        a1 = np.full((COUNT, self.K, self.lay["NCONES"]), np.nan)
        ad = np.full((COUNT, self.K, self.lay["NCONES"]), np.nan)
        self.probe.call("dir", MODELS[self.model], self.K, int(scvx), COUNT, int(store_final), om, np.ascontiguousarray(Ld), np.ascontiguousarray(ainv0), rec, a1, ad)
        return rec, a1, ad

    # ---- a primitive on every cone of every stage: one probe call per cone dimension (the compile-time function, as the steps use)
    def prim(self, fn, a, b, eta=None):
        out = np.full(a.shape, np.nan)
        sc = np.full((COUNT, self.K, self.lay["NCONES"]), np.nan)
        flag = np.full((COUNT, self.K, self.lay["NCONES"]), -1, dtype=np.int32)
        for d in sorted(set(self.lay["coneDim"])):
            cs = [(c, off) for c, off, dd in self.cones if dd == d]
            ga = np.concatenate([a[:, :, off:off + d].reshape(-1, d) for _, off in cs])
            gb = np.concatenate([b[:, :, off:off + d].reshape(-1, d) for _, off in cs])
            ge = None if eta is None else np.concatenate([eta[:, :, c].ravel() for c, _ in cs])
            o, s, f = self.probe.prim(fn, False, ga, gb, ge)
            n = COUNT * self.K
            for j, (c, off) in enumerate(cs):
                out[:, :, off:off + d] = o[j * n:(j + 1) * n].reshape(COUNT, self.K, d)
                sc[:, :, c] = s[j * n:(j + 1) * n].reshape(COUNT, self.K)
                flag[:, :, c] = f[j * n:(j + 1) * n].reshape(COUNT, self.K)
        return out, sc, flag

    def row0(self):
        """[LP0] mask of row 0 of every cone"""
        m = np.zeros(self.lay["LP0"], dtype=bool)
        m[self.lay["coneOff"]] = True
        return m

    def scaled(self, rng):
        """(s, z, eta, w, lam) of interior iterates, the scaling from the primitives' probe: inputs of coneT and coneDir"""
        s, z = self.points(rng), self.points(rng)
        w, eta, ok = self.prim(FN_NT, s, z)
        assert (ok == 1).all()
        lam = self.prim(FN_W, w, z, eta)[0]
        return s, z, eta, w, lam


def fused_neg_mul_add(om, rz, ld):
    """-om rz + ld rounded once"""
    from fractions import Fraction

    out = np.empty(rz.shape)
    for idx in np.ndindex(rz.shape):
        out[idx] = float(-Fraction(float(om[idx[0]])) * Fraction(float(rz[idx])) + Fraction(float(ld[idx])))
    return out


def stage_scalars(rng):
    om = rng.uniform(0.05, 1., COUNT)
    sigmu = 10. ** rng.uniform(-6., 1., COUNT)
    return om, sigmu


def outside_lanes(st):
    """one (instance, lane, cone) per instance whose s lies outside the cone"""
    return [(q, (7 * q + 1) % st.K, q % st.lay["NCONES"]) for q in range(COUNT)]


def seed_of(model, K):
    return 20261200 + 1000 * MODELS[model] + K


def all_steps(st, rng):
    """the inputs of the five step variants as (name, fields, eta, runner(rec, scvx) -> (rec, returned values..), output fields, eta is an output, skip)"""
    s, z, eta, w, lam = st.scaled(rng)
    rz, dss, tz, Ld = st.vectors(rng), st.vectors(rng), st.vectors(rng), st.vectors(rng)
    om, sigmu = stage_scalars(rng)
    ainv0 = rng.choice([-1., 1.], size=(COUNT, st.K)) * 10. ** rng.uniform(-2., 2., size=(COUNT, st.K))
    s_out = s.copy()
    skip = outside_lanes(st)
    for q, k, c in skip:
        off = st.lay["coneOff"][c]
        s_out[q, k, off] *= 1e-3  # s0 below |s1|: outside the cone
        assert s_out[q, k, off] ** 2 < (s_out[q, k, off + 1:off + st.lay["coneDim"][c]] ** 2).sum()
    inputs = {"s": s, "z": z, "eta": eta, "w": w, "lam": lam, "rz": rz, "dss": dss, "tz": tz, "Ld": Ld, "om": om, "sigmu": sigmu, "ainv0": ainv0, "s_out": s_out,
              "skip": skip}
    steps = [
        ("coneScaling", {"F_S": s_out, "F_Z": z}, None, lambda rec, scvx: st.scaling(rec, scvx), ["F_WB", "F_LS"], True, skip),
        ("coneT pass 0", {"F_WB": w, "F_RZ": rz, "F_Z": z}, eta, lambda rec, scvx: st.t(rec, scvx, 0, om, sigmu), ["F_TZ"], False, ()),
        ("coneT pass 1", {"F_WB": w, "F_RZ": rz, "F_DSS": dss, "F_LS": lam}, eta, lambda rec, scvx: st.t(rec, scvx, 1, om, sigmu), ["F_TZ"], False, ()),
        ("coneDir predictor", {"F_WB": w, "F_TZ": tz, "F_RZ": rz, "F_LS": lam}, eta, lambda rec, scvx: st.dir(rec, scvx, False, om, Ld, ainv0), ["F_DSS"], False, ()),
        ("coneDir final", {"F_WB": w, "F_TZ": tz, "F_RZ": rz, "F_LS": lam}, eta, lambda rec, scvx: st.dir(rec, scvx, True, om, Ld, ainv0), ["F_DZ", "F_DS"], False, ()),
    ]
    return inputs, steps


# ---------------------------------------------------------------- c. the per-cone steps are their primitives plus glue
@pytest.mark.parametrize("K", STAGE_K)
@pytest.mark.parametrize("model", STAGE_MODELS)
def test_steps_are_primitives_plus_glue(probe, model, K):
    """coneScaling, coneT (both passes) and coneDir (both store_final) replayed as chains of primitive-probe calls with the glue in numpy (the
    scalings by om, + sigmu on row 0, elementwise sums and differences): every output field, a1 and ainv_dual equal the chain BITWISE -- the
    build forms fused multiply-adds per source expression so that the same arithmetic rounds the same in different surroundings.  The one glue
    expression written as a multiply-add, ds = -om rz + Ld of coneDir, may round fused (device) or unfused (emulator): one of the two must
    match every element of the launch that stores ds, and the chain is fed from that one.
    One lane per instance has s outside one cone: coneScaling returns 1 there and stores nothing for that cone; every other lane returns 0."""
    st = Stage(probe, model, K, zero_rows=False)
    x, steps = all_steps(st, np.random.default_rng(seed_of(model, K)))
    run = {name: runner(st.record(fields, eta), False) for name, fields, eta, runner, _, _, _ in steps}
    ncones = st.lay["NCONES"]

    def differs(a, b):
        return np.argwhere(bits(a) != bits(b))[:8]

    # coneScaling = nt_scaling, applyW
    rec, ret = run["coneScaling"]
    w, eta, ok = st.prim(FN_NT, x["s_out"], x["z"])
    want = np.zeros((COUNT, K), dtype=np.int32)
    for q, k, c in x["skip"]:
        want[q, k] = 1 << c
    assert np.array_equal(ret[:, :K], want) and (ret[:, K:] == -1).all(), np.argwhere(ret[:, :K] != want)[:8]
    left = np.zeros((COUNT, K, ncones), dtype=bool)
    for q, k, c in x["skip"]:
        left[q, k, c] = True
    assert np.array_equal(ok == 0, left)
    lam = st.prim(FN_W, w, x["z"], eta)[0]
    stored = st.written(["F_WB"], eta=True, skip=x["skip"])
    f = st.lay["F_WB"]
    keep = stored[:, f:f + st.lay["LP0"], :K].transpose(0, 2, 1)  # [COUNT][K][LP0]: False where the cone left and nothing is stored
    assert not differs(st.field(rec, "F_WB")[keep], w[keep]).size
    assert not differs(st.field(rec, "F_LS")[keep], lam[keep]).size
    assert not differs(st.eta(rec)[ok == 1], eta[ok == 1]).size

    # coneT = applyWinv2 (- z | + applyWinv(conicDivision - lam))
    eta, w, lam, om = x["eta"], x["w"], x["lam"], x["om"][:, None, None]
    b2 = st.prim(FN_WINV2, w, x["rz"] * om, eta)[0]
    rec, tout = run["coneT pass 0"]
    t0 = b2 - x["z"]
    assert not differs(st.field(rec, "F_TZ"), t0).size and not differs(tout, t0).size
    rec, tout = run["coneT pass 1"]
    dsv = np.where(st.row0(), -x["dss"] + x["sigmu"][:, None, None], -x["dss"])
    aa = st.prim(FN_WINV, w, st.prim(FN_DIV, lam, dsv)[0] - lam, eta)[0]
    t1 = b2 + aa
    assert not differs(st.field(rec, "F_TZ"), t1).size and not differs(tout, t1).size

    # coneDir = applyWinv2, applyWinv, applyW, (conicProduct), stepInv twice
    aa = st.prim(FN_WINV2, w, x["Ld"], eta)[0]
    dz = -aa + x["tz"]
    rec_f, a1_f, ad_f = run["coneDir final"]
    ds_dev = st.field(rec_f, "F_DS")
    ds_unfused = -x["om"][:, None, None] * x["rz"] + x["Ld"]
    ds_fused = fused_neg_mul_add(x["om"], x["rz"], x["Ld"])
    assert same_bits(ds_dev, ds_fused) or same_bits(ds_dev, ds_unfused), (differs(ds_dev, ds_fused), differs(ds_dev, ds_unfused))
    ds = ds_fused if same_bits(ds_dev, ds_fused) else ds_unfused
    print(f"{probe.backend} {model} K = {K}: ds = -om rz + Ld rounds {'fused' if ds is ds_fused else 'unfused'}"
          f" ({int((bits(ds_fused) != bits(ds_unfused)).sum())} of {ds.size} elements tell the two apart)")
    assert not differs(st.field(rec_f, "F_DZ"), dz).size
    dss = st.prim(FN_WINV, w, ds, eta)[0]
    dzs = st.prim(FN_W, w, dz, eta)[0]
    a1 = st.prim(FN_STEP, lam, dss)[1]
    a2 = st.prim(FN_STEP, lam, dzs)[1]
    ad = np.where(a2 > x["ainv0"][:, :, None], a2, x["ainv0"][:, :, None])
    assert ((a2 > x["ainv0"][:, :, None]).any() and (a2 <= x["ainv0"][:, :, None]).any())  # the running maximum goes both ways
    assert not differs(a1_f, a1).size and not differs(ad_f, ad).size
    rec_p, a1_p, ad_p = run["coneDir predictor"]
    assert not differs(st.field(rec_p, "F_DSS"), st.prim(FN_PROD, dss, dzs)[0]).size
    assert not differs(a1_p, a1).size and not differs(ad_p, ad).size


# ---------------------------------------------------------------- d. footprint, and the out-of-range view
@pytest.mark.parametrize("K", STAGE_K)
@pytest.mark.parametrize("model", STAGE_MODELS)
def test_footprint_and_padded_view(probe, model, K):
    """Before a step every double of the record block that is not a documented input of the step holds a distinct quiet-NaN payload (all STREC
    fields, all pitch lanes, the pad lanes >= K too).  Afterwards every double outside the documented outputs at lanes < K (F_ETA + cix, F_WB,
    F_LS for coneScaling; F_TZ for coneT; F_DZ and F_DS, or F_DSS, for coneDir) is bitwise what it was, and every documented output was written.
    SCvx: each step runs once with scvx = false and rows 1 .. NXV of the trust-region cone +0. in every cone-vector field it reads, and once
    with scvx = true and payloads in those rows of the fields it reads AND writes: all other outputs and every returned value agree bitwise,
    and the rows still hold their payloads -- a load through padView returned 0 and a store through it was dropped, by the buffer hardware on
    the device.  Rows NXV + 1 .. 16 and row 0 are read and written normally in both runs."""
    st = Stage(probe, model, K, zero_rows=True)
    _, steps = all_steps(st, np.random.default_rng(seed_of(model, K) + 500))
    nxv = st.nxv
    for name, fields, eta, runner, outs, eta_out, skip in steps:
        before_a, before_b = st.record(fields, eta), st.record(fields, eta, payload_rows=True)
        for f in fields:  # the inputs differ in the padded rows only
            lo = st.lay[f]
            assert (before_a[:, lo + 1:lo + 1 + nxv, :K] == 0).all() and (before_b[:, lo + 1:lo + 1 + nxv] == st.base[:, lo + 1:lo + 1 + nxv]).all()
        res_a, res_b = runner(before_a, False), runner(before_b, True)
        after_a, after_b = res_a[0], res_b[0]
        ma, mb = st.written(outs, eta_out, False, skip), st.written(outs, eta_out, True, skip)
        for tag, before, after, m in (("scvx = false", before_a, after_a, ma), ("scvx = true", before_b, after_b, mb)):
            assert (after[~m] == before[~m]).all(), (name, tag, np.argwhere((after != before) & ~m)[:8])  # [instance][field][lane]
            assert (after[m] != before[m]).all(), (name, tag, np.argwhere((after == before) & m)[:8])
            assert not (np.isnan(after.view(np.float64)) & m).any(), (name, tag)
        assert (after_a[mb] == after_b[mb]).all(), (name, np.argwhere((after_a != after_b) & mb)[:8])
        for ra, rb in zip(res_a[1:], res_b[1:]):
            assert np.array_equal(ra.view(np.uint8), rb.view(np.uint8)), name
        if name == "coneScaling":
            want = np.zeros((COUNT, K), dtype=np.int32)
            for q, k, c in skip:
                want[q, k] = 1 << c
            assert np.array_equal(res_b[1][:, :K], want)

"""The solver's tile engine (csrc/tile_engine.h) and lane primitives (csrc/common.h), each function alone, against references that share
nothing with them (tile_reference.py: mpmath, longdouble, a float64 twin, index maps written from the comments).

Every test runs on the wave emulator (`emu`: checks the harness, the reference and the algebra) and on the device (`hip`, marked gpu: the
DPP control words, the permlane swaps, the hardware reciprocal seeds and the real MFMA register layouts, none of which the emulator has).
The kernels are those of tests/tile_probe/tile_probe.cpp: one wavefront per item, four per block, one or two launches per test."""
import ctypes
import os

import mpmath
import numpy as np
import pytest

import tile_reference as tr
from tile_reference import EPS

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
COUNT = 37  # items per launch: not a multiple of the four wavefronts of a block
SIZES = [1, 4, 5, 6, 7, 13, 14, 16]  # the product's 6, 7, 14, 16 and the sizes next to a register-row boundary
KAPPAS = [10., 1e4, 1e8]
PER_CASE = 8


class Probe:
    def __init__(self, path, backend):
        self.backend = backend
        self.lib = ctypes.CDLL(path)
        self.cache = {}

    def call(self, name, *args):
        conv = []
        for a in args:
            if isinstance(a, np.ndarray):
                assert a.flags["C_CONTIGUOUS"]
                conv.append(a.ctypes.data_as(ctypes.c_void_p))
            else:
                conv.append(ctypes.c_int(a))
        f = getattr(self.lib, "tile_probe_" + name)
        f.restype = ctypes.c_int
        rc = f(*conv)
        assert rc == 0, (name, rc)


@pytest.fixture(scope="module", params=BACKENDS)
def probe(request):
    """the probe library of the emulation build or of the device build"""
    import __graft_entry__ as g

    if request.param == "emu":
        return Probe(os.environ.get("SCPP_TILE_PROBE_EMU_LIBRARY") or g.build_tile_probe_emu(), "emu")
    lib = os.environ.get("SCPP_TILE_PROBE_LIBRARY") or g.TILE_PROBE_LIB
    if not os.path.exists(lib):
        g.build_tile_probe()
    return Probe(lib, "hip")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------- a. lane moves, bitwise
def test_lane_moves_bitwise(probe):
    maps = tr.lane_maps()
    names = sorted(maps, key=lambda k: maps[k][0]) + ["readLane(63)"]  # 92 moves + one repeated: not a multiple of the 4 wavefronts of a block
    n = len(names)
    assert n == 93
    rng = np.random.default_rng(20261018)
    v = rng.integers(1 << 20, 1 << 32, size=(n, 64), dtype=np.uint64) << np.uint64(32) | rng.integers(1 << 20, 1 << 32, size=(n, 64), dtype=np.uint64)
    assert ((v >> np.uint64(32)) != (v & np.uint64(0xFFFFFFFF))).all()  # every move splits a double into two ints: the halves must differ
    ops = np.array([maps[k][0] for k in names], dtype=np.int32)
    out = np.zeros_like(v)
    probe.call("lane_move", n, ops, v, out)
    bad = [k for q, k in enumerate(names) if not np.array_equal(out[q], tr.apply_map(v[q], maps[k][1]))]
    assert not bad, bad
    q = names.index("prevLane")  # lane 0 receives 0, and the shift crosses the rows of 16 lanes
    assert out[q, 0] == 0 and all(out[q, l] == v[q, l - 1] for l in (16, 32, 48))


def test_any_lane(probe):
    pred = np.zeros((66, 64), dtype=np.int32)  # all false, all true, exactly one true lane for each of the 64 lanes
    pred[1] = 1
    pred[2:] = np.eye(64, dtype=np.int32)
    out = np.full_like(pred, -1)
    probe.call("any_lane", 66, pred, out)
    assert (out[0] == 0).all()
    assert (out[1:] == 1).all(), np.argwhere(out[1:] != 1)


# ---------------------------------------------------------------- b. reductions
def test_reductions(probe):
    rng = np.random.default_rng(20261019)
    v = rng.choice([-1., 1.], size=(COUNT, 64)) * 10. ** rng.uniform(-8., 8., size=(COUNT, 64))
    out = np.zeros((COUNT, 6, 64))
    probe.call("reduce", COUNT, v, out)
    rs, rm, sd, sx, md, mx = (out[:, q] for q in range(6))
    for q in range(COUNT):
        for row in range(4):
            sl = slice(16 * row, 16 * row + 16)
            assert len(set(bits(rs[q, sl]).tolist())) == 1 and len(set(bits(rm[q, sl]).tolist())) == 1  # one value per row, bitwise
            assert rm[q, 16 * row] == v[q, sl].max()
        assert same_bits(rs[q], tr.row_sum16_replay(v[q]))  # the four butterflies in their order
        exact, bound = tr.mp_sum(v[q]), 64 * EPS * np.abs(v[q]).sum()
        for s in (sd, sx):
            assert len(set(bits(s[q]).tolist())) == 1
            assert abs(mpmath.mpf(float(s[q, 0])) - exact) <= bound, (q, s[q, 0], exact)
        assert bits(sd[q, :1])[0] == bits(np.array([tr.wave_sum_dpp_replay(v[q])]))[0]  # (r0 + r1) + (r2 + r3) of the row sums
        assert (md[q] == v[q].max()).all() and (mx[q] == v[q].max()).all()  # maxima are exact
    neg = -np.abs(v[:5])  # all negative: a maximum must not start from 0
    out5 = np.zeros((5, 6, 64))
    probe.call("reduce", 5, np.ascontiguousarray(neg), out5)
    assert (out5[:, 4] == neg.max(axis=1, keepdims=True)).all() and (out5[:, 5] == neg.max(axis=1, keepdims=True)).all()
    assert (out5[:, 1].reshape(5, 4, 16) == neg.reshape(5, 4, 16).max(axis=2, keepdims=True)).all()


# ---------------------------------------------------------------- c. fastRcp, fastRsqrt
def mantissas():
    rng = np.random.default_rng(20261020)
    m = [1., np.nextafter(2., 1.), np.nextafter(1., 2.), 1.5, 1.25, 1.75, np.sqrt(2.), np.nextafter(np.sqrt(2.), 1.), 4. / 3., 5. / 3.]
    return np.array(m + list(rng.uniform(1., 2., 16 - len(m))))


def run_rcp(probe, d):
    n = (d.size + 63) // 64
    arg = np.ones(n * 64)
    arg[: d.size] = d.ravel()
    rcp, rsq = np.zeros(n * 64), np.zeros(n * 64)
    probe.call("rcp", n, arg, rcp, rsq)
    return rcp[: d.size].reshape(d.shape), rsq[: d.size].reshape(d.shape)


def test_fast_rcp_rsqrt_one_ulp(probe):
    """1 ulp of the correctly rounded result, derived: the last Newton step is one rounded FMA of a quantity whose relative error is the
    square of an already squared seed error, so any seed good to 2^-14 gives 0.5 ulp plus a binade-edge effect.
    1 / (m 2^k) = (1 / m) 2^-k and 1 / sqrt(m 2^k) = (1 / sqrt(m or 2 m)) 2^-(k div 2) exactly, so mpmath is asked 16 and 32 values and the
    device result, scaled back by its power of two (exact), is compared with each as a sum of two doubles.
    The emulator has no Newton iteration: its stand-ins are 1. / d (correctly rounded: 0.5 ulp) and 1. / sqrt(d), two correctly rounded
    operations -- the square root's relative 2^-53 is up to 1 ulp of a result just below a power of two, plus 0.5 ulp of the division: the
    stand-in's own bar is 1.5 ulp, and only the stand-in gets it."""
    m = mantissas()
    k = np.arange(-510, 511)
    d = np.ldexp(m[:, None], k[None, :])
    rcp, rsq = run_rcp(probe, d)
    worst = {}
    for name, dev, back, ref in (
        ("fastRcp", rcp, k[None, :], [tr.hi_lo(1 / mpmath.mpf(float(x))) for x in m]),
        ("fastRsqrt", rsq, (k // 2)[None, :], None),
    ):
        scaled = np.ldexp(dev, np.broadcast_to(back, dev.shape))  # exact: results are normal and far from the ends
        if ref is None:  # even k: 1 / sqrt(m), odd k: 1 / sqrt(2 m)
            r0 = [tr.hi_lo(1 / mpmath.sqrt(mpmath.mpf(float(x)))) for x in m]
            r1 = [tr.hi_lo(1 / mpmath.sqrt(2 * mpmath.mpf(float(x)))) for x in m]
            hi = np.where(k[None, :] % 2 == 0, np.array([r[0] for r in r0])[:, None], np.array([r[0] for r in r1])[:, None])
            lo = np.where(k[None, :] % 2 == 0, np.array([r[1] for r in r0])[:, None], np.array([r[1] for r in r1])[:, None])
        else:
            hi = np.broadcast_to(np.array([r[0] for r in ref])[:, None], dev.shape)
            lo = np.broadcast_to(np.array([r[1] for r in ref])[:, None], dev.shape)
        err = np.abs((scaled - hi) - lo) / np.spacing(hi)  # in ulps of the correctly rounded result
        worst[name] = float(err.max())
        w = np.unravel_index(np.argmax(err), err.shape)
        print(f"{probe.backend} {name}: worst {err.max():.4f} ulp at m = {m[w[0]]!r}, k = {k[w[1]]}; above 0.5 ulp: {(err > 0.5).mean():.4f} of {err.size}")
    assert worst["fastRcp"] <= 1. and worst["fastRsqrt"] <= (1. if probe.backend == "hip" else 1.5), worst


def test_fast_rcp_rsqrt_domain(probe):
    """The whole exponent range, k in [-1074, 1023]: no accuracy asserted.  Asserted: finite and positive wherever the argument AND the
    true result are normal numbers (fastRsqrt: wherever the argument is normal).  Measured and printed: where the 1 ulp of the test above
    and where finiteness stop (recorded in DESIGN.md section 2)."""
    m = mantissas()
    k = np.arange(-1074, 1024)
    d = np.ldexp(m[:, None], k[None, :])  # (below 2^-1022 the mantissas round to what a subnormal can hold)
    rcp, rsq = run_rcp(probe, d)
    tiny, big = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    with np.errstate(all="ignore"):
        t_rcp = np.longdouble(1) / tr.ld(d)
        t_rsq = np.longdouble(1) / np.sqrt(tr.ld(d))
    for name, dev, true in (("fastRcp", rcp, t_rcp), ("fastRsqrt", rsq, t_rsq)):
        good = np.isfinite(dev) & (dev > 0)
        with np.errstate(all="ignore"):
            ulp = np.abs(tr.ld(dev) - true) / tr.ld(np.spacing(np.minimum(true, big).astype(np.float64)))
        acc = good & (ulp <= 1.)  # (longdouble reference: 2^-11 ulp of its own)
        print(f"{probe.backend} {name}: finite and positive for arguments in [{d[good].min()!r}, {d[good].max()!r}], "
              f"fails inside that range: {int((~good & (d >= d[good].min()) & (d <= d[good].max())).sum())}; "
              f"within 1 ulp for arguments in [{d[acc].min()!r}, {d[acc].max()!r}], "
              f"fails inside that range: {int((~acc & (d >= d[acc].min()) & (d <= d[acc].max())).sum())}")
        normal = (d >= tiny) & (true >= tiny) & (true <= big)
        assert good[normal].all(), (name, d[normal & ~good][:8])


# ---------------------------------------------------------------- d. mm, loads, transposes
def random_tiles(seed, count=COUNT):
    """non-symmetric, entries +-10^U(-3, 3); the second half with row scales 2^+-40"""
    rng = np.random.default_rng(seed)
    t = rng.choice([-1., 1.], size=(count, 16, 16)) * 10. ** rng.uniform(-3., 3., size=(count, 16, 16))
    t[count // 2:] *= np.ldexp(1., rng.choice([-40, 40], size=(count - count // 2, 16, 1)))
    return t


def test_mm(probe):
    X, Y = random_tiles(1), random_tiles(2)
    C0, C1 = np.zeros_like(X), np.zeros_like(X)
    probe.call("mm", COUNT, X, Y, C0, C1)
    for q in range(COUNT):
        # mm(X, Y) = X'Y; through loadTileT both operands arrive transposed: X Y'
        for C, a, b in ((C0[q], X[q].T, Y[q]), (C1[q], X[q], Y[q].T)):
            err = np.abs(tr.ld(C) - tr.matmul_ld(a, b))
            bound = 16 * EPS * tr.matmul_ld(np.abs(a), np.abs(b))
            assert (err <= bound).all(), (q, float((err / bound).max()))


def test_loads_and_transposes(probe):
    X = random_tiles(3)
    X[0, 2, 5], X[0, 7, 7], X[1, 0, 15] = -0., 0., -0.
    nan_payload = np.array([0x7FF8DEADBEEF1234, 0xFFF4000000000001], dtype=np.uint64).view(np.float64)  # a quiet and a signalling NaN
    Xn = X.copy()
    Xn[2, 3, 11], Xn[2, 12, 1], Xn[3, 15, 0] = nan_payload[0], nan_payload[1], np.inf
    out = np.zeros((COUNT, 4, 16, 16))
    probe.call("transpose", COUNT, Xn, out)
    Xt = np.ascontiguousarray(Xn.transpose(0, 2, 1))
    assert same_bits(out[:, 0], Xn)  # storeTile(loadTile(p)) returns p
    assert same_bits(out[:, 1], Xt)  # loadTileT(p) is loadTile of the host-transposed array
    assert same_bits(out[:, 2], Xt)  # the LDS transpose: bitwise, -0.0 and NaN payloads included
    fin = np.isfinite(Xn).all(axis=(1, 2))  # the matrix-core transpose is x * 1 + sum of x' * 0: exact for FINITE tiles only
    assert fin.sum() == COUNT - 2
    assert (out[fin, 3] == Xt[fin]).all()


# ---------------------------------------------------------------- e. mv
def test_mv(probe):
    T, T2 = random_tiles(4), random_tiles(5)
    rng = np.random.default_rng(6)
    x = rng.choice([-1., 1.], size=(COUNT, 16)) * 10. ** rng.uniform(-3., 3., size=(COUNT, 16))
    y1, y2 = np.zeros((COUNT, 64)), np.zeros((COUNT, 64))
    probe.call("mv", COUNT, T, T2, x, y1, y2)
    e = tr.v_elem(np.arange(64))
    assert sorted(np.bincount(e, minlength=16).tolist()) == [4] * 16
    first = np.array([int(np.flatnonzero(e == c)[0]) for c in range(16)])
    for q in range(COUNT):
        for y in (y1[q], y2[q]):
            assert same_bits(y, y[first][e])  # the four lanes that hold one element agree
        a, b = y1[q][first], y2[q][first]
        b1 = 16 * EPS * tr.matmul_ld(np.abs(T[q].T), np.abs(x[q]))
        e1 = np.abs(tr.ld(a) - tr.matmul_ld(T[q].T, x[q]))
        assert (e1 <= b1).all(), (q, float((e1 / b1).max()))
        # chained, nothing re-arranged in between: the second product's own error on the device's first result + the first error carried through
        b2 = 16 * EPS * tr.matmul_ld(np.abs(T2[q].T), np.abs(a)) + tr.matmul_ld(np.abs(T2[q].T), b1)
        e2 = np.abs(tr.ld(b) - tr.matmul_ld(T2[q].T, tr.matmul_ld(T[q].T, x[q])))
        assert (e2 <= b2).all(), (q, float((e2 / b2).max()))


# ---------------------------------------------------------------- f, g. eliminations
def floor_steps(n):
    """j = n - 1 at every n, and j in {0, 3, 4, n - 2} where they exist"""
    return list(dict.fromkeys([n - 1] + [j for j in (0, 3, 4, n - 2) if 0 <= j < n - 1]))


def floored_cases(n, base):
    """(kind, j, matrix): A_jj lowered so that the Schur complement at step j is -0.5 A_jj (pivot = A_jj - c, so A_jj = 2 c / 3 with c what
    the elimination has subtracted: read off the twin); a NaN on a diagonal entry; a NaN on an off-diagonal entry (both of its mirror images)"""
    _, raw = tr.twin(base, n, False)
    cases = []
    for j in floor_steps(n):
        A = base.copy()
        A[j, j] = 2. * (base[j, j] - raw[j]) / 3.
        cases.append(("floor", j, A))
    A = base.copy()
    A[n // 2, n // 2] = np.nan
    cases.append(("nan_diag", n // 2, A))
    if n > 1:
        A = base.copy()
        A[n - 1, 0] = A[0, n - 1] = np.nan
        cases.append(("nan_off", n - 1, A))
    return cases


def elimination(probe, n):
    """one launch per n and backend: the 3 x 8 SPD matrices of (f), then the floored / NaN cases of (g) built on the first of them"""
    if n in probe.cache:
        return probe.cache[n]
    rng = np.random.default_rng(1000 + n)
    spd = [(kappa, tr.spd_matrix(rng, n, kappa)) for kappa in KAPPAS for _ in range(PER_CASE)]
    cases = floored_cases(n, spd[0][1])
    A = np.ascontiguousarray([a for _, a in spd] + [a for _, _, a in cases])
    assert len(A) % 4 != 0
    out, ok = np.zeros((len(A), 4, 16, 16)), np.full(len(A), -1, dtype=np.int32)
    probe.call("invchol", n, len(A), A, out, ok)
    probe.cache[n] = (spd, cases, A, out, ok)
    return probe.cache[n]


def check_structure(Li, n, what):
    assert same_bits(np.triu(Li, 1), np.zeros((16, 16))), what  # above the diagonal: exactly +0
    pad = np.eye(16)
    pad[:n, :n] = Li[:n, :n]
    assert same_bits(Li, pad), what  # rows and columns >= n: the identity


@pytest.mark.parametrize("n", SIZES)
def test_invchol_spd(probe, n):
    """Li = chol(A)^-1 on graded SPD matrices.  The bar on max |Li A Li' - I| (longdouble, from the device's Li) is 8 x the float64 twin's
    residual on the same matrix, floored at 64 eps: with triangularity and a positive diagonal it pins Li uniquely; the 8 covers another
    operation order, FMA contraction and a reciprocal that is not correctly rounded."""
    spd, _, A, out, ok = elimination(probe, n)
    worst = {}
    for q, (kappa, a) in enumerate(spd):
        tw, raw = tr.twin(a, n, False)
        assert (raw > 1e-10 * np.diag(a)[:n]).all()  # precondition, on the reference alone: the floor cannot be in play
        assert (tr.twin(a, n, True)[0] == tw).all()
        Lu, Lf, Lc, LT = out[q]
        assert ok[q] == 1
        assert same_bits(Lu, Lf) and same_bits(Lu, Lc)  # when ok, the unfloored result is bitwise the floored one
        bar = max(8 * tr.residual(tw, a), 64 * EPS)
        for name, Li in (("invCholFactor", Lc), ("invCholFactorT", np.ascontiguousarray(LT.T))):
            check_structure(Li, n, (name, q))
            assert (np.diag(Li) > 0).all()
            res = tr.residual(Li, a)
            key = (name, kappa)
            worst[key] = max(worst.get(key, 0.), res / max(tr.residual(tw, a), 1e-300))
            assert res <= bar, (name, q, kappa, res, bar)
        if q % PER_CASE == 0:  # the mpmath factor itself, on one matrix per kappa: the residual bar pins it, this shows it
            ref = tr.mp_to_f64(tr.inv_chol_mp(a, n))
            scale = np.abs(ref).max(axis=1, keepdims=True)
            e_dev, e_tw = np.abs(Lc - ref) / scale, np.abs(tw - ref) / scale
            assert e_dev.max() <= max(8 * e_tw.max(), 64 * EPS * kappa), (q, e_dev.max(), e_tw.max())
    print(f"{probe.backend} n = {n:2d}: worst residual / twin residual " + ", ".join(
        f"{name} {' / '.join('%.2f' % worst[name, kappa] for kappa in KAPPAS)}" for name in ("invCholFactor", "invCholFactorT")) + "  (kappa = 10 / 1e4 / 1e8)")


@pytest.mark.parametrize("n", SIZES)
def test_invchol_floored(probe, n):
    """The floored path, deterministic by construction: a pivot of -0.5 A_jj, or a NaN.  invCholImpl<n, false> says not ok and invCholFactor
    is bitwise the floored elimination.  A NaN pivot does not reach the rows that were complete before it.
    j = n - 1: nothing follows the floored pivot, row n - 1 is compared with mpmath and the other rows are those of the clean matrix.  j < n - 1: the
    1e14 multipliers make numbers meaningless; finiteness is asserted where the float64 twin of the floored elimination stays below 1e250
    (every further step squares the growth: 1e14, 1e42, 1e98, 1e210, overflow -- a property of the floor, not of the kernel).
    j = 0 is degenerate: the Schur complement at step 0 is A_00 itself, so the construction gives A_00 = 0, pivot and floor are both 0 and the
    reciprocal is infinite -- the floor is relative to the diagonal and cannot rescue a diagonal that is not positive."""
    spd, cases, A, out, ok = elimination(probe, n)
    base_out = out[0]
    for c, (kind, j, a) in enumerate(cases):
        q = len(spd) + c
        Lu, Lf, Lc, LT = out[q]
        what = (kind, j)
        assert ok[q] == 0, what
        assert same_bits(Lc, Lf), what
        check_structure(Lc, n, what)
        check_structure(np.ascontiguousarray(LT.T), n, what)
        if kind == "nan_diag":
            # Step j touches only the registers with a row below the pivot (4 r + 3 > j): the rows of the registers that lie entirely at or above
            # it were complete before the NaN entered, and stay what they are on the clean matrix -- also next to a register boundary (j & 3 == 3)
            done = min(j, 4 * ((j + 1) // 4))
            assert same_bits(Lc[:done], base_out[2][:done]) and same_bits(Lu[:done], base_out[0][:done]), what
        if kind != "floor" or j == 0:
            continue
        tw, _ = tr.twin(a, n, True)
        if j < n - 1:
            if np.isfinite(tw).all() and np.abs(tw).max() < 1e250:
                assert np.isfinite(Lc).all() and np.isfinite(LT).all(), what
            continue
        assert np.isfinite(Lc).all() and np.isfinite(LT).all(), what
        assert same_bits(Lc[: n - 1], base_out[2][: n - 1]) and same_bits(LT[:, : n - 1], base_out[3][:, : n - 1])  # the other rows are unaffected
        ref = tr.mp_to_f64(tr.gauss_mp(a, n, True))[n - 1]
        e_tw = np.abs(tw[n - 1] - ref).max() / np.abs(ref).max()
        bar = max(8 * e_tw, 64 * EPS)
        for name, row in (("invCholFactor", Lc[n - 1]), ("invCholFactorT", LT[:, n - 1])):
            e = np.abs(row - ref).max() / np.abs(ref).max()
            assert e <= bar, (name, what, e, bar)


def test_reference_agrees_with_itself():
    """the two mpmath routes to chol(A)^-1 (Cholesky + triangular inverse; elimination on [A | I]) and the twin agree"""
    rng = np.random.default_rng(7)
    for n in (1, 5, 16):
        a = tr.spd_matrix(rng, n, 1e4)
        r0, r1 = tr.mp_to_f64(tr.inv_chol_mp(a, n)), tr.mp_to_f64(tr.gauss_mp(a, n, False))
        assert np.abs(r0 - r1).max() <= 4 * EPS * np.abs(r0).max()
        assert tr.residual(r0, a) < 64 * EPS
        assert tr.residual(tr.twin(a, n, False)[0], a) < 1e-10

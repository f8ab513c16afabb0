"""The block-tridiagonal KKT sweeps of the interior-point solver (csrc/sweeps.h: factor, forward, backward), alone: each system the sweeps are
handed is solved again by references that share nothing with them (sweep_reference.py: mpmath, a longdouble residual, a float64 twin).

Every test runs on the wave emulator (`emu`: checks the harness, the reference and the algebra) and on the device (`hip`, marked gpu: the raw buffer
instructions whose out-of-pattern lanes rely on the hardware's range check, the 4x4x4 matrix-core path of the vector sweeps and its DPP broadcasts,
none of which the emulator has).  The kernel is that of tests/sweep_probe/sweep_probe.cpp: the product's geometry, one wavefront per system, systems of
all four models and of different horizons in one launch, every record block a slice of one arena whose other bytes hold a sentinel.

A launch sequence per population (`Run`): factor (n = 2 in SC mode, n = 1 in SCvx mode), resolve on the unchanged right-hand side, then a new
right-hand side and a resolve with n = 1 and, in SC mode, with n = 2; once through the sweeps the product selects and once through the tile form."""
import ctypes
import os

import numpy as np
import pytest

import sweep_reference as sr
from sweep_reference import EPS, NV

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
MODELS = ["RocketQuatSC", "Rocket2dSC", "Lander3dofSC", "ZeroOrderHold<RocketQuatSC>"]
OFF_N = 8  # (the probe's enum Offs)
O_SX, O_FAC, O_SV, O_A, O_B, O_C, O_IP, O_UNUSED = range(8)
SENTINEL = np.uint64(0x7FF4DEADBEEF0000)  # a signalling NaN; the low 16 bits carry the position
STEPS = ("factor", "resolve_same", "resolve_n1", "resolve_n2")


class Probe:
    def __init__(self, path, backend):
        self.backend = backend
        self.lib = ctypes.CDLL(path)
        self.lib.sweep_probe_layout_names.restype = ctypes.c_char_p
        self.runs = {}
        self._lay = {}

    def layout(self, model):
        if model not in self._lay:
            out = np.zeros(self.lib.sweep_probe_layout_count(), dtype=np.int32)
            assert self.lib.sweep_probe_layout(model, out.ctypes.data_as(ctypes.c_void_p)) == 0
            names = self.lib.sweep_probe_layout_names().decode().split()
            lay = {n: int(out[i]) for i, n in enumerate(names)}
            p = len(names)
            lay["PAT"] = out[p:p + 256].reshape(16, 16).astype(np.int64)
            lay["XMAP"] = out[p + 256:p + 272].tolist()
            lay["UMAP"] = out[p + 272:p + 288].tolist()
            assert p + 288 == len(out)
            self._lay[model] = lay
        return self._lay[model]

    def fixed_masks(self, model, K):
        fm = [self.lib.sweep_probe_fixed_mask(model, k, K) for k in range(K)]
        assert min(fm) >= 0
        return fm

    def run(self, desc, offs, arena):
        assert desc.dtype == np.int32 and offs.dtype == np.int64 and arena.dtype == np.float64
        rc = self.lib.sweep_probe_run(len(desc), desc.ctypes.data_as(ctypes.c_void_p), offs.ctypes.data_as(ctypes.c_void_p),
                                      arena.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(arena.size))
        assert rc == 0, rc


@pytest.fixture(scope="module", params=BACKENDS)
def probe(request):
    """the probe library of the emulation build or of the device build"""
    import __graft_entry__ as g

    if request.param == "emu":
        return Probe(os.environ.get("SCPP_SWEEP_PROBE_EMU_LIBRARY") or g.build_sweep_probe_emu(), "emu")
    lib = os.environ.get("SCPP_SWEEP_PROBE_LIBRARY") or g.SWEEP_PROBE_LIB
    if not os.path.exists(lib):
        g.build_sweep_probe()
    return Probe(lib, "hip")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def canon(a):
    """bit patterns with the position taken out of the sentinels: blocks at different places of an arena, or of two arenas, compare equal"""
    b = bits(a).copy()
    b[(b & ~np.uint64(0xFFFF)) == SENTINEL] = SENTINEL
    return b


# ---------------------------------------------------------------- the cases and their references (computed once, shared by both backends)
def case_keys(late):
    """(model, K, scvx, late): K = 3 .. 8 for every model -- both residues of the two-fold unrolled factor loop, all three of the three buffers of
    the substitution sweeps, K = 3 the smallest horizon the ABI admits -- and K = 50, 64 for RocketQuat; SC and SCvx mode"""
    keys = [(m, K, scvx, late) for m in range(4) for K in range(3, 9) for scvx in (False, True)]
    return keys + [(0, K, scvx, late) for K in (50, 64) for scvx in (False, True)]


class Case:
    """a system, its new right-hand side and what the references say about both"""

    def __init__(self, probe, key):
        model, K, scvx, late = key
        self.key = key
        lay = probe.layout(model)
        # (the seed: the first of 20261101, 20261102, ... at which the TWIN's residual stays a factor 10 below the 1e-6 of test_inputs_are_admissible
        #  on every system and column -- 8.6e-8 at worst; chosen on the twin alone, before any kernel ran on these systems)
        rng = np.random.default_rng([20261103, model, K, int(scvx), int(late)])
        self.sys = sr.generate(model, lay, probe.fixed_masks(model, K), K, scvx, late, rng)
        self.new = sr.new_rhs(self.sys, rng)
        self.blocks = sr.blocks(self.sys)
        self.twin = sr.Twin(self.blocks)
        self.cols = {}  # (which right-hand side, border) -> (beta, rho, twin x, twin lam, twin's worst residual)
        for which, s in (("orig", self.sys), ("new", self.new)):
            for border in self.borders():
                beta, rho = sr.rhs(s, border)
                x, lam = self.twin.solve(beta, rho)
                self.cols[which, border] = (beta, rho, x, lam, sr.worst(*sr.residual(self.blocks, beta, rho, x, lam)))
        # the twin's residual ON THIS SYSTEM: the worst of the columns it solved on it.  (One column's figure is one draw of a rounding error that the
        # explicit inverses amplify: between two float64 runs of the same recursion -- the twin and the emulated kernel -- the column-by-column
        # quotient scatters from 0.02 to 29 over these populations; the quotient to the system's figure stays below 5.2 there and 5.6 on the device.)
        self.res_tw = max(c[4] for c in self.cols.values())
        self._mp = None

    def borders(self):
        """the columns the mode has: the regular one (False) and, in SC mode, the sigma border (True)"""
        return (False,) if self.sys.scvx else (False, True)

    def mp(self):
        """50-digit solutions of the original right-hand side: {border: (x, lam)}"""
        if self._mp is None:
            self._mp = dict(zip(self.borders(), sr.solve_mp(self.blocks, [self.cols["orig", b][:2] for b in self.borders()])))
        return self._mp

    def label(self):
        m, K, scvx, late = self.key
        return f"{MODELS[m]} K={K} {'SCvx' if scvx else 'SC'} {'late' if late else 'benign'}"


CASES = {}


def get_case(probe, key):
    if key not in CASES:
        CASES[key] = Case(probe, key)
    return CASES[key]


# ---------------------------------------------------------------- the arena
class Arena:
    """record blocks of the jobs as slices of one array of doubles; every other entry holds the sentinel"""

    def __init__(self, jobs):
        """jobs: [(Case, form)]"""
        self.jobs = jobs
        rng = np.random.default_rng(5)
        offs, pos = np.zeros((len(jobs), OFF_N), dtype=np.int64), 16
        self.sizes = []
        for q, (case, _) in enumerate(jobs):
            lay, K = case.sys.lay, case.sys.K
            size = [K * lay["XREC"], K * lay["FACREC"], K * lay["SVREC"], (K - 1) * lay["NX"] ** 2, (K - 1) * lay["NX"] * lay["NU"],
                    (K - 1) * lay["NX"] * lay["NU"], lay["IP_N"], 16]
            for f in range(OFF_N):
                if f in (O_SX, O_FAC, O_SV):  # the record blocks start on a 128-byte line, as the product's do
                    pos = (pos + 15) & ~15
                offs[q, f] = pos
                pos += size[f] + int(rng.integers(1, 24))
            self.sizes.append(size)
        self.offs = offs
        self.a = np.zeros(pos + 16)
        bits(self.a)[:] = SENTINEL | (np.arange(self.a.size, dtype=np.uint64) & np.uint64(0xFFFF))
        self.inside = np.zeros(self.a.size, dtype=bool)  # inside a record block
        for q, (case, _) in enumerate(jobs):
            for f in range(OFF_N - 1):
                self.inside[offs[q, f]:offs[q, f] + self.sizes[q][f]] = True
            self.write_inputs(q, case.sys, everything=True)

    def sx(self, q):
        case = self.jobs[q][0]
        return self.a[self.offs[q, O_SX]:][:self.sizes[q][O_SX]].reshape(case.sys.K, case.sys.lay["XREC"])

    def block(self, q, f):
        return self.a[self.offs[q, f]:][:self.sizes[q][f]]

    def write_inputs(self, q, s, everything=False):
        """what the phases would hand over; the fields no sweep reads keep the sentinel: the solution fields, the gaps of the record, the
        multiplier entries beyond NL and stage K-1's segment fields (there is no segment K-1)"""
        lay, K = s.lay, s.K
        NL, sx = lay["NL"], self.sx(q)
        sx[:, lay["X_BETA"]:][:, :NV] = s.beta
        for name, v in (("X_RHO", s.rho), ("X_S", s.S)):
            sx[:K - 1, lay[name]:][:, :NL] = v[:K - 1, :NL]
        if not everything:
            return
        sx[:K - 1, lay["X_EINV"]:][:, :NL] = s.einv[:K - 1, :NL]
        sx[:, lay["X_HS"]:][:, :lay["HS_N"]] = s.hs[:, :lay["HS_N"]]
        sx[:, lay["X_HC"]] = s.e2
        sx[:, lay["X_HC"] + 1] = s.cc
        sx[:, lay["X_WBT"]:][:, :NV] = s.wbt
        self.block(q, O_A)[:] = s.A.ravel()
        self.block(q, O_B)[:] = s.B.ravel()
        self.block(q, O_C)[:] = s.C.ravel()
        self.block(q, O_IP)[lay["IP_SCVX"]] = 1. if s.scvx else 0.

    def allowed(self, q, n, factor):
        """mask of the entries job q may write: the solution fields of the n columns asked for, the saved columns of those n, and, in a
        factorisation, the packed factors (nothing of stage K-1 beyond Li and a: it has no segment)"""
        case = self.jobs[q][0]
        lay, K = case.sys.lay, case.sys.K
        NL = lay["NL"]
        m = np.zeros(self.a.size, dtype=bool)
        sx = m[self.offs[q, O_SX]:][:self.sizes[q][O_SX]].reshape(K, lay["XREC"])
        sx[:, lay["X_VW"]:][:, :NV] = True
        sx[:K - 1, lay["X_VL"]:][:, :NL] = True
        if n == 2:
            sx[:, lay["X_BCW"]:][:, :NV] = True
            sx[:K - 1, lay["X_BCL"]:][:, :NL] = True
        sv = m[self.offs[q, O_SV]:][:self.sizes[q][O_SV]].reshape(K, lay["SVREC"])
        sv[:, :n * 16] = True
        sv[:K - 1, lay["NRHS_MAX"] * 16:][:, :n * 16] = True
        if factor:
            fac = m[self.offs[q, O_FAC]:][:self.sizes[q][O_FAC]].reshape(K, lay["FACREC"])
            fac[:, lay["FAC_LI"]:][:, :NV * (NV + 1) // 2] = True
            fac[:K - 1, lay["FAC_YT"]:lay["FAC_TI"] + NL * (NL + 1) // 2] = True
        return m

    def solution(self, q, border):
        """(x [K][16], lam [K-1][NL]) of the regular or the border column"""
        case = self.jobs[q][0]
        lay, K = case.sys.lay, case.sys.K
        sx = self.sx(q)
        w, l = ("X_BCW", "X_BCL") if border else ("X_VW", "X_VL")
        return sx[:, lay[w]:][:, :NV].copy(), sx[:K - 1, lay[l]:][:, :lay["NL"]].copy()


def mode_n(case):
    return 1 if case.sys.scvx else 2


class Run:
    """the launch sequence on one list of jobs: snapshots of the arena before the first and after every launch"""

    def __init__(self, probe, jobs):
        self.arena = ar = Arena(jobs)
        self.snap = {"start": ar.a.copy()}
        self.n = {}
        for step in STEPS:
            if step == "resolve_n1":
                for q, (case, _) in enumerate(jobs):
                    ar.write_inputs(q, case.new)
                self.snap["new_rhs"] = ar.a.copy()
            # (SCvx mode has no sigma border, n = 1 throughout: a border column is not defined there -- the state rows of H vanish, and with beta = 0
            #  a row of the system can consist of one multiplier alone)
            self.n[step] = [mode_n(c) if step != "resolve_n1" else 1 for c, _ in jobs]
            desc = np.array([[c.key[0], c.sys.K, self.n[step][q], 0 if step == "factor" else 1, form] for q, (c, form) in enumerate(jobs)], dtype=np.int32)
            probe.run(desc, ar.offs, ar.a)
            self.snap[step] = ar.a.copy()
        self.before = {"factor": "start", "resolve_same": "factor", "resolve_n1": "new_rhs", "resolve_n2": "resolve_n1"}

    def at(self, step):
        """the arena as it was after `step`"""
        v = Arena.__new__(Arena)
        v.__dict__.update(self.arena.__dict__)
        v.a = self.snap[step]
        return v


def population(probe, late, form=0):
    key = ("population", late, form)
    if key not in probe.runs:
        probe.runs[key] = Run(probe, [(get_case(probe, k), form) for k in case_keys(late)])
    return probe.runs[key]


def columns_of(run, step, q):
    """[(which right-hand side, border)] of the columns job q solved at `step`"""
    which = "orig" if step in ("factor", "resolve_same") else "new"
    return [(which, False)] + ([(which, True)] if run.n[step][q] == 2 else [])


# ---------------------------------------------------------------- the condition on the inputs (not a measurement)
@pytest.mark.parametrize("late", [False, True], ids=["benign", "late"])
def test_inputs_are_admissible(probe, late):
    """on every generated system the float64 twin factors with all pivots positive and its relative residual is below 1e-6, for every column any
    test solves: asserted of the twin, before anything looks at the device; no case is dropped"""
    for key in case_keys(late):
        case = get_case(probe, key)
        assert case.twin.pivots_ok, case.label()
        for col, (_, _, x, lam, res) in case.cols.items():
            assert np.isfinite(x).all() and np.isfinite(lam).all() and res < 1e-6, (case.label(), col, res)


# ---------------------------------------------------------------- a. solution against mpmath
def small_keys():
    return [(m, K, scvx, False) for m in range(4) for K in (3, 4) for scvx in (False, True)]


@pytest.mark.parametrize("model", range(4), ids=MODELS)
def test_solution_against_mpmath(probe, model):
    """K = 3, 4, both modes, benign population: every entry of X_VW, X_VL (and X_BCW, X_BCL where the mode has a border) within the bar of the
    50-digit solution, relative to the largest entry of that field at that stage.  Bar: 100 x the twin's own error in that field on the same
    system (what tests/mpc_compare.py gives a device over a float64 twin's rounding floor), floored at 64 eps."""
    run = population(probe, False)
    ar = run.at("factor")
    ratios = []
    for q, (case, _) in enumerate(ar.jobs):
        if case.key not in small_keys() or case.key[0] != model:
            continue
        # the twin's own error on this system, per field: the worst stage of the worst column
        e_tw = [max(float(sr.stage_error(case.cols["orig", b][2 + f], case.mp()[b][f]).max()) for b in case.borders()) for f in (0, 1)]
        for which, border in columns_of(run, "factor", q):
            for f, name in enumerate(("w", "lam")):
                e_dev = sr.stage_error(ar.solution(q, border)[f], case.mp()[border][f])
                bar = max(100. * e_tw[f], 64 * EPS)
                ratios.append(float(np.nan_to_num(e_dev, nan=np.inf).max()) / max(e_tw[f], 64 * EPS / 100.))
                assert (e_dev <= bar).all(), (case.label(), "border" if border else "regular", name, "stage %d" % int(np.argmax(~(e_dev <= bar))),
                                              float(np.nanmax(e_dev)), bar)
    assert len(ratios) == 2 * (2 * 2 + 2 * 1)  # per K: SC has two columns, SCvx one; two fields each
    print(f"{probe.backend} {MODELS[model]}: largest error against mpmath / twin's error = {max(ratios):.2f}")


# ---------------------------------------------------------------- b, c. residual on every case, every launch
def check_residuals(probe, late, model, step):
    run = population(probe, late)
    ar = run.at(step)
    worst, failures = {}, []
    for q, (case, _) in enumerate(ar.jobs):
        if case.key[0] != model:
            continue
        for which, border in columns_of(run, step, q):
            beta, rho, res_tw = case.cols[which, border][0], case.cols[which, border][1], case.res_tw
            x, lam = ar.solution(q, border)
            qx, ql = sr.residual(case.blocks, beta, rho, x, lam)
            bar = max(8. * res_tw, 64 * EPS)
            mode = "SCvx" if case.key[2] else "SC"
            worst[mode] = max(worst.get(mode, 0.), sr.worst(qx, ql) / max(res_tw, 8 * EPS))
            over = sr.first_over(qx, ql, bar)
            if over is not None:
                failures.append(f"{case.label()} {step} {'border' if border else 'regular'} column: {over} (twin {res_tw:.3e})")
    print(f"{probe.backend} {'late' if late else 'benign'} {MODELS[model]} {step}: worst residual / twin's residual " + ", ".join(f"{m} {v:.2f}" for m, v in sorted(worst.items())))
    assert not failures, failures


@pytest.mark.parametrize("model", range(4), ids=MODELS)
@pytest.mark.parametrize("late", [False, True], ids=["benign", "late"])
def test_residual_of_the_factorisation(probe, late, model):
    """max |T x - b| scaled row by row by |T| |x| + |b| (longdouble, from the device's x), for each column: at most 8 x the twin's on the same system
    (Case.res_tw), floored at 64 eps -- the bar test_tile_engine.py holds the eliminations to (5.8 x measured there).  A failure names the first stage and row over it."""
    check_residuals(probe, late, model, "factor")


@pytest.mark.parametrize("model", range(4), ids=MODELS)
@pytest.mark.parametrize("late", [False, True], ids=["benign", "late"])
@pytest.mark.parametrize("step", STEPS[1:])
def test_residual_of_a_resolve(probe, late, model, step):
    """forward + backward sweep on the factor record an earlier launch left: the unchanged right-hand side (not bitwise the fused result -- the
    forward sweep forms N'(Ti' c), the fused pass Z' c -- but inside the same bar), then a new one with n = 1 and, in SC mode, n = 2.  The packed
    factors and the saved columns are complete and re-read at the right offsets, or the residual against the new right-hand side shows it."""
    check_residuals(probe, late, model, step)


# ---------------------------------------------------------------- d. tile form = vector form, bitwise
@pytest.mark.parametrize("late", [False, True], ids=["benign", "late"])
def test_tile_form_equals_vector_form(probe, late):
    """sweeps.h: 'results are BITWISE those of the tile sweeps' -- the four solution fields and the whole saved-column record, after the fused
    factorisation (n = 2 in SC mode, n = 1 in SCvx mode) and after forward + backward sweeps with n = 1 and n = 2"""
    vec, til = population(probe, late, 0), population(probe, late, 1)
    diff = []
    for step in STEPS:
        a, b = vec.at(step), til.at(step)
        assert np.array_equal(a.offs, b.offs)
        for q, (case, _) in enumerate(a.jobs):
            for name, u, v in (("sx", a.sx(q), b.sx(q)), ("sv", a.block(q, O_SV), b.block(q, O_SV)), ("fac", a.block(q, O_FAC), b.block(q, O_FAC))):
                ne = bits(u) != bits(v)
                if ne.any():
                    w = np.argwhere(ne)[0]
                    with np.errstate(all="ignore"):
                        ulp = np.abs(u[ne] - v[ne]) / np.spacing(np.abs(u[ne]))
                    diff.append(f"{case.label()} {step} {name}: {int(ne.sum())} entries differ, first at {w.tolist()}, up to {np.nanmax(ulp):.1f} ulp")
    assert not diff, diff[:8]


# ---------------------------------------------------------------- e. structure
def outside_entries(s, rng):
    """a copy of system s that differs only where no sweep may read: input columns >= NUV and state columns outside XMAP; the A / B column of a
    variable fixed at k; the C column of a variable fixed at k + 1; the X_HS entries in a row or column of a variable fixed at k; the state
    block of wbt in SCvx mode and wbt of a fixed variable"""
    lay, K = s.lay, s.K
    t = s.copy()
    NXV, NVU, pat = lay["NXV"], lay["NVU"], lay["PAT"]
    xcols, ucols = lay["XMAP"][:NXV], lay["UMAP"][:NVU - NXV]
    n = 0
    for k in range(K):
        f = s.fixed(k)
        for j in range(NV):
            if f[j] or (s.scvx and j < NXV):
                t.wbt[k, j] = rng.standard_normal()
                n += 1
        for a_ in range(NV):
            for b_ in range(NV):
                if pat[a_, b_] >= 0 and (f[a_] or f[b_]):
                    t.hs[k, pat[a_, b_]] = rng.standard_normal()
                    n += 1
        if k == K - 1:
            break
        fn = s.fixed(k + 1)
        for c in range(lay["NX"]):
            if c not in xcols or f[xcols.index(c)]:
                t.A[k, :, c] = rng.standard_normal(lay["NX"])
                n += 1
        for c in range(lay["NU"]):
            if c not in ucols or f[NXV + ucols.index(c)]:
                t.B[k, :, c] = rng.standard_normal(lay["NX"])
                n += 1
            if c not in ucols or fn[NXV + ucols.index(c)]:
                t.C[k, :, c] = rng.standard_normal(lay["NX"])
                n += 1
    assert n > 0
    return t


def structure_keys():
    """one system per model and mode at K = 3 .. 8 in turn, late population, and RocketQuat at K = 50: 13 systems"""
    keys = [(m, 3 + (2 * m + int(scvx)) % 6, scvx, True) for m in range(4) for scvx in (False, True)]
    return keys + [(0, 50, False, True), (0, 7, True, False), (3, 4, False, False), (1, 6, False, False), (2, 3, True, False)]


def outputs_equal(a, qa, b, qb):
    return all(np.array_equal(canon(a.block(qa, f)), canon(b.block(qb, f))) for f in (O_SX, O_FAC, O_SV))


def test_pattern_zeros_are_not_read(probe):
    """two systems that differ only in entries outside what the sweeps may read give bitwise equal records, after every launch"""
    rng = np.random.default_rng(11)
    jobs = []
    for key in structure_keys()[:8]:
        case = get_case(probe, key)
        twin_case = Case.__new__(Case)
        twin_case.__dict__.update(case.__dict__)
        twin_case.sys = outside_entries(case.sys, rng)
        twin_case.new = case.new
        jobs += [(case, 0), (twin_case, 0)]
    run = Run(probe, jobs)
    for step in STEPS:
        ar = run.at(step)
        for q in range(0, len(jobs), 2):
            sx0, sx1 = ar.sx(q).copy(), ar.sx(q + 1).copy()
            lay = jobs[q][0].sys.lay
            for lo, n in ((lay["X_HS"], lay["HS_N"]), (lay["X_WBT"], NV)):  # (the inputs that differ on purpose)
                sx0[:, lo:lo + n] = sx1[:, lo:lo + n] = 0.
            assert np.array_equal(canon(sx0), canon(sx1)), (jobs[q][0].label(), step)
            for f in (O_FAC, O_SV):
                assert np.array_equal(canon(ar.block(q, f)), canon(ar.block(q + 1, f))), (jobs[q][0].label(), step, f)


def test_independent_of_the_neighbours(probe):
    """a system's records are bitwise the same alone in a launch and inside a mixed launch of 13 systems"""
    keys = structure_keys()
    assert len(keys) == 13 and len(set(keys)) == 13
    cases = [get_case(probe, k) for k in keys]
    mixed = Run(probe, [(c, 0) for c in cases])
    for q in (0, 5, 8, 12):
        alone = Run(probe, [(cases[q], 0)])
        for step in STEPS:
            assert outputs_equal(mixed.at(step), q, alone.at(step), 0), (cases[q].label(), step)


@pytest.mark.parametrize("late", [False, True], ids=["benign", "late"])
def test_nothing_else_is_written(probe, late):
    """after every launch: every sentinel outside the record blocks, A, B, C, ip and every entry of sx, fac and sv that the launch was not asked to
    produce are bitwise what they were before it; with n = 1 the border fields X_BCW / X_BCL keep what they held"""
    for form in (0, 1):
        run = population(probe, late, form)
        ar = run.arena
        for step in STEPS:
            before, after = run.snap[run.before[step]], run.snap[step]
            may = np.zeros(ar.a.size, dtype=bool)
            for q in range(len(ar.jobs)):
                may |= ar.allowed(q, run.n[step][q], step == "factor")
            assert not (may & ~ar.inside).any()
            changed = bits(before) != bits(after)
            bad = np.flatnonzero(changed & ~may)
            assert bad.size == 0, (form, step, bad[:8].tolist(), [int(np.searchsorted(ar.offs[:, 0], b, side="right")) - 1 for b in bad[:8]])
            if step == "factor":  # and what it was asked to produce has been produced: no sentinel is left there
                left = np.flatnonzero(may & ((bits(after) & ~np.uint64(0xFFFF)) == SENTINEL))
                assert left.size == 0, (form, left[:8].tolist())


def test_fixed_variables_return_beta(probe):
    """the identity rows: x_j = beta_j on fixed and padding variables.  The twin returns it BITWISE (read off the twin here: the pivot of such a row is
    exactly 1, its multipliers exactly 0), so the same is asserted of the sweeps, for the regular column (beta) and the border column (0)"""
    for late in (False, True):
        run = population(probe, late)
        for step in STEPS:
            ar = run.at(step)
            for q, (case, _) in enumerate(ar.jobs):
                f = np.array([case.sys.fixed(k) for k in range(case.sys.K)])
                for which, border in columns_of(run, step, q):
                    beta, _, tx, _, _ = case.cols[which, border]
                    assert np.array_equal(bits(tx[f] + 0.), bits(beta[f] + 0.)), (case.label(), "twin")
                    x, _ = ar.solution(q, border)
                    assert np.array_equal(bits(x[f] + 0.), bits(beta[f] + 0.)), (case.label(), step, border)  # (+ 0.: -0 and +0 are the same zero)


# ---------------------------------------------------------------- f. the reference against itself (CPU only)
def test_reference_agrees_with_itself():
    """on every small case the twin, the longdouble residual and mpmath agree -- a defect of the reference is not read as one of the kernel: the
    50-digit solution has a residual at the rounding of its float64 copy; the twin is within its own conditioning of it; the stage-wise residual
    is the dense one; L D L' and mpmath's pivoted LU give the same digits"""
    import __graft_entry__ as g

    probe = Probe(os.environ.get("SCPP_SWEEP_PROBE_EMU_LIBRARY") or g.build_sweep_probe_emu(), "emu")
    for key in small_keys():
        case = get_case(probe, key)
        T, n0 = sr.dense(case.blocks)
        assert np.array_equal(T, T.T)
        for border in case.borders():
            beta, rho, tx, tl, res_tw = case.cols["orig", border]
            mx, ml = case.mp()[border]
            qx, ql = sr.residual(case.blocks, beta, rho, mx, ml)
            assert sr.worst(qx, ql) <= 4 * EPS, (case.label(), border, sr.worst(qx, ql))
            v, c = sr.pack(mx, ml), sr.pack(beta, rho)
            with np.errstate(all="ignore"):
                r = np.abs(sr.ld(T) @ sr.ld(v) - sr.ld(c))
                r = np.where(r == 0, 0, r / (np.abs(sr.ld(T)) @ np.abs(sr.ld(v)) + np.abs(sr.ld(c))))
            assert abs(float(r.max()) - sr.worst(qx, ql)) <= 0.05 * EPS  # the stage-wise residual is the dense one (to longdouble's own rounding)
            assert res_tw < 1e-6
            for tw, ref in ((tx, mx), (tl, ml)):
                assert float(sr.stage_error(tw, ref).max()) < 1e-6, case.label()
    key = (1, 3, True, False)
    case = get_case(probe, key)
    cols = [case.cols["orig", b][:2] for b in case.borders()]
    for (x0, l0), (x1, l1) in zip(case.mp().values(), sr.solve_mp(case.blocks, cols, lu=True)):
        assert np.array_equal(x0, x1) and np.array_equal(l0, l1)

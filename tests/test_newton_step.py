"""ONE iteration of the interior-point loop (csrc/ipm_solve.h: ipmSolveInstance) and its once-per-solve start points, alone, on the wave emulator (`emu`)
and on the device (`hip`, marked gpu), through tests/step_probe/step_probe.cpp: the product's geometry, one wavefront per instance, EVERY block of a Ctx a
slice of one arena, the phases called in the order and with the early exits of the solve's text.  What connects the separately tested pieces (tile engine,
sweeps, cone steps, residual pass, constraint rows) into a Newton step -- buildHs / addConeHs with the delta_k elimination and the sigma block, the two
right-hand sides with their condensation of nu, nu_b, delta_k, the sigma border's Schur complement through two wave sums, the recovery of the eliminated
variables, ds and dz, the step lengths and the centring parameter from wave-wide maxima, the cold and warm start points -- is held to the problem it
claims to solve: the Newton system of the literal cone program, assembled as explicit matrices and solved at high precision by tests/newton_reference.py,
which shares nothing with the kernel's condensation (see its docstring for the equations, the signs and how it is solved).

Instances: the phase tests' `draw` (imported), population `benign` (cone margins 10^U(-2, 0)): four models x K in (3, 4) x SC / SCvx x 3 instances, and
RocketQuat at K = 50, 63, 64 (every lane live but one, lane 63 without a segment, the odd record pitch), all jobs of a mode in ONE launch (27 wavefronts).
Drawn once per module, references computed once per case and shared by both backends and all tests.  Instance 2 of some cells has ONE cone re-drawn until
a cone of a wanted kind binds a step length (FORCE).  Population `late` (tests 3, 4, 5), the same cells: an INTERIOR late iterate -- s z about 1e-10,
rz at 1e-9, ry and rx at 1e-8 of their terms, every cone pair strictly inside -- built by newton_late.py on instances of draw of its own
(test_phase_residuals.make_late's points lie outside the cones: bad = 1); there alpha is 0.7 .. 0.999, against 3e-4 .. 5e-3 on `benign`.  Everything an op does not read holds a distinct quiet NaN -- but for the rows of s, z, ds, dz
that belong to a cone or LP row a stage does not have: the phases load those with the rest of the stage vector and mask them through their content,
the zeros phSetup left (test_footprint says what was measured and what is asserted of them instead).
The reference: K = 3, 4 the literal system stated and solved in mpmath (newton_reference.MpNewton: phase_reference's mpmath rows, cone_reference.nt_scaling,
45 digits), K = 50, 63, 64 the float64 solve refined with longdouble residuals; test 1 holds the second to the first on every small instance.
SCvx mode: the sweeps' static dual regularisation (1e-9 on the multiplier block, stated by sweep_reference.DUAL_REG) is part of the system the chain solves,
so it is part of the reference's: E dx - reg dy = -om ry.

What is compared with what, and where each bar comes from
 1. test_populations_on_the_reference (no kernel): conditions on the instances.  The twin's error on every field <= 1e-6 of the field's largest entry; at
    least a third of the instances have alpha_p, alpha_d strictly inside (1e-8, 0.999) and different, at least a third sigma strictly inside (1e-4, 1); a
    stage cone, a stage LP row, a segment LP row and a wave-uniform row (ss and sc3; not s3, see FORCE) each bind a step length at least once; in SC mode
    an instance has dsig and ddsg above 1e-3 of |dx|; the longdouble cone algebra agrees with cone_reference's mpmath; at K = 3, 4 the refined
    longdouble solve is within a tenth of the twin's error (a thousandth of test 3's bar) of the mpmath solve, per field, predictor and corrector.
 2. test_predictor_blocks_and_centring (PREDICT): sigma_c against the reference's sigma, bar max(100 x |the twin's sigma - sigma|, 64 u); F_HDD, F_HDW,
    X_HS (mapped through PAT: the one place PAT is used, it takes no part in arithmetic), Hsd, Hdd, hsig against the blocks of G'W^-2 G formed from the
    reference's W: sums of products, bar (n + 1) u T with T carried by the reference, plus the scaling's own error 2 (D + 8) u (kappa(s) + kappa(z)) T
    (test_cone_math.py: nt_scaling's c(D) and amplification; doubled for the square); X_HC = {1 / eta^2, 2 / (2 w0^2 - 1)} at the scaling's bar (the
    second times the condition of its difference).  `schur` (SC mode) against the Schur complement of sigma in the literal system's matrix, stated
    without any elimination as 1 / (M^-1)[sigma, sigma], at the bar rule of test 3 with its own twin.  sigma_c is held to the twin rule here, not to the
    composite step-length bar of test 5 from the stored predictor direction (left out, see below).
 3. test_direction_against_the_literal_system (ITER): F_DW, F_DDL, F_DS, F_DZ, the thirteen wave-uniform directions, and dnu, dnu_b, dlam, ds1, dz1,
    ds2, dz2 entrywise against the literal solution.  The corrector stores no segment direction (phUpdate recomputes it), so those are recovered from the
    ITER_STEP point as (new - old) / alpha, with the 2 u (|x| + |alpha dx|) / alpha that costs added to the bar.  Bar per field: max(100 x the twin's
    largest error on that field, 64 u x the field's largest reference entry), the rule test_sweeps.py holds the eliminations to; each of the thirteen
    wave-uniform directions is a field of its own.  (G_DNU, G_DNUB, G_DLAM are written by neither PREDICT nor ITER: asserted.)  Fixed variables:
    exactly 0.  Masked reads: see the comment in the test.
 4. test_iteration_in_residual_form (ITER_STEP and ITER_FUSED, on `late` and on `benign`): rx, ry, rz of the literal problem at the stored point
    against (1 - alpha om) r with the device's own alpha, alpha_d, sigma_c; per block the norm of the defect <= max(100 x the defect of the twin's direction
    applied with the same step lengths in float64, the norm of the entries' (n + 1) u T); the new point is strictly inside every cone.
 5. test_step_lengths_from_the_stored_direction (ITER): from the ds, dz the chain stored (segment rows: phase_reference.segment_row on phUpdate's stored
    inputs) the exact largest steps over ALL cones, the clamps, and alpha / alpha_d within the composite bar of ainv_with_bar (test_cone_math.py's
    stepInv bar, plus its inputs'), itself <= 1e-6 relative.  Under the split rule and under Iter::common_step = 1 (the two runs agree bitwise but for
    alpha, alpha_d and the flag); test_compile_time_common_step_equals_the_flag_bitwise (device) holds the -DIPM_SPLIT_STEPS=0 build to the flag.
 6. test_bitwise_equalities: ITER_STEP == ITER_FUSED on the iterate; LDS-resident == workspace-resident segment fields (whole arena, four ops); a job
    alone == the same job in the launch of all; the ITER prefix of ITER_STEP == ITER, and ITER leaves the iterate alone.
 7. test_footprint: no sentinel changes; inside the blocks the data, the centre, uhat, the pad lanes, the SCvx structural zeros and border column, and
    (ITER, PREDICT) the iterate keep their bits; the rows of cones a stage does not have hold zeros before and after the step.
 8. test_bad_exits: a stage slack outside its cone -> bad = 1 after phScalings; an Inf in Z -> non-finite direction, bad = 1; the iterate bitwise unchanged
    under ITER_STEP and ITER_FUSED; the other instances of the launch bitwise what they are without these two.
 9. test_cold_start (COLD), 10. test_warm_start (WARM): see their docstrings.

Measured worst ratios, error / the twin's error per field on `benign` (the bar is 100 of these, or the 64 u floor):
    emulator  SC    F_DW 17  F_DDL 38  F_DS 26  F_DZ 18  dnu 7.9  dnub 4.7  dlam 14  ds1 7.6  dz1 16  ds2 10  dz2 11    worst scalar 147 (dsc3_0)
    emulator  SCvx  F_DW 1.3  F_DS 3.6  F_DZ 19  dnu 1.5  dnub 1.8  dlam 5.6  ds1 2.7  dz1 6.1  ds2 1.4  dz2 9.8        worst scalar 95 (dss)
    device    SC    F_DW 15  F_DDL 67  F_DS 34  F_DZ 33  dnu 13  dnub 7.7  dlam 26  ds1 17  dz1 29  ds2 13  dz2 20      worst scalar 78 (dzs)
    device    SCvx  F_DW 2.1  F_DS 2.4  F_DZ 4.7  dnu 2.1  dnub 1.6  dlam 2.5  ds1 0.8  dz1 2.0  ds2 1.5  dz2 9.3       worst scalar 61 (dzc3_0)
On `late`, emulator | device: largest field dnu 30 | 23, every other field <= 6.2 | 2.7; single scalars up to 294 | 227.
(a scalar above 100 of its own twin's error -- dsc3_0, 147 on the emulator -- is inside the 64 u floor.)  Every `report` line prints them again.

Not here: the s3 row as the cone that binds the corrector's step (FORCE says why).  The cold start without any violation (shift 1 - gamma): no case of
this problem class -- at both start points some cone has v0 - |v1| <= 0 whatever the data (never_unviolated shows it on the literal G and E and
asserts it), so bring2cone's start value -gamma decides no output of the product either.  In SCvx mode the late points' rx is small on all columns but
the states' (no trust-region row absorbs them).  sigma_c at the composite
step-length bar from the stored predictor direction (test 2 holds it to the twin rule).  NaN payloads in the rows of inactive cones (test_footprint)."""
import ctypes
import os

import numpy as np
import pytest

import newton_late as nl
import newton_reference as nr
import phase_reference as pr
import test_phase_residuals as tpr
import test_sweeps as tsw
from phase_reference import NV, U
from test_phase_residuals import BACKENDS, MODELS, PAYLOAD, SENTINEL, bits

LD = np.longdouble
GAMMA = 0.99  # ECOS's step-length safety factor (Settings::gamma)
SMALL_K, LARGE_K, NINST = (3, 4), (50, 63, 64), 3
SEG_STATE = tpr.SEG_STATE
GLOB_IN, GLOB_STEP, GLOB_OUT = tpr.GLOB_IN, tpr.GLOB_STEP, tpr.GLOB_OUT
ITER_IN = tpr.ITER_IN + ["gamma", "sigbar"]


class Probe:
    """the step probe of one backend; the layouts come from the emulation builds of the phase probe and the sweep probe (interface constants: the same
    in every build)"""

    def __init__(self, path, backend):
        import __graft_entry__ as g

        self.backend, self.path = backend, path
        self.lib = ctypes.CDLL(path)
        for f in ("block_names", "op_names"):
            getattr(self.lib, "step_probe_" + f).restype = ctypes.c_char_p
        self.blocks = self.lib.step_probe_block_names().decode().split()
        self.ops = self.lib.step_probe_op_names().decode().split()
        assert len(self.blocks) == self.lib.step_probe_off_n() and self.lib.step_probe_desc_n() == 5
        self.phase = tpr.Probe(os.environ.get("SCPP_PHASE_PROBE_EMU_LIBRARY") or g.build_phase_probe_emu(), "emu")
        self.sweep = tsw.Probe(os.environ.get("SCPP_SWEEP_PROBE_EMU_LIBRARY") or g.build_sweep_probe_emu(), "emu")
        self.glob_names, self.iter_names = self.phase.glob_names, self.phase.iter_names
        self.split_steps = self.lib.step_probe_split_steps()
        self._lay = {}

    def layout(self, model):
        if model not in self._lay:
            lay = dict(self.phase.layout(model))
            sw = self.sweep.layout(model)
            for n in ("X_BETA", "X_BCW", "X_VW", "X_HS", "X_HC", "X_WBT", "X_RHO", "X_EINV", "X_S", "FACREC", "SVREC", "HS_N", "PAT"):
                lay[n] = sw[n]
            ex = np.zeros(8, dtype=np.int32)
            assert self.lib.step_probe_extra_layout(model, ex.ctypes.data_as(ctypes.c_void_p)) == 0
            assert (lay["X_HS"], lay["X_HC"], lay["HS_N"], lay["FACREC"], lay["SVREC"]) == tuple(ex[:5])
            lay["GSAVE"], lay["F_ETA"], lay["F_WB"] = int(ex[5]), int(ex[6]), int(ex[7])
            self._lay[model] = lay
        return self._lay[model]

    def masks(self, model, K):
        return self.phase.masks(model, K)

    def sizes(self, model, K):
        need = np.zeros(len(self.blocks), dtype=np.int64)
        assert self.lib.step_probe_block_sizes(model, K, need.ctypes.data_as(ctypes.c_void_p)) == 0
        return need.tolist()

    def run_rc(self, desc, offs, arena):
        assert desc.dtype == np.int32 and offs.dtype == np.int64 and arena.dtype == np.float64
        return self.lib.step_probe_run(len(desc), desc.ctypes.data_as(ctypes.c_void_p), offs.ctypes.data_as(ctypes.c_void_p),
                                       arena.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(arena.size))

    def run(self, desc, offs, arena):
        rc = self.run_rc(desc, offs, arena)
        assert rc == 0, rc


@pytest.fixture(scope="module", params=BACKENDS)
def probe(request):
    """the probe library of the emulation build or of the device build"""
    import __graft_entry__ as g

    if request.param == "emu":
        return Probe(os.environ.get("SCPP_STEP_PROBE_EMU_LIBRARY") or g.build_step_probe_emu(), "emu")
    lib = os.environ.get("SCPP_STEP_PROBE_LIBRARY") or g.STEP_PROBE_LIB
    if not os.path.exists(lib):
        g.build_step_probe()
    return Probe(lib, "hip")


def common_probe(probe):
    """the build of the same backend with the compile-time common step length (device only: the emulation build has the shipped rule)"""
    import __graft_entry__ as g

    lib = os.environ.get("SCPP_STEP_PROBE_COMMON_LIBRARY") or g.STEP_PROBE_COMMON_LIB
    if not os.path.exists(lib):
        g.build_step_probe_common_step()
    p = Probe(lib, "hip")
    assert p.split_steps == 0 and probe.split_steps == 1
    return p


# ---------------------------------------------------------------- the instances (drawn once, shared by both backends): the phase tests' populations
CASES = {}


def get_case(probe, model, K, scvx, pop, inst):
    """phase tests' draw (imported, not copied) with the step probe's layout, the solver's gamma and sigbar in Iter"""
    key = (model, K, scvx, pop, inst)
    if key not in CASES:
        # `late`: an interior late iterate built on an instance of draw's benign population of its own (newton_late.py says how and why not make_late's)
        d = tpr.draw(probe, model, K, scvx, "benign", inst + (100 if pop == "late" else 0))
        if pop == "late":
            d = nl.make_interior_late(d, np.random.default_rng([20261211, model, K, int(scvx), inst]))
        d["iter"] = dict(d["iter"], gamma=GAMMA, sigbar=d["glob"]["sigbar"])
        if pop == "benign" and inst == 2 and (model, K, scvx) in FORCE:
            d = force_binding(d, *FORCE[model, K, scvx])
        CASES[key] = d
    return CASES[key]


def case_keys(scvx, pop):
    return [(m, K, scvx, pop, i) for m in range(4) for K in SMALL_K for i in range(NINST)] + [(0, K, scvx, pop, 0) for K in LARGE_K]


def label_of(d, inst=None):
    return tpr.label_of(d, inst)


# ---------------------------------------------------------------- the arena
class Arena:
    """EVERY block of a job's Ctx as a slice of one array of doubles: sentinels between and around the blocks, quiet-NaN payloads in every double of a
    block that is not an input of the op.  jobs: [(d, policy, op name)]; COLD gets the record state phSetup leaves (test_cold_start asserts it)."""

    def __init__(self, probe, jobs):
        self.probe, self.jobs = probe, jobs
        self.NB = NB = len(probe.blocks)
        self.B = {n: i for i, n in enumerate(probe.blocks)}
        rng = np.random.default_rng(11)
        offs, pos, self.sizes = np.zeros((len(jobs), NB), dtype=np.int64), 16, []
        for q, (d, _, _) in enumerate(jobs):
            size = probe.sizes(d["model"], d["K"])
            for f in range(NB):
                pos = (pos + 15) & ~15 if probe.blocks[f] in ("sx", "fac", "sv") else (pos + 1) & ~1
                offs[q, f] = pos
                pos += size[f] + int(rng.integers(1, 24))
            self.sizes.append(size)
        self.offs = offs
        self.a = np.zeros(pos + 16)
        bits(self.a)[:] = SENTINEL | (np.arange(self.a.size, dtype=np.uint64) & np.uint64(0xFFFF))
        for q, (d, _, op) in enumerate(jobs):
            for f in range(NB):
                bits(self.block(q, f))[:] = PAYLOAD | (np.uint64(f) << np.uint64(32)) | (np.arange(self.sizes[q][f], dtype=np.uint64) + np.uint64(1))
            self.write_inputs(q, d, op)
        self.desc = np.array([[d["model"], policy, d["K"], probe.ops.index(op), d.get("setup_v0", 0)] for d, policy, op in jobs], dtype=np.int32)

    def block(self, q, f, a=None):
        f = self.B[f] if isinstance(f, str) else f
        return (self.a if a is None else a)[self.offs[q, f]:][:self.sizes[q][f]]

    def own(self, q):
        m = np.zeros(self.a.size, dtype=bool)
        for f in range(self.NB):
            self.block(q, f, m)[:] = True
        return m

    def views(self, q, a=None):
        d = self.jobs[q][0]
        pitch = (d["K"] + 1) & ~1
        return (self.block(q, "st", a).reshape(-1, pitch), self.block(q, "sg", a).reshape(-1, pitch), self.block(q, "dy", a).reshape(-1, pitch),
                self.block(q, "sx", a).reshape(d["K"], -1))

    def write_inputs(self, q, d, op):
        lay, K, scvx = d["lay"], d["K"], d["scvx"]
        NL, NS, NX, NU, NXV, NUV = (lay[n] for n in ("NL", "NS", "NX", "NU", "NXV", "NUV"))
        st, sg, dy, sx = self.views(q)
        cold = op == "COLD"
        if cold:  # phSetup clears the three record blocks of a cold solve
            st[:, :K], sx[:], sg[:, :K - 1] = 0., 0., 0.

        rows_on = np.array([pr.active_rows(lay, a) for a in d["act"]])  # [k][row]: the rows of the cones and LP rows stage k has

        def put_pad(f, v):  # a stage vector that starts at the trust-region cone: SCvx keeps the payloads in rows 1 .. NXV.  The rows of a cone or
            for i in range(NS):  # LP row the stage does not have: zeros, as phSetup leaves them, or the instance's `inactive_fill` (test_footprint)
                if not (scvx and 1 <= i <= NXV):
                    st[f + i, :K] = np.where(rows_on[:, i], v[:, i], d.get("inactive_fill", 0.))

        st[lay["F_W"]:lay["F_W"] + NV, :K] = d["W"].T
        st[lay["F_DL"], :K] = d["DL"]
        st[lay["F_WBAR"]:lay["F_WBAR"] + NV, :K] = d["WBAR"].T
        st[lay["F_UHAT"]:lay["F_UHAT"] + 3, :K] = d["UHAT"].T
        if cold:
            st[lay["F_ETA"]:lay["F_ETA"] + lay["NCONES"], :K] = 1.
            for c in range(lay["NCONES"]):
                st[lay["F_WB"] + lay["coneOff"][c], :K] = 1.
        else:
            put_pad(lay["F_S"], d["S"])
            put_pad(lay["F_Z"], d["Z"])
            for f in ("F_DS", "F_DZ"):  # (the cleared record again: the step adds alpha ds to every row, the rows a stage does not have included)
                st[lay[f]:lay[f] + NS, :K] = np.where(rows_on.T, st[lay[f]:lay[f] + NS, :K], 0.)
        for n in ("NU", "NUB") if cold else SEG_STATE:
            sg[lay["G_" + n] * NL:lay["G_" + n] * NL + NL, :K - 1] = d[n].T
        for i in range(NL):
            for j in range(NXV):
                dy[lay["DY_A"] + i * NX + lay["XMAP"][j], :K - 1] = d["A"][:, i, lay["XMAP"][j]]
            for j in range(NUV):
                dy[lay["DY_B"] + i * NU + lay["UMAP"][j], :K - 1] = d["B"][:, i, lay["UMAP"][j]]
                dy[lay["DY_C"] + i * NU + lay["UMAP"][j], :K - 1] = d["C"][:, i, lay["UMAP"][j]]
            if not scvx:
                dy[lay["DY_S"] + i, :K - 1] = d["Sc"][:, i]
            elif cold:  # phSetup copies S = 0; the start-point phases read it, the loop's phases go through the padded view (a payload stays there)
                dy[lay["DY_S"] + i, :K - 1] = 0.
            dy[lay["DY_Z"] + i, :K - 1] = d["Zc"][:, i]
        # phSetup's copy of S_k in the exchange record (the border column's right-hand side); SCvx: S = 0
        sx[:K - 1, lay["X_S"]:lay["X_S"] + NX] = 0. if scvx else d["Sc"]
        self.block(q, "A")[:] = d["A"].ravel()
        self.block(q, "B")[:] = d["B"].ravel()
        self.block(q, "C")[:] = d["C"].ravel()
        self.block(q, "S")[:] = 0. if scvx else d["Sc"].ravel()
        self.block(q, "Z")[:] = d["Zc"].ravel()
        self.block(q, "ip")[:] = d["ip"]
        gl, it = self.block(q, "glob"), self.block(q, "iter")
        if cold:
            gl[:] = 0.  # phSetup: everything 0 but ss = zs = s3 = z3 = seta = sw_0 = 1 (the start values of sig, dsg, n1 are the test's)
            for n in ("ss", "zs", "s3", "z3", "seta", "sw_0"):
                gl[self.probe.glob_names.index(n)] = 1.
            for n in ("sig", "dsg", "n1", "sigbar"):
                gl[self.probe.glob_names.index(n)] = d["glob"][n]
        else:
            for n in GLOB_IN:
                gl[self.probe.glob_names.index(n)] = d["glob"][n]
        for n in ITER_IN:
            it[self.probe.iter_names.index(n)] = d["iter"][n]

    def outputs(self, q, a):
        """what job q left in its blocks, from arena contents a: stage / segment fields as [k][entry] arrays, the exchange record, Glob and Iter as dicts"""
        d = self.jobs[q][0]
        lay, K = d["lay"], d["K"]
        NL, NS = lay["NL"], lay["NS"]
        st, sg, _, sx = self.views(q, a)
        o = {n: st[lay[n]:lay[n] + w, :K].T.copy() for n, w in (("F_W", NV), ("F_DW", NV), ("F_S", NS), ("F_Z", NS), ("F_DS", NS), ("F_DZ", NS), ("F_RZ", NS),
                                                                 ("F_RXW", NV), ("F_HDW", NV))}
        for n in ("F_DL", "F_DDL", "F_HDD", "F_RXD"):
            o[n] = st[lay[n], :K].copy()
        for n in SEG_STATE + ("RY", "DNU", "DNUB", "DLAM", "DS1", "DS2"):
            o["G_" + n] = sg[lay["G_" + n] * NL:lay["G_" + n] * NL + NL, :K - 1].T.copy()
        o["sx"] = sx.copy()
        o["glob"] = dict(zip(self.probe.glob_names, self.block(q, "glob", a)))
        o["iter"] = dict(zip(self.probe.iter_names, self.block(q, "iter", a)))
        return o


class Run:
    def __init__(self, probe, jobs):
        self.arena = Arena(probe, jobs)
        self.before = self.arena.a.copy()
        probe.run(self.arena.desc, self.arena.offs, self.arena.a)
        self.after = self.arena.a


RUNS = {}


def with_rule(d, common):
    return dict(d, iter=dict(d["iter"], common_step=1.)) if common else d


def get_run(probe, scvx, pop, policy, op, common=False, tag=None):
    """all instances of one population and mode in ONE launch"""
    key = (tag or probe.backend, scvx, pop, policy, op, common)
    if key not in RUNS:
        RUNS[key] = Run(probe, [(with_rule(get_case(probe, *k), common), policy, op) for k in case_keys(scvx, pop)])
    return RUNS[key]


# ---------------------------------------------------------------- the references (once per case, shared by both backends and all tests)
KINDS = ("stage cone", "stage LP row", "segment LP row", "wave-uniform row")
# instance 2 of some models at K = 3 has the slack and dual of ONE cone re-drawn until a cone of this kind binds a step length: naturally the segment and
# stage LP rows bind at K = 3, 4 and a stage cone at the large horizons; a step length taken over the wrong set of cones must not go unnoticed
# (model, K, scvx) -> (kind, first row key of the cone or None for any cone of the kind).  Of the three wave-uniform cones ss and sc3 can be made to bind;
# the s3 row cannot on these populations: its dual moves by om (w_vc - z3) whatever the point is, so -dz3 / z3 < 1 and -ds3 / s3 = 1 + dz3 / z3 - ... stays
# O(1) while the other cones of a point this far from the central path reach 20 .. 4000 (scanned over s3, z3 in 1e-8 .. 1e4: never above 1.3)
FORCE = {(0, 3, False): ("stage cone", None), (0, 3, True): ("stage cone", None), (1, 3, False): ("wave-uniform row", ("sc", 0)),
         (1, 3, True): ("wave-uniform row", ("sc", 0)), (3, 3, False): ("wave-uniform row", ("ss",)), (2, 3, True): ("wave-uniform row", ("ss",))}
REFS = {}


class Ref:
    def __init__(self, d, small_mp=True):
        self.N = N = nr.Newton(d, GAMMA, small_mp)
        self.R, self.T = nr.fields_of(N.L, N.ref), nr.fields_of(N.L, N.twin)
        self.kind_p, self.kind_d = N.L.cones[N.bind_p][0], N.L.cones[N.bind_d][0]

    def alphas(self, common):
        a, ad = self.N.alpha_p, self.N.alpha_d
        return (min(a, ad), min(a, ad)) if common else (a, ad)


def slack_slot(d, key, which):
    """(array or dict, index) of one slack (which = 's') or dual ('z') entry of instance d"""
    up = which.upper()
    if key[0] == "st":
        return d[up], (key[1], key[2])
    if key[0] in ("s1", "s2"):
        return d[up + key[0][1]], (key[1], key[2])
    if key[0] == "sc":
        return d["glob"], "%sc3_%d" % (which, key[1])
    return d["glob"], {"ss": "ss", "s3": "s3"}[key[0]] if which == "s" else {"ss": "zs", "s3": "z3"}[key[0]]


FACTORS = [(1., 1e-2), (1e-2, 1.), (1., 1e-4), (1e-4, 1.), (1e2, 1e-2), (1e-2, 1e2), (1e4, 1e-4), (1e-4, 1e4), (1e4, 1e-6), (1e-6, 1e4), (1e6, 1e-6), (1e-6, 1e6)]


def force_binding(d, kind, first=None):
    """a copy of d in which the slack and the dual of ONE cone of `kind` are re-drawn (scaled by the pairs of FACTORS in turn: the point stays interior) until
    a cone of that kind binds alpha_p or alpha_d; decided on the reference alone.  Why scalings: in a Newton step ds / s + dz / z of an LP pair is
    -1 + sigma mu / (s z) whatever the margins are, so a cone binds when one of the two quotients is large and positive -- a small dual against the O(1)
    change dual feasibility asks of it (with a slack large enough that sigma mu / (s z) does not outweigh it), or the other way round."""
    r = Ref(d, small_mp=False)  # (the search for a binding cone runs on the refined longdouble solve; the case's reference is made afterwards)
    binds = lambda r_: [i for i in (r_.N.bind_p, r_.N.bind_d) if r_.N.L.cones[i][0] == kind and first in (None, r_.N.L.cones[i][1][0])]
    if binds(r):
        return d
    for ci, (kd, keys) in enumerate(r.N.L.cones):
        if kd != kind or first not in (None, keys[0]):
            continue
        for fs, fz in FACTORS:
            e = dict(d, glob=dict(d["glob"]), **{n: d[n].copy() for n in ("S", "Z", "S1", "Z1", "S2", "Z2")})
            for which, v, f in (("s", r.N.s[ci], fs), ("z", r.N.z[ci], fz)):
                for key, x in zip(keys, v):
                    box, idx = slack_slot(e, key, which)
                    box[idx] = float(x) * f
            if binds(Ref(e, small_mp=False)):
                return e
    raise AssertionError(f"no cone of kind {kind} can be made to bind in {label_of(d)}")


def reference(probe, key):
    if key not in REFS:
        REFS[key] = Ref(get_case(probe, *key))
    return REFS[key]


def field_masks(d, on):
    """which entries of the stage fields carry a value of the literal problem: free variables, rows that exist"""
    K = d["K"]
    free = np.array([[not (d["fm"][k] >> j) & 1 and j < d["lay"]["NVU"] for j in range(NV)] for k in range(K)])
    return dict(F_DW=free, F_DDL=np.ones(K, dtype=bool), F_DS=on, F_DZ=on)


def field_bar(ref, twin):
    """max(100 x the twin's largest error on the field, 64 u x the field's largest reference entry): the rule test_sweeps.py holds the eliminations to"""
    ref = np.asarray(ref, dtype=LD)
    terr = float(np.abs(np.asarray(twin, dtype=LD) - ref).max(initial=0))
    return max(100. * terr, 64 * U * float(np.abs(ref).max(initial=0))), terr


def report(probe, what, worst):
    for name, w in worst.items():
        print(f"[newton step] {probe.backend} {what} {name}: " + "  ".join(f"{n} {v:.3g}" for n, v in w.items()))


POPS = [False, True]
POP_IDS = ["SC", "SCvx"]
POINTS = ["benign", "late"]
GLOB_DIR = GLOB_STEP
SEG_DIR = (("dnu", "G_NU", "NU", 0), ("dnub", "G_NUB", "NUB", 0), ("dlam", "G_LAM", "LAM", 1), ("ds1", "G_S1", "S1", 0), ("dz1", "G_Z1", "Z1", 1),
           ("ds2", "G_S2", "S2", 0), ("dz2", "G_Z2", "Z2", 1))


# ---------------------------------------------------------------- 1. the populations, on the reference alone
@pytest.mark.parametrize("scvx", POPS, ids=POP_IDS)
def test_populations_on_the_reference(probe, scvx):
    keys = case_keys(scvx, "benign")
    inside_a = inside_s = border = 0
    ld_gap = 0.
    bound, uniform = set(), set()
    for key in keys:
        d, r = get_case(probe, *key), reference(probe, key)
        N = r.N
        for n in ("F_DW", "F_DDL", "F_DS", "F_DZ") + tuple(s[0] for s in SEG_DIR):
            big = float(np.abs(r.R[n]).max(initial=0))
            assert float(np.abs(r.T[n] - r.R[n]).max(initial=0)) <= 1e-6 * big, (label_of(d, key[4]), n)
        for n, v in r.R["glob"].items():
            assert abs(float(r.T["glob"][n] - v)) <= 1e-6 * max(abs(float(x)) for x in r.R["glob"].values()), (label_of(d, key[4]), n)
        # K = 3, 4: the reference is the mpmath solve; the refined longdouble solve, which is the reference of the large horizons, must be ten
        # times nearer to it than the twin (64 against 53 bits promise 2^-11; the worst measured is 1e-2), on the predictor and on the corrector
        assert (N.mp is not None) == (d["K"] <= 4), label_of(d, key[4])
        if N.mp is not None:
            for exact, ld, twin in ((N.aff, N.aff_ld, N.aff64), (N.ref, N.ref_ld, N.twin)):
                Rm, Rl, Tw = nr.fields_of(N.L, exact), nr.fields_of(N.L, ld), nr.fields_of(N.L, twin)
                for n in ("F_DW", "F_DDL", "F_DS", "F_DZ") + tuple(s[0] for s in SEG_DIR):
                    terr = max(float(np.abs(Tw[n] - Rm[n]).max(initial=0)), U * float(np.abs(Rm[n]).max(initial=0)))
                    gap = float(np.abs(Rl[n] - Rm[n]).max(initial=0))
                    assert gap <= 1e-1 * terr, (label_of(d, key[4]), n, gap, terr)  # (a thousandth of the bar of test 3: it changes no verdict)
                    ld_gap = max(ld_gap, gap / terr) if terr else ld_gap
        a, ad = float(N.alpha_p), float(N.alpha_d)
        inside_a += 1e-8 < a < 0.999 and 1e-8 < ad < 0.999 and a != ad
        inside_s += 1e-4 < float(N.sigma_unclamped) < 1.
        bound |= {r.kind_p, r.kind_d}
        uniform |= {N.L.cones[i][1][0][0] for i in (N.bind_p, N.bind_d) if N.L.cones[i][0] == "wave-uniform row"}
        dxn = float(np.sqrt((N.ref.dx * N.ref.dx).sum()))
        border += (not scvx) and abs(float(r.R["glob"]["dsig"])) > 1e-3 * dxn and abs(float(r.R["glob"]["ddsg"])) > 1e-3 * dxn
    assert 3 * inside_a >= len(keys) and 3 * inside_s >= len(keys), (inside_a, inside_s, len(keys))
    assert bound == set(KINDS), bound
    assert uniform >= {"ss", "sc"}, uniform  # (FORCE says why s3 is not among them)
    assert scvx or border >= 1
    print(f"[newton step] {'SCvx' if scvx else 'SC'} refined longdouble solve against the mpmath solve, worst gap / the twin's error: {ld_gap:.3g}")
    # the longdouble cone algebra against cone_reference's mpmath: W of the first stage cone and of the sigma cone
    import cone_reference as cr

    N = reference(probe, keys[0]).N
    for ci in (0, len(N.L.cones) - 1):
        w, eta = cr.nt_scaling([float(x) for x in N.s[ci]], [float(x) for x in N.z[ci]])
        Wm = cr.w_matrix(float(eta), [float(x) for x in w])  # (rounded to float64 on the way in: 1e-15 is what this comparison can show)
        assert max(abs(float(Wm[i][j]) - float(N.W[ci][i, j])) for i in range(len(w)) for j in range(len(w))) <= 1e-14 * float(np.abs(N.W[ci]).max())


# ---------------------------------------------------------------- 3. the direction
def segment_from_step(d, o_step):
    """the segment directions as (new - old) / alpha from the ITER_STEP point, and the 2 u (|x| + |alpha dx|) / alpha that costs"""
    a = (o_step["iter"]["alpha"], o_step["iter"]["alpha_d"])
    got, extra = {}, {}
    for n, f, src, dual in SEG_DIR:
        step = o_step[f] - d[src]
        got[n] = step / a[dual]
        extra[n] = float((2 * U * (np.abs(d[src]) + np.abs(step)) / a[dual]).max())
    return got, extra


@pytest.mark.parametrize("pop", POINTS)
@pytest.mark.parametrize("scvx", POPS, ids=POP_IDS)
def test_direction_against_the_literal_system(probe, scvx, pop):
    run, step = get_run(probe, scvx, pop, 0, "ITER"), get_run(probe, scvx, pop, 0, "ITER_STEP")
    pred = get_run(probe, scvx, pop, 0, "PREDICT")
    worst, vs_twin = {}, {}
    for q, key in enumerate(case_keys(scvx, pop)):
        d, r = get_case(probe, *key), reference(probe, key)
        o, os_ = run.arena.outputs(q, run.after), step.arena.outputs(q, step.after)
        lab = label_of(d, key[4])
        assert o["iter"]["bad"] == 0. and os_["iter"]["bad"] == 0., lab
        # masked reads: lane K - 1 (no segment) and lane 0 (no previous one) read segment 0 through the clamped views.  Every quantity they can pick up
        # there is far from zero, so a term of segment 0 where a zero belongs moves the direction of stage K - 1 or 0 by more than any bar below: the
        # comparison with the literal system IS the masked-read test of this chain, at K = 63 (lane 63 idle), 64 (lane 63 is stage K - 1) and 3, 4
        for n in ("LAM", "NU", "Zc") + (() if scvx else ("Sc",)):
            assert np.abs(d[n][0]).max() > 1e-3 * max(1. if pop == "benign" else 0., np.abs(d[n]).max()), (lab, n)  # (late: the duals' scale is 1e-10)
        assert np.abs(d["A"][0] - np.eye(d["lay"]["NX"])).max() > 1e-2 and np.abs(d["B"][0]).max() > 1e-2, lab
        w, vt = worst.setdefault(MODELS[d["model"]], {}), vs_twin.setdefault(MODELS[d["model"]], {})
        masks = field_masks(d, r.N.L.on)
        got, extra = segment_from_step(d, os_)
        # (neither phDirSeg<0> nor phDirSeg<1> writes G_DNU, G_DNUB, G_DLAM: after PREDICT and after ITER they hold their payloads still, asserted here;
        # the loop keeps these directions in registers until phUpdate, so the recovery above is the only way to them)
        op_ = pred.arena.outputs(q, pred.after)
        assert all(np.isnan(x[f]).all() for x in (o, op_) for f in ("G_DNU", "G_DNUB", "G_DLAM")), lab
        for n in ("F_DW", "F_DDL", "F_DS", "F_DZ"):
            got[n], extra[n] = o[n], 0.
            if n == "F_DW":  # a fixed variable does not move: exactly zero
                fx = np.array([[bool((d["fm"][k] >> j) & 1) for j in range(NV)] for k in range(d["K"])])
                assert (o[n][fx] == 0.).all(), lab
        for n in got:
            m = masks.get(n, np.ones(got[n].shape, dtype=bool))
            bar, terr = field_bar(r.R[n][m], r.T[n][m])
            assert np.isfinite(got[n][m]).all(), (lab, n)
            err = float(np.abs(got[n][m].astype(LD) - r.R[n][m]).max(initial=0))
            if bar + extra[n] == 0.:
                assert err == 0., (lab, n)
                continue
            w[n] = max(w.get(n, 0.), err / (bar + extra[n]))
            vt[n] = max(vt.get(n, 0.), err / max(terr, 1e-300)) if terr > 0 else vt.get(n, 0.)
        for n in GLOB_DIR:
            err = abs(float(LD(o["glob"][n]) - r.R["glob"][n]))
            bar, terr = field_bar([r.R["glob"][n]], [r.T["glob"][n]])  # each scalar its own field, as the issue lists them
            if bar == 0.:
                assert err == 0., (lab, n)
                continue
            w[n] = max(w.get(n, 0.), err / bar)
            if terr > 0:
                vt[n] = max(vt.get(n, 0.), err / terr)
    report(probe, f"ITER {pop} {'SCvx' if scvx else 'SC'} worst error / bar", worst)
    report(probe, f"ITER {pop} {'SCvx' if scvx else 'SC'} worst error / twin's error", vs_twin)
    assert all(v <= 1. for w in worst.values() for v in w.values()), worst


# ---------------------------------------------------------------- 2. the predictor
def hessian_blocks(d, r):
    """G'W^-2 G of every stage from the reference's W, entry by entry with T (the sum of the absolute values of the products) and n (their number): H[k]
    [16][16] over the stage's w, hdd[k] (delta, delta), hdw[k][16] (delta, w); and the sigma block (Hss, Hsd, Hdd) of the scalar rows"""
    L, N = r.N.L, r.N
    K = d["K"]
    H, T, cnt = np.zeros((K, NV + 1, NV + 1), dtype=LD), np.zeros((K, NV + 1, NV + 1)), np.zeros((K, NV + 1, NV + 1), dtype=int)
    S, ST = np.zeros((2, 2), dtype=LD), np.zeros((2, 2))
    for ci, ((kind, keys), (cols, Gl)) in enumerate(zip(L.cones, L.loc)):
        if not len(cols):
            continue
        W2 = N.W2[ci]
        vs = [L.vars[c] for c in cols]
        if keys[0][0] == "st":
            k = keys[0][1]
            pos = [v[2] if v[0] == "w" else NV for v in vs]
            for a, pa in enumerate(pos):
                for b, pb in enumerate(pos):
                    terms = [Gl[i, a] * W2[i, j] * Gl[j, b] for i in range(len(keys)) for j in range(len(keys)) if Gl[i, a] != 0 and Gl[j, b] != 0]
                    H[k, pa, pb] += sum(terms, LD(0))
                    T[k, pa, pb] += float(sum(abs(t) for t in terms))
                    cnt[k, pa, pb] += len(terms)
        elif keys[0][0] in ("ss", "sc"):
            pos = [{"sig": 0, "dsg": 1}[v[0]] for v in vs]
            for a, pa in enumerate(pos):
                for b, pb in enumerate(pos):
                    terms = [Gl[i, a] * W2[i, j] * Gl[j, b] for i in range(len(keys)) for j in range(len(keys))]
                    S[pa, pb] += sum(terms, LD(0))
                    ST[pa, pb] += float(sum(abs(t) for t in terms))
    return H, T, cnt, S, ST


def scaling_amp(r, ci):
    """relative error of a cone's W^-2 that the scaling's own rounding may cause: (D + 8) u (kappa(s) + kappa(z)) (test_cone_math.py: nt_scaling), doubled
    for the square"""
    s, z = r.N.s[ci], r.N.z[ci]
    if len(s) == 1:
        return 4 * U
    kap = lambda x: float((x[0] * x[0] + (x[1:] * x[1:]).sum()) / nr.jdot(x, x))
    return 2 * (len(s) + 8) * U * (kap(s) + kap(z))


@pytest.mark.parametrize("scvx", POPS, ids=POP_IDS)
def test_predictor_blocks_and_centring(probe, scvx):
    run = get_run(probe, scvx, "benign", 0, "PREDICT")
    worst = {}
    for q, key in enumerate(case_keys(scvx, "benign")):
        d, r = get_case(probe, *key), reference(probe, key)
        if d["K"] > 4 and key[1] != 63:  # the blocks are per stage: one large horizon (the odd record pitch) is enough here
            continue
        lay, K, lab = d["lay"], d["K"], label_of(d, key[4])
        o = run.arena.outputs(q, run.after)
        w = worst.setdefault(MODELS[d["model"]], {})
        assert o["iter"]["bad"] == 0., lab
        # sigma_c against the reference's sigma: the clamped cube of 1 - alpha_aff; the twin gives the yardstick, the composite step-length bar the floor
        sig_bar = max(100. * abs(float(r.N.sigma_twin - r.N.sigma)), 64 * U)
        w["sigma_c"] = max(w.get("sigma_c", 0.), abs(float(LD(o["iter"]["sigma_c"]) - r.N.sigma)) / sig_bar)
        if not scvx:  # schur, the pivot of the sigma border: the Schur complement of sigma in the literal system's matrix, at the bar of test 3
            sref, stwin = r.N.schur_sigma()
            w["schur"] = max(w.get("schur", 0.), abs(float(LD(o["glob"]["schur"]) - sref)) / field_bar([sref], [stwin])[0])
        H, T, cnt, S, ST = hessian_blocks(d, r)
        amp = max(scaling_amp(r, ci) for ci, (kind, keys) in enumerate(r.N.L.cones) if keys[0][0] == "st")
        fx = [[bool((d["fm"][k] >> j) & 1) for j in range(NV)] for k in range(K)]
        # the delta_k elimination: F_HDD = H_dd, F_HDW_j = H_dw_j (SC mode; fixed variables: 0)
        if not scvx:
            for k in range(K):
                bar = (cnt[k, NV, NV] + 1) * U * T[k, NV, NV] + amp * T[k, NV, NV]
                w["F_HDD"] = max(w.get("F_HDD", 0.), abs(float(LD(o["F_HDD"][k]) - H[k, NV, NV])) / bar)
                for j in range(lay["NVU"]):
                    if fx[k][j]:
                        assert o["F_HDW"][k, j] == 0., (lab, k, j)
                        continue
                    bar = (cnt[k, NV, j] + 1) * U * T[k, NV, j] + amp * T[k, NV, j]
                    if bar == 0.:
                        assert o["F_HDW"][k, j] == 0., (lab, k, j)
                    else:
                        w["F_HDW"] = max(w.get("F_HDW", 0.), abs(float(LD(o["F_HDW"][k, j]) - H[k, NV, j])) / bar)
        # X_HS through PAT (the one place PAT is used: it maps reference entries to slots): the application cones' and LP rows' part of H_ww, i.e. H_ww
        # without the trust-region cone's contribution, which X_HC carries as {1 / eta^2, 2 / (2 w0^2 - 1)} (SCvx: -2)
        Ha = app_hessian(d, r)
        pat = lay["PAT"]
        for k in range(K):
            slot_v, slot_t, slot_n = np.zeros(lay["HS_N"], dtype=LD), np.zeros(lay["HS_N"]), np.zeros(lay["HS_N"], dtype=int)
            for a in range(NV):
                for b in range(NV):
                    if pat[a, b] >= 0 and not (slot_t[pat[a, b]] and a > b):
                        slot_v[pat[a, b]], slot_t[pat[a, b]], slot_n[pat[a, b]] = Ha[0][k, a, b], Ha[1][k, a, b], Ha[2][k, a, b]
            for i in range(lay["HS_N"]):
                got = o["sx"][k, lay["X_HS"] + i]
                bar = (slot_n[i] + 1) * U * slot_t[i] + amp * slot_t[i]  # (n + 1) u T with n from the reference, plus the scaling's own error
                if bar == 0.:
                    assert got == 0., (lab, k, i, got)
                else:
                    w["X_HS"] = max(w.get("X_HS", 0.), abs(float(LD(got) - slot_v[i])) / bar)
        # X_HC: {1 / eta^2, 2 / (2 w0^2 - 1)} of the trust-region cone's scaling (SCvx: -2, delta_k is a constant), the scaling's own bar; the second
        # is a quotient by a difference: times its condition (2 w0^2 + 1) / (2 w0^2 - 1)
        tr = {keys[0][1]: ci for ci, (kind, keys) in enumerate(r.N.L.cones) if kind == "stage cone" and keys[0][2] == 0}
        for k in range(K):
            ci = tr[k]
            e2 = np.sqrt(nr.jdot(r.N.z[ci], r.N.z[ci]) / nr.jdot(r.N.s[ci], r.N.s[ci]))
            w0 = r.N.W[ci][0, 0] * np.sqrt(e2)
            den, ak = 2 * w0 * w0 - 1, scaling_amp(r, ci) + 8 * U
            w["X_HC_0"] = max(w.get("X_HC_0", 0.), abs(float(LD(o["sx"][k, lay["X_HC"]]) - e2)) / (ak * float(e2)))
            if scvx:
                assert o["sx"][k, lay["X_HC"] + 1] == -2., (lab, k)
            else:
                w["X_HC_1"] = max(w.get("X_HC_1", 0.), abs(float(LD(o["sx"][k, lay["X_HC"] + 1]) - 2 / den)) / (ak * float((2 * w0 * w0 + 1) / den * 2 / den)))
        # the sigma block: Hsd, Hdd as stored, hsig = Hss - Hsd^2 / Hdd
        ampS = scaling_amp(r, len(r.N.L.cones) - 1) + 4 * U
        for n, v, t in (("Hsd", S[0, 1], ST[0, 1]), ("Hdd", S[1, 1], ST[1, 1]), ("hsig", S[0, 0] - S[0, 1] * S[0, 1] / S[1, 1], ST[0, 0] + abs(float(S[0, 1] * S[0, 1] / S[1, 1])))):
            bar = (12 * U + 3 * ampS) * t
            w[n] = max(w.get(n, 0.), abs(float(LD(o["glob"][n]) - v)) / bar)
    report(probe, f"PREDICT benign {'SCvx' if scvx else 'SC'} worst error / bar", worst)
    assert all(v <= 1. for w in worst.values() for v in w.values()), worst


def app_hessian(d, r):
    """(value, T, n) [K][16][16] of G'W^-2 G over w restricted to the application cones and the stage LP rows (everything but cone 0 of a stage)"""
    L, N, K, lay = r.N.L, r.N, d["K"], d["lay"]
    H, T, cnt = np.zeros((K, NV, NV), dtype=LD), np.zeros((K, NV, NV)), np.zeros((K, NV, NV), dtype=int)
    for ci, (kind, keys) in enumerate(L.cones):
        if keys[0][0] != "st" or (kind == "stage cone" and keys[0][2] == 0):
            continue
        # (over ALL stage variables, fixed ones included: buildHs fills the slots whatever is fixed, the mask is applied where the tile is built)
        k, W2 = keys[0][1], N.W2[ci]
        pos = sorted({v[2] for key in keys for v, _ in L.P.rows[key][0]})
        Gl = np.zeros((len(keys), len(pos)), dtype=LD)
        for i, key in enumerate(keys):
            for v, c in L.P.rows[key][0]:
                Gl[i, pos.index(v[2])] += c
        for a, pa in enumerate(pos):
            for b, pb in enumerate(pos):
                terms = [Gl[i, a] * W2[i, j] * Gl[j, b] for i in range(len(keys)) for j in range(len(keys)) if Gl[i, a] != 0 and Gl[j, b] != 0]
                H[k, pa, pb] += sum(terms, LD(0))
                T[k, pa, pb] += float(sum(abs(t) for t in terms))
                cnt[k, pa, pb] += len(terms)
    return H, T, cnt


# ---------------------------------------------------------------- 5. step lengths and centring from the stored direction
def stored_direction(d, r, o):
    """per cone of the reference's list, (ds, dz) as the chain stored them (longdouble) and a bound on what recomputing an unstored one costs: the stage rows
    from F_DS / F_DZ, the wave-uniform rows from Glob, the segment rows through phase_reference.segment_row on the stored inputs of phUpdate (X_VL, X_BCL,
    the predictor's products, dsig, sigma_c, mu, dz3) with step lengths 1"""
    lay, K, scvx = d["lay"], d["K"], d["scvx"]
    NL = lay["NL"]
    bcl = np.zeros((K - 1, NL)) if scvx else o["sx"][:K - 1, lay["X_BCL"]:lay["X_BCL"] + NL]
    args = [d[n] for n in ("NU", "NUB", "S1", "Z1", "S2", "Z2", "LAM")] + [o["G_DS1"], o["G_DS2"], o["sx"][:K - 1, lay["X_VL"]:lay["X_VL"] + NL], bcl]
    args += [o["glob"]["dsig"], o["iter"]["sigma_c"], o["iter"]["mu"], d["glob"]["z3"], o["glob"]["dz3"], 1., 1.]
    new = pr.segment_row(*[np.asarray(a, dtype=LD) for a in args])
    err = pr.segment_row(*[pr.Err(a) for a in args])
    seg = {n: (v - np.asarray(d[n], dtype=LD), e.e.astype(np.float64)) for n, v, e in zip(pr.SEG_OUT, new, err)}
    ds, dz, eds, edz = [], [], [], []
    for kind, keys in r.N.L.cones:
        a, b, ea, eb = [], [], [], []
        for key in keys:
            if key[0] == "st":
                a.append(o["F_DS"][key[1], key[2]]), b.append(o["F_DZ"][key[1], key[2]]), ea.append(0.), eb.append(0.)
            elif key[0] in ("s1", "s2"):
                i = key[0][1]
                a.append(seg["S" + i][0][key[1], key[2]]), b.append(seg["Z" + i][0][key[1], key[2]])
                ea.append(seg["S" + i][1][key[1], key[2]]), eb.append(seg["Z" + i][1][key[1], key[2]])
            else:
                sn, zn = {"ss": ("dss", "dzs"), "s3": ("ds3", "dz3")}[key[0]] if key[0] != "sc" else ("dsc3_%d" % key[1], "dzc3_%d" % key[1])
                a.append(o["glob"][sn]), b.append(o["glob"][zn]), ea.append(0.), eb.append(0.)
        ds.append(np.array(a, dtype=LD)), dz.append(np.array(b, dtype=LD)), eds.append(max(ea)), edz.append(max(eb))
    return ds, dz, eds, edz


def ainv_with_bar(r, ds, dz, eds, edz):
    """(ainv_p, bar), (ainv_d, bar): the exact reciprocal step to the boundary over all cones, and the composite bar test_cone_math.py holds coneDir's
    stepInv to: c(D) u kappa(lambda) (|mu_1| + |mu_2|) with c = 2 (D + 8) for stepInv itself, plus (D + 8) u (kappa(s) + kappa(z)) for the scaling that made
    lambda and (D + 8) u for each of applyWinv / applyW that made the scaled direction (relative errors of stepInv's inputs, which it amplifies by the same
    kappa(lambda) (|mu_1| + |mu_2|)); an LP row is the quotient -ds / s: 3 u of it.  A recomputed (unstored) direction adds its own bound / s.  The bar of a
    maximum is the largest bar among the cones that can attain it (value + bar not below the largest value - bar)."""
    N = r.N
    out = []
    for v, dv, ev, scaled in ((N.s, ds, eds, lambda ci, x: N.Wi[ci] @ x), (N.z, dz, edz, lambda ci, x: N.W[ci] @ x)):
        cand = [(LD(0), 0.)]
        for ci in range(len(v)):
            a = nr.step_inv(v[ci], dv[ci])
            D = len(v[ci])
            if D == 1:
                b = 3 * U * abs(float(dv[ci][0] / v[ci][0])) + ev[ci] / float(v[ci][0])
            else:
                lam, sv = N.lam[ci], scaled(ci, dv[ci])
                aq, bq, cq = nr.jdot(lam, lam), nr.jdot(lam, sv), nr.jdot(sv, sv)
                rt = np.sqrt(max(bq * bq - aq * cq, LD(0)))
                mus = abs(float((bq - rt) / aq)) + abs(float((bq + rt) / aq))
                kap = lambda x: float((x[0] * x[0] + (x[1:] * x[1:]).sum()) / nr.jdot(x, x))
                b = U * kap(lam) * mus * (2 * (D + 8) + (D + 8) * (kap(N.s[ci]) + kap(N.z[ci])) + 2 * (D + 8))
            cand.append((a, b))
        floor = max(float(a) - b for a, b in cand)
        out.append((max(a for a, _ in cand), max(b for a, b in cand if float(a) + b >= floor)))
    return out


def alpha_bar(gamma, ainv, bar):
    """alpha = clamp(min(gamma / ainv, 1), 1e-8, 0.999): |d alpha| <= gamma bar / ainv^2 + 2 u alpha (a clamp does not expand)"""
    return gamma * bar / float(ainv) ** 2 + 2 * U if ainv > 0 else 2 * U


def check_step_lengths(probe, run, scvx, common, worst, tag, pop="benign"):
    for q, key in enumerate(case_keys(scvx, pop)):
        d, r = get_case(probe, *key), reference(probe, key)
        o = run.arena.outputs(q, run.after)
        ds, dz, eds, edz = stored_direction(d, r, o)
        (ap_inv, bp), (ad_inv, bd) = ainv_with_bar(r, ds, dz, eds, edz)
        ap, ad = nr.clamp_step(GAMMA, ap_inv), nr.clamp_step(GAMMA, ad_inv)
        bap, bad_ = alpha_bar(GAMMA, ap_inv, bp), alpha_bar(GAMMA, ad_inv, bd)
        if common:
            ap = ad = min(ap, ad)
            bap = bad_ = max(bap, bad_)
        w = worst.setdefault(MODELS[d["model"]], {})
        assert bap <= 1e-6 * float(ap) and bad_ <= 1e-6 * float(ad), (label_of(d, key[4]), bap, bad_)
        w["alpha " + tag] = max(w.get("alpha " + tag, 0.), abs(float(LD(o["iter"]["alpha"]) - ap)) / bap)
        w["alpha_d " + tag] = max(w.get("alpha_d " + tag, 0.), abs(float(LD(o["iter"]["alpha_d"]) - ad)) / bad_)
        if common:
            assert o["iter"]["alpha"] == o["iter"]["alpha_d"], label_of(d, key[4])


@pytest.mark.parametrize("pop", POINTS)
@pytest.mark.parametrize("scvx", POPS, ids=POP_IDS)
def test_step_lengths_from_the_stored_direction(probe, scvx, pop):
    worst = {}
    split, common = get_run(probe, scvx, pop, 0, "ITER"), get_run(probe, scvx, pop, 0, "ITER", common=True)
    check_step_lengths(probe, split, scvx, False, worst, "split", pop)
    check_step_lengths(probe, common, scvx, True, worst, "common_step", pop)
    # the direction does not depend on the rule: everything but alpha, alpha_d and the flag itself is bitwise the same
    ar = split.arena
    diff = bits(split.after) != bits(common.after)
    for q in range(len(ar.jobs)):
        it = ar.block(q, "iter", diff)
        for n in ("alpha", "alpha_d", "common_step"):
            it[probe.iter_names.index(n)] = False
    assert not diff.any(), np.flatnonzero(diff)[:8]
    assert any(bits(np.array(split.arena.outputs(q, split.after)["iter"]["alpha"])) != bits(np.array(common.arena.outputs(q, common.after)["iter"]["alpha"]))
               or bits(np.array(split.arena.outputs(q, split.after)["iter"]["alpha_d"])) != bits(np.array(common.arena.outputs(q, common.after)["iter"]["alpha_d"]))
               for q in range(len(ar.jobs)))
    report(probe, f"step lengths {pop} {'SCvx' if scvx else 'SC'} worst error / bar", worst)
    assert all(v <= 1. for w in worst.values() for v in w.values()), worst


@pytest.mark.gpu
@pytest.mark.parametrize("scvx", POPS, ids=POP_IDS)
def test_compile_time_common_step_equals_the_flag_bitwise(scvx):
    """device only: the build with -DIPM_SPLIT_STEPS=0 against the shipped build with Iter::common_step = 1 (ITER and ITER_STEP): every double of the arena
    but the flag itself and the two scalars phDirStage hands to phDirSeg, Iter::part_ainv and part_ainv_d.  Those cannot agree: the shipped build keeps the
    stage part of the primal and the dual bound apart until phDirSeg folds them under the flag, the compile-time rule folds them in phDirStage already and
    never writes part_ainv_d.  What must hold instead does: its part_ainv is the larger of the shipped build's two, bit for bit.  (The same three names,
    and nothing else, differ between the two emulation builds.)"""
    import __graft_entry__ as g

    lib = os.environ.get("SCPP_STEP_PROBE_LIBRARY") or g.STEP_PROBE_LIB
    if not os.path.exists(lib):
        g.build_step_probe()
    shipped = Probe(lib, "hip")
    built = common_probe(shipped)
    names = shipped.iter_names
    for op in ("ITER", "ITER_STEP"):
        a = get_run(shipped, scvx, "benign", 0, op, common=True)
        b = get_run(built, scvx, "benign", 0, op, common=False, tag="hip-common-build")
        diff = bits(a.after) != bits(b.after)
        for q in range(len(a.arena.jobs)):
            for n in ("common_step", "part_ainv", "part_ainv_d"):
                a.arena.block(q, "iter", diff)[names.index(n)] = False
            ia, ib = a.arena.block(q, "iter", a.after), b.arena.block(q, "iter", b.after)
            folded = max(ia[names.index("part_ainv")], ia[names.index("part_ainv_d")])
            assert bits(np.array(folded)) == bits(np.array(ib[names.index("part_ainv")])), (op, q)
        assert not diff.any(), (op, np.flatnonzero(diff)[:8])
        worst = {}
        if op == "ITER":
            check_step_lengths(built, b, scvx, True, worst, "compile-time common")
            assert all(v <= 1. for w in worst.values() for v in w.values()), worst


# ---------------------------------------------------------------- 6. bitwise equalities
def iterate_mask(ar, q):
    """the doubles of job q that hold the iterate: what phUpdate / the fused residual pass change"""
    d = ar.jobs[q][0]
    lay, K, NL, NS = d["lay"], d["K"], d["lay"]["NL"], d["lay"]["NS"]
    m = np.zeros(ar.a.size, dtype=bool)
    st, sg, _, _ = ar.views(q, m)
    st[lay["F_W"]:lay["F_W"] + NV, :K] = True
    st[lay["F_DL"], :K] = True
    st[lay["F_S"]:lay["F_S"] + NS, :K] = True
    st[lay["F_Z"]:lay["F_Z"] + NS, :K] = True
    for n in SEG_STATE:
        sg[lay["G_" + n] * NL:lay["G_" + n] * NL + NL, :K - 1] = True
    gl = ar.block(q, "glob", m)
    for n in GLOB_OUT:
        gl[ar.probe.glob_names.index(n)] = True
    return m


def all_iterates(ar):
    m = np.zeros(ar.a.size, dtype=bool)
    for q in range(len(ar.jobs)):
        m |= iterate_mask(ar, q)
    return m


@pytest.mark.parametrize("scvx", POPS, ids=POP_IDS)
def test_bitwise_equalities(probe, scvx):
    it_, st_, fu_ = (get_run(probe, scvx, "benign", 0, op) for op in ("ITER", "ITER_STEP", "ITER_FUSED"))
    it_m = all_iterates(it_.arena)
    # the two ways of applying the step store the same iterate
    diff = np.flatnonzero((bits(st_.after) != bits(fu_.after)) & it_m)
    assert diff.size == 0, diff[:8]
    assert ((bits(st_.after) != bits(st_.before)) & it_m).sum() > 1000
    # the ITER prefix of ITER_STEP: everything but the iterate is what ITER left, and ITER leaves the iterate alone
    diff = np.flatnonzero((bits(st_.after) != bits(it_.after)) & ~it_m)
    assert diff.size == 0, diff[:8]
    assert not ((bits(it_.after) != bits(it_.before)) & it_m).any()
    # LDS-resident against workspace-resident segment fields
    for op in ("ITER", "ITER_STEP", "ITER_FUSED", "PREDICT"):
        a, b = get_run(probe, scvx, "benign", 0, op), get_run(probe, scvx, "benign", 1, op)
        diff = np.flatnonzero(bits(a.after) != bits(b.after))
        assert diff.size == 0, (op, diff[:8])
    # a job alone against the same job in the launch of all
    for op in ("ITER_STEP", "PREDICT"):
        run = get_run(probe, scvx, "benign", 0, op)
        picks = (1, 2 * NINST + 1, 5 * NINST + 2, len(run.arena.jobs) - 1, len(run.arena.jobs) - 2)
        for q in picks:
            alone = Run(probe, [run.arena.jobs[q]])
            for f in range(run.arena.NB):
                assert (bits(alone.arena.block(0, f)) == bits(run.arena.block(q, f))).all(), (op, q, probe.blocks[f])


# ---------------------------------------------------------------- 7. footprint
@pytest.mark.parametrize("scvx", POPS, ids=POP_IDS)
def test_footprint(probe, scvx):
    """Outside the jobs' blocks no sentinel changes.  Inside, the chain writes the fields its phases' header comments name and nothing else: NOT the data
    (ip, A .. Z, the field-major dynamics, gsave), the trust-region centre and uhat, the pad lanes (>= K of the stage fields, >= K - 1 of the segment
    fields), in SCvx mode the structural-zero rows 1 .. NXV of the padded vectors (they hold their payloads still: a load through the padded view returned
    0, a store was dropped) nor the S column and the border column; and ITER / PREDICT do not touch the iterate.  Everything an op does not read holds a
    distinct quiet NaN: had the chain read one, a direction would be NaN, which test_direction_against_the_literal_system excludes."""
    for op in ("ITER", "ITER_STEP", "PREDICT"):
        for policy in (0, 1):
            run = get_run(probe, scvx, "benign", policy, op)
            ar = run.arena
            changed = bits(run.after) != bits(run.before)
            keep = np.ones(ar.a.size, dtype=bool)  # what must not change
            for q, (d, _, _) in enumerate(ar.jobs):
                lay, K, NL, NS, NXV = d["lay"], d["K"], d["lay"]["NL"], d["lay"]["NS"], d["lay"]["NXV"]
                own = ar.own(q)
                keep &= ~own
                m = np.zeros(ar.a.size, dtype=bool)
                for f in ("ip", "A", "B", "C", "S", "Z", "dy", "gsave"):
                    ar.block(q, f, m)[:] = True
                st, sg, _, sx = ar.views(q, m)
                st[:, K:] = True
                sg[:, K - 1:] = True
                st[lay["F_WBAR"]:lay["F_WBAR"] + NV, :] = True
                st[lay["F_UHAT"]:lay["F_UHAT"] + 3, :] = True
                sx[:, lay["X_S"]:lay["X_S"] + 16] = True
                if scvx:
                    for f in ("F_S", "F_Z", "F_DS", "F_DZ", "F_RZ", "F_TZ", "F_LS", "F_DSS", "F_WB"):
                        st[lay[f] + 1:lay[f] + 1 + NXV, :] = True
                    st[lay["F_HDW"]:lay["F_HDW"] + NV, :] = True
                    sx[:, lay["X_BCW"]:lay["X_BCW"] + NV] = True
                    sx[:, lay["X_BCL"]:lay["X_BCL"] + 16] = True
                if op != "ITER_STEP":
                    m |= iterate_mask(ar, q)
                keep |= m
            bad = np.flatnonzero(changed & keep)
            assert bad.size == 0, (op, policy, bad[:8])
    # The slack and dual rows of a cone or LP row a stage does not have.  The phases load them with the rest of the stage vector and mask them through
    # their CONTENT: phSetup cleared them, and a zero there contributes nothing.  Measured on the emulator: with a NaN in them the chain ends with
    # bad = 1, with another finite number (-3.5) the direction of that stage changes -- so neither a NaN payload (as in the SCvx rows) nor "no output
    # depends on them" can be asserted of these rows.  What the chain owes the next iteration is asserted instead: the zeros are there on the way in
    # (draw's) and still there, in s, z, ds and dz, after the step, whichever way it is applied
    for op in ("ITER_STEP", "ITER_FUSED"):
        run, inactive = get_run(probe, scvx, "benign", 0, op), 0
        for q, (d, _, _) in enumerate(run.arena.jobs):
            lay, K, NS = d["lay"], d["K"], d["lay"]["NS"]
            off = ~np.array([pr.active_rows(lay, a) for a in d["act"]]).T
            for f in ("F_S", "F_Z", "F_DS", "F_DZ"):
                if f in ("F_S", "F_Z"):
                    assert (run.arena.views(q, run.before)[0][lay[f]:lay[f] + NS, :K][off] == 0.).all(), (op, q, f)
                assert (run.arena.views(q, run.after)[0][lay[f]:lay[f] + NS, :K][off] == 0.).all(), (op, q, f)
            inactive += off.sum()
        assert inactive > 0


@pytest.mark.parametrize("scvx", POPS, ids=POP_IDS)
def test_inactive_rows_are_masked_by_their_content(probe, scvx):
    """The contract test_footprint describes, pinned: with a NaN in the slack and dual rows of the cones and LP rows a stage does not have, the chain
    ends with Iter::bad = 1 and the iterate outside those rows keeps every bit, under both ways of applying the step.  A restructuring of these loads
    that stops reading the rows (or starts masking them by the activity bits) turns this red and has to say so."""
    keys = [(m, K, scvx, "benign", 1) for m in range(4) for K in SMALL_K]
    for op in ("ITER_STEP", "ITER_FUSED"):
        run = Run(probe, [(dict(get_case(probe, *k), inactive_fill=np.nan), 0, op) for k in keys])
        changed = bits(run.after) != bits(run.before)
        for q, (d, _, _) in enumerate(run.arena.jobs):
            lay, K, NS = d["lay"], d["K"], d["lay"]["NS"]
            off = ~np.array([pr.active_rows(lay, a) for a in d["act"]]).T
            assert off.any(), q
            for f in ("F_S", "F_Z"):
                assert np.isnan(run.arena.views(q, run.before)[0][lay[f]:lay[f] + NS, :K][off]).all()
            assert run.arena.outputs(q, run.after)["iter"]["bad"] == 1., (op, q)
            assert not (changed & iterate_mask(run.arena, q)).any(), (op, q)


# ---------------------------------------------------------------- 8. the bad exits
@pytest.mark.parametrize("scvx", POPS, ids=POP_IDS)
def test_bad_exits(probe, scvx):
    """finite or NaN data only.  One instance has ONE stage slack outside its cone: Iter::bad = 1 after phScalings and no field of the iterate changes.  One
    has an Inf in its Z dynamics constant: the direction is non-finite, bad = 1, and ITER_STEP leaves the iterate bitwise unchanged, as the product's loop
    would (it breaks before the next pass applies the step).  The other instances of the launch are bitwise what they are in a launch without these two."""
    keys = [(m, K, scvx, "benign", 0) for m in range(4) for K in (3, 4)]
    base = [get_case(probe, *k) for k in keys]
    out = dict(base[2], S=base[2]["S"].copy())
    lay = out["lay"]
    c = 1 if lay["NCONES"] > 1 else 0
    o_, dim = lay["coneOff"][c], lay["coneDim"][c]
    k_ = next(k for k in range(out["K"]) if out["act"][k] & (1 << c))
    out["S"][k_, o_] = 0.5 * np.sqrt((out["S"][k_, o_ + 1:o_ + dim] ** 2).sum())
    assert 0. < out["S"][k_, o_] < np.sqrt((out["S"][k_, o_ + 1:o_ + dim] ** 2).sum())
    inf = dict(base[5], Zc=base[5]["Zc"].copy())
    inf["Zc"][1, 0] = np.inf
    for op in ("ITER_STEP", "ITER_FUSED"):
        jobs = [(d, 0, op) for d in base]
        jobs.insert(3, (out, 0, op))
        jobs.insert(7, (inf, 0, op))
        run, clean = Run(probe, jobs), Run(probe, [(d, 0, op) for d in base])
        for q in (3, 7):
            o = run.arena.outputs(q, run.after)
            assert o["iter"]["bad"] == 1., (op, q)
            m = iterate_mask(run.arena, q)
            assert not ((bits(run.after) != bits(run.before)) & m).any(), (op, q)
        assert not np.isfinite(run.arena.outputs(7, run.after)["F_DW"]).all()
        others = [q for q in range(len(jobs)) if q not in (3, 7)]
        for qc, q in enumerate(others):
            assert clean.arena.outputs(qc, clean.after)["iter"]["bad"] == 0.
            for f in range(run.arena.NB):
                assert (bits(clean.arena.block(qc, f)) == bits(run.arena.block(q, f))).all(), (op, q, probe.blocks[f])


# ---------------------------------------------------------------- 4. the iteration in residual form
def moved(d, F_W, F_DL, F_S, F_Z, seg, glob):
    e = dict(d, W=F_W, DL=F_DL, S=F_S.copy(), Z=F_Z.copy(), glob=dict(d["glob"], **glob), **seg)
    if d["scvx"]:  # rows 1 .. NXV hold payloads there (the kernel reads zeros)
        e["S"][:, 1:1 + d["lay"]["NXV"]] = e["Z"][:, 1:1 + d["lay"]["NXV"]] = 0.
    return e


def defect_blocks(d, r, e, a, ad, om):
    """per block the norm of r(new point) - (1 - alpha om) r(old point) and the norm of the entries' (n + 1) u T: the Newton equations promise
    ry+ = (1 - alpha_p om) ry, rz+ = (1 - alpha_p om) rz, rx+ = (1 - alpha_d om) rx; in SCvx mode the regularised row E dx - reg dy = -om ry adds
    alpha_p reg dy to the first, with dy = (lam+ - lam) / alpha_d as stored"""
    L = r.N.L
    P0, P1 = L.P, pr.Problem(e, pr.Num("ld"))
    a, ad, om = LD(a), LD(ad), LD(om)
    out = {}

    def add(block, dv, bar):
        n, b = out.get(block, (LD(0), 0.))
        out[block] = (n + dv * dv, b + bar * bar)

    rz0, rz1 = P0.rz(), P1.rz()
    for kind, keys in L.cones:
        for key in keys:
            block = {"st": "rz stage", "s1": "rz segment", "s2": "rz segment"}.get(key[0], "rz scalar")
            add(block, rz1[key][0] - (1 - a * om) * rz0[key][0], pr.bar(rz1[key][2], rz1[key][1]))
    ry0, ry1 = P0.ry(), P1.ry()
    for key in L.ekeys:
        reg = a * L.reg * (LD(e["LAM"][key]) - LD(d["LAM"][key])) / ad
        add("ry", ry1[key][0] - (1 - a * om) * ry0[key][0] - reg, pr.bar(ry1[key][2] + 1, ry1[key][1] + abs(float(reg))))
    rx0, rx1 = P0.rx(), P1.rx()
    for v in L.vars:
        block = "rx " + {"w": "w", "dl": "delta", "nu": "nu", "nub": "nu_b"}.get(v[0], "scalars")
        add(block, rx1[v][0] - (1 - ad * om) * rx0[v][0], pr.bar(rx1[v][2], rx1[v][1]))
    return {b: (float(np.sqrt(n)), float(np.sqrt(t))) for b, (n, t) in out.items()}


@pytest.mark.parametrize("op", ["ITER_STEP", "ITER_FUSED"])
@pytest.mark.parametrize("pop", POINTS)
@pytest.mark.parametrize("scvx", POPS, ids=POP_IDS)
def test_iteration_in_residual_form(probe, scvx, pop, op):
    run = get_run(probe, scvx, pop, 0, op)
    worst = {}
    for q, key in enumerate(case_keys(scvx, pop)):
        d, r = get_case(probe, *key), reference(probe, key)
        o = run.arena.outputs(q, run.after)
        lab = label_of(d, key[4])
        a, ad, om = o["iter"]["alpha"], o["iter"]["alpha_d"], 1. - o["iter"]["sigma_c"]
        e = moved(d, o["F_W"], o["F_DL"], o["F_S"], o["F_Z"], {n: o["G_" + n] for n in SEG_STATE}, {n: o["glob"][n] for n in GLOB_OUT})
        dev = defect_blocks(d, r, e, a, ad, om)
        # the twin's direction applied with the same step lengths in float64
        T, fm = r.T, field_masks(d, r.N.L.on)
        tw = moved(d, d["W"] + np.where(fm["F_DW"], a * T["F_DW"], 0.), d["DL"] + a * T["F_DDL"], d["S"] + np.where(fm["F_DS"], a * T["F_DS"], 0.),
                   d["Z"] + np.where(fm["F_DZ"], ad * T["F_DZ"], 0.), {src: d[src] + (ad if dual else a) * T[n] for n, _, src, dual in SEG_DIR},
                   {x: d["glob"][x] + (ad if x[0] == "z" else a) * float(T["glob"]["d" + x]) for x in GLOB_OUT})
        twin = defect_blocks(d, r, tw, a, ad, om)
        w = worst.setdefault(MODELS[d["model"]], {})
        for b, (norm, barnorm) in dev.items():
            w[b] = max(w.get(b, 0.), norm / max(100. * twin[b][0], barnorm))
        # the new point stays strictly inside every cone
        P1 = pr.Problem(e, pr.Num("ld"))
        for kind, keys in r.N.L.cones:
            for src in (P1.s, P1.z):
                v = np.array([src[k_] for k_ in keys], dtype=LD)
                assert nr.violation(v) < 0, (lab, kind, keys[0])
    report(probe, f"{op} {pop} {'SCvx' if scvx else 'SC'} worst defect / bar", worst)
    assert all(v <= 1. for w in worst.values() for v in w.values()), worst


# ---------------------------------------------------------------- 9. / 10. the start points
def cone_values(d, L, o, which):
    """per cone of the reference's list the slack ('s') or dual ('z') entries job output o holds"""
    e = dict(d, S=o["F_S"], Z=o["F_Z"], S1=o["G_S1"], Z1=o["G_Z1"], S2=o["G_S2"], Z2=o["G_Z2"], glob=o["glob"])
    out = []
    for _, keys in L.cones:
        vals = []
        for key in keys:
            box, idx = slack_slot(e, key, which)
            vals.append(box[idx])
        out.append(np.array(vals, dtype=np.float64))
    return out


def primal_values(d, L, o):
    e = dict(w=o["F_W"], dl=o["F_DL"], nu=o["G_NU"], nub=o["G_NUB"])
    return np.array([e[v[0]][v[1:]] if v[0] in e else o["glob"][v[0]] for v in L.vars])


COLD_KEYS = [(m, K, scvx, "benign", i) for scvx in (False, True) for m in range(4) for K in SMALL_K for i in range(2)] + [(0, 63, False, "benign", 0)]
COLD = {}


def cold_case(probe, key):
    """the benign instance with nu = nu_b = 0: phInitPrimalRhs writes zeros for their right-hand sides, i.e. presupposes the cleared segment record"""
    d = get_case(probe, *key)
    d = dict(d, NU=np.zeros_like(d["NU"]), NUB=np.zeros_like(d["NUB"]))
    if key[:2] == (1, 3) and key[4] == 1:  # sigbar far from everything else: the row sig - sigbar of sc3 holds the largest violation of the slacks
        d = dict(d, glob=dict(d["glob"], sigbar=1e3), iter=dict(d["iter"], sigbar=1e3))
    return d


def cold_reference(probe, key):
    if key not in COLD:
        d = cold_case(probe, key)
        COLD[key] = (nr.ColdStart(d, GAMMA), nr.ColdStart(d, GAMMA, dt=np.float64))
    return COLD[key]


def never_unviolated(L, ref, lab):
    """Why `nothing is violated, so the shift is 1 - gamma` is no case of this problem class -- bring2cone counts a cone with v0 - |v1| <= 0, and at
    both start points some cone has exactly that, whatever the data; shown on the literal G, E and on the reference's solutions.
    Dual, z = G u of the least-norm problem: either an active stage cone's first row of G is empty (the bound of a norm cone is a constant: TILT,
    WMAX, TMAX), so z0 = 0 <= |z1|, or two LP rows of a stage are each other's negatives in G (the two sides of a box), so z_i = -z_j and one of
    them is <= 0.  Primal, s = h - G x of the least-squares problem: n1 stands in the row s3 alone and in no equality row, so optimality makes that
    row's residual zero, s3 = 0; in SC mode the same holds of delta_k and row 0 of every trust-region cone.  The cost of the phases has entries on
    delta_k, sigma, delta_sigma and n1 only (phInitDualRhs writes zeros for the w rows), so no choice of cost moves the least-norm dual off this."""
    rowsG = []
    for (kind, keys), (cols, Gl) in zip(L.cones, L.loc):
        for i, key in enumerate(keys):
            rowsG.append((kind, key, i, {int(c): Gl[i, j] for j, c in enumerate(cols) if Gl[i, j] != 0}))
    empty_first = [key for kind, key, i, g_ in rowsG if kind == "stage cone" and i == 0 and not g_]
    lp = [(key, g_) for kind, key, i, g_ in rowsG if kind == "stage LP row"]
    boxes = [(a, b) for ia, (a, ga) in enumerate(lp) for b, gb in lp[ia + 1:] if a[1] == b[1] and ga and ga == {c: -v for c, v in gb.items()}]
    assert empty_first or boxes, lab
    assert min(-nr.violation(v) for v in ref.z_pre) <= 0, lab  # exactly: a product with an empty row, a pair of negatives
    n1 = L.vi["n1",]
    hit = [key for kind, key, i, g_ in rowsG if n1 in g_]
    assert hit == [("s3",)] and not L.E[:, n1].any(), lab
    i3 = next(i for i, (_, keys) in enumerate(L.cones) if keys[0] == ("s3",))
    assert abs(float(ref.s_pre[i3][0])) <= 1e-15 * max(1., float(max(np.abs(v).max() for v in ref.s_pre))), lab


def test_cold_start(probe):
    """COLD on records as phSetup leaves them -- the three record blocks cleared, the fixed values, the trust-region centre and uhat in place, identity
    scalings (F_ETA = 1, F_WB = e), S in the exchange record, Glob at its defaults; asserted on the inputs below -- with the start values of the free
    variables drawn at random (draw's W, DL, NU, NUB, sig, dsg, n1; a second launch re-draws them).  x after phInitPrimalFinish and y against the
    least-squares / least-norm problems; bar per field: max(100 x the twin's largest error, 64 u x the largest entry).  bring2cone's alpha is read off
    the outputs (a wave-uniform row whose unshifted value is still stored), which gives s and z BEFORE the shift: those against the reference at the same
    rule, alpha itself against the exact shift of those entries at 4 u of the largest term plus the 5 u the recovery costs (the comments say which), and
    against the reference's alpha at its inputs' bar.  Which cone holds the largest violation is recorded: over the population a stage row, a segment
    row and the sigma cone sc3 (one instance has sigbar = 1e3 for that) each do.  No instance is without a violation, so the shift 1 - gamma does not
    occur; bring2cone's other constant, the + 1, does in every shift.  The start point lies strictly inside every cone."""
    jobs = [(cold_case(probe, k), 0, "COLD") for k in COLD_KEYS]
    rng = np.random.default_rng(5)
    again = []
    for d, _, _ in jobs:
        free = field_masks(d, None)["F_DW"]
        again.append((dict(d, W=np.where(free, rng.standard_normal(d["W"].shape), d["W"]), DL=rng.uniform(0.5, 2., d["K"]),
                           glob=dict(d["glob"], sig=rng.uniform(1., 3.), dsg=rng.standard_normal(), n1=rng.uniform(1., 5.))), 0, "COLD"))
    run, run2 = Run(probe, jobs), Run(probe, again)
    # the presuppositions, on the inputs: cleared records, identity scalings, Glob's defaults
    for q, (d, _, _) in enumerate(jobs):
        lay, K = d["lay"], d["K"]
        st, sg, _, sx = run.arena.views(q, run.before)
        zero = np.ones(st.shape, dtype=bool)
        for f, wd in (("F_W", NV), ("F_DL", 1), ("F_WBAR", NV), ("F_UHAT", 3), ("F_ETA", lay["NCONES"]), ("F_WB", lay["LP0"])):
            zero[lay[f]:lay[f] + wd] = False
        zero[:, K:] = False
        assert (st[zero] == 0.).all() and (st[lay["F_ETA"]:lay["F_ETA"] + lay["NCONES"], :K] == 1.).all()
        wb = st[lay["F_WB"]:lay["F_WB"] + lay["LP0"], :K]
        assert (wb[lay["coneOff"][:lay["NCONES"]]] == 1.).all() and wb.sum() == lay["NCONES"] * K
        segz = np.ones(sg.shape, dtype=bool)
        segz[:, K - 1:] = False
        assert (sg[segz] == 0.).all() and (np.delete(sx, np.s_[lay["X_S"]:lay["X_S"] + lay["NX"]], axis=1) == 0.).all()
        gl = dict(zip(probe.glob_names, run.arena.block(q, "glob", run.before)))
        assert all(gl[n] == (1. if n in ("ss", "zs", "s3", "z3", "seta", "sw_0") else 0.) for n in gl if n not in ("sig", "dsg", "n1", "sigbar"))
    worst, seen, where = {}, set(), set()
    for q, key in enumerate(COLD_KEYS):
        d = jobs[q][0]
        ref, twin = cold_reference(probe, key)
        L, lab = ref.L, label_of(d, key[4])
        w = worst.setdefault(MODELS[d["model"]], {})
        outs = [run.arena.outputs(q, run.after), run2.arena.outputs(q, run2.after)]
        xr, xt = np.array([ref.x[v] for v in L.vars]), np.array([twin.x[v] for v in L.vars])
        yr, yt = np.array([ref.y[k] for k in L.ekeys]), np.array([twin.y[k] for k in L.ekeys])
        bx, by = field_bar(xr, xt)[0], field_bar(yr, yt)[0]
        Dmax = max(len(keys) for _, keys in L.cones)
        for which, pre_r, pre_t, sh, alpha in (("s", ref.s_pre, twin.s_pre, ref.s, ref.alpha_s), ("z", ref.z_pre, twin.z_pre, ref.z, ref.alpha_z)):
            bpre = field_bar(np.concatenate(pre_r), np.concatenate(pre_t))[0]
            big = max(float(np.abs(np.concatenate(sh)).max()), abs(float(alpha)))
            for tag, o in zip(("", " (other start values)"), outs):
                got = cone_values(d, L, o, which)
                assert all(nr.violation(np.asarray(v, dtype=LD)) < 0 for v in got), (lab, which)  # strictly inside every cone
                # bring2cone's alpha, from what the phases stored: a wave-uniform row whose value before the shift is still there.  Primal: ss =
                # sig - 0.001 of the stored sig (the affine map of the scalar row, by the reference); dual: zs = -dsig, and dsig stays in Glob.  Each is
                # one rounding of the kernel's and one here: 2 u of the largest term
                x_dev = dict(d, W=o["F_W"], DL=o["F_DL"], NU=o["G_NU"], NUB=o["G_NUB"], glob=dict(d["glob"], **{n: o["glob"][n] for n in ("sig", "dsg", "n1")}))
                a_dev = LD(o["glob"]["ss"]) - pr.Problem(x_dev, pr.Num("ld")).saff()["ss",] if which == "s" else LD(o["glob"]["zs"]) + LD(o["glob"]["dsig"])
                # (a) before the shift: the stored entries less alpha in the first entry of every cone and in every LP row, against the least-squares
                # / least-norm solution, at the bar of test 3 plus 3 u of the largest term (the kernel's addition, alpha's 2 u)
                pre = [np.concatenate([[LD(v[0]) - a_dev], v[1:].astype(LD)]) for v in got]
                err = max(float(np.abs(g - r_).max()) for g, r_ in zip(pre, pre_r))
                w[which + " before the shift" + tag] = max(w.get(which + " before the shift" + tag, 0.), err / (bpre + 3 * U * big))
                # (b) alpha alone: exact arithmetic on a maximum -- from the entries before the shift as the kernel had them (known to 3 u, above)
                # the reference takes the largest violation, adds 1: 4 u of the largest term for the kernel's norm, difference and sum, and the 3 u + 2 u
                # that recovering its inputs and alpha itself costs
                _, a_exp, who = nr.cone_shift(pre, -GAMMA, 1.)
                w[which + " alpha" + tag] = max(w.get(which + " alpha" + tag, 0.), abs(float(a_dev - a_exp)) / (9 * U * big))
                # ... and against the reference's own alpha, whose inputs carry the field's bar (a norm of D entries: 1 + sqrt(D) of it)
                w[which + " alpha, reference" + tag] = max(w.get(which + " alpha, reference" + tag, 0.), abs(float(a_dev - alpha)) / (bpre * (1 + np.sqrt(Dmax)) + 9 * U * big))
                where.add((which, "none" if who is None else L.cones[who][1][0][0]))
        for tag, o in zip(("", " (other start values)"), outs):
            w["x" + tag] = max(w.get("x" + tag, 0.), float(np.abs(primal_values(d, L, o).astype(LD) - xr).max()) / bx)
            ey = float(np.abs(np.array([o["G_LAM"][k] for k in L.ekeys]).astype(LD) - yr).max())
            if by == 0.:  # SCvx: S = 0 decouples sigma and the cost touches no variable of an equality row -- the least-norm multipliers are exactly zero
                assert ey == 0., (lab, ey)
            else:
                w["y" + tag] = max(w.get("y" + tag, 0.), ey / by)
            fx = ~field_masks(d, None)["F_DW"]
            assert (bits(o["F_W"][fx]) == bits(d["W"][fx])).all(), lab  # fixed variables keep their values
        seen |= {L.cones[i][0] for i in (ref.who_s, ref.who_z) if i is not None}
        never_unviolated(L, ref, lab)
    assert not {w_ for w_ in where if w_[1] == "none"}, where
    report(probe, "COLD worst error / bar", worst)
    print(f"[newton step] {probe.backend} COLD largest violation in: {sorted(seen)}")
    assert all(v <= 1. for w in worst.values() for v in w.values()), worst
    assert {"segment LP row", "wave-uniform row"} <= seen and seen & {"stage cone", "stage LP row"}, seen
    print(f"[newton step] {probe.backend} COLD largest violation, by the stored entries: {sorted(where)}")
    # the largest violation sits in a stage row, in a segment row and in the sigma cone sc3 (the instance with sigbar = 1e3), each at least once
    assert {w_[1] for w_ in where} >= {"st", "sc"} and {w_[1] for w_ in where} & {"s1", "s2"}, where


def test_warm_start(probe):
    """WARM (solveWarmInit, both forms of the set-up schedule, bitwise equal): s = h - G x re-evaluated on the data within (n + 1) u T plus 2 u for the
    shift, z kept and shifted ((D + 4) u of the largest term: a norm of D entries and two sums), against newton_reference.WarmStart; primal variables and
    multipliers bitwise unchanged; the start point strictly inside every cone.  Both cases of the shift occur: the slacks of the benign points do not match
    the data (large violations, in whichever cone), their duals are interior (nothing violated: the shift is theta alone, asserted at least once)."""
    keys = [(m, K, scvx, "benign", 0) for scvx in (False, True) for m in range(4) for K in SMALL_K] + [(0, 63, False, "benign", 0), (0, 64, True, "benign", 0)]
    jobs, refs = [], []
    for key in keys:
        d = get_case(probe, *key)
        for v0 in (0, 1):
            jobs.append((dict(d, setup_v0=v0), 0, "WARM"))
        refs.append(nr.WarmStart(d, 1e-2))
    run = Run(probe, jobs)
    worst, thetas = {}, 0
    for i, (key, ref) in enumerate(zip(keys, refs)):
        d, L = jobs[2 * i][0], ref.L
        o, o1 = run.arena.outputs(2 * i, run.after), run.arena.outputs(2 * i + 1, run.after)
        for f in range(run.arena.NB):
            assert (bits(run.arena.block(2 * i, f)) == bits(run.arena.block(2 * i + 1, f))).all(), (key, probe.blocks[f])
        w = worst.setdefault(MODELS[d["model"]], {})
        got_s, got_z = cone_values(d, L, o, "s"), cone_values(d, L, o, "z")
        big = max(float(np.abs(np.concatenate(ref.s)).max()), abs(float(ref.alpha_s)))
        bpre = max(float(((n + 1) * U * T).max()) for n, T in zip(ref.n, ref.T))
        Dmax = max(len(k_) for _, k_ in L.cones)
        w["s"] = max(w.get("s", 0.), max(float(np.abs(g.astype(LD) - r_).max()) for g, r_ in zip(got_s, ref.s)) / (bpre * (2 + np.sqrt(Dmax)) + 2 * U * big))
        bigz = max(float(np.abs(np.concatenate(ref.z)).max()), abs(float(ref.alpha_z)))
        w["z"] = max(w.get("z", 0.), max(float(np.abs(g.astype(LD) - r_).max()) for g, r_ in zip(got_z, ref.z)) / ((Dmax + 4) * U * bigz))
        assert all(nr.violation(np.asarray(v, dtype=LD)) < 0 for v in got_s + got_z), key
        for n, src in (("F_W", "W"), ("F_DL", "DL"), ("G_NU", "NU"), ("G_NUB", "NUB"), ("G_LAM", "LAM")):
            assert (bits(o[n]) == bits(d[src])).all(), (key, n)
        assert all(o["glob"][n] == d["glob"][n] for n in ("sig", "dsg", "n1", "sigbar")), key
        thetas += float(ref.alpha_z) == 1e-2
    report(probe, "WARM worst error / bar", worst)
    assert all(v <= 1. for w in worst.values() for v in w.values()), worst
    assert thetas >= 1  # the duals of the benign points are interior: their shift is theta alone


# ---------------------------------------------------------------- the host side of the probe
def test_host_refuses_what_the_phases_do_not_admit(probe):
    """before anything is launched (the arena keeps every bit), with the return codes of the other probes: 2 a bad count, 3 a job description the phases
    do not admit (model, policy, horizon, op, schedule flag), 4 a block that does not lie inside the arena or is not aligned as the product aligns it"""
    ar = Arena(probe, [(get_case(probe, 1, 3, False, "benign", 0), 0, "ITER"), (get_case(probe, 2, 4, True, "benign", 0), 1, "WARM")])
    before = ar.a.copy()
    assert probe.run_rc(ar.desc[:0], ar.offs[:0], ar.a) == 2
    for col, bad_values in ((0, (-1, 4)), (1, (-1, 2)), (2, (2, 65)), (3, (-1, len(probe.ops))), (4, (-1, 2))):
        for v in bad_values:
            desc = ar.desc.copy()
            desc[1, col] = v
            assert probe.run_rc(desc, ar.offs, ar.a) == 3, (col, v)
    for f in range(ar.NB):
        for v in (-2, ar.a.size - ar.sizes[1][f] + 2, ar.a.size + 16):
            offs = ar.offs.copy()
            offs[1, f] = v
            assert probe.run_rc(np.ascontiguousarray(ar.desc), offs, ar.a) == 4, (probe.blocks[f], v)
    offs = ar.offs.copy()
    offs[0, ar.B["fac"]] += 2  # inside the arena, off the 128-byte line
    assert probe.run_rc(ar.desc, offs, ar.a) == 4
    assert (bits(ar.a) == bits(before)).all()

"""The residual pass of the interior-point solver (csrc/ipm_solve.h: phResiduals), alone, its fused form (the previous iteration's step applied on the
way in) and the two phases the fused form claims to equal (phUpdate, then phResiduals), on the wave emulator (`emu`) and on the device (`hip`, marked
gpu), through tests/phase_probe/phase_probe.cpp: the product's geometry, one wavefront per instance, every record block a slice of one arena.

What is compared with what
  * RES against phase_reference.py: the literal problem as matrices, rz = s - (h - G x), ry = E x - e, rx = c + G'z + E'y, mpmath at 50 digits for
    K = 3, 4 and longdouble for K = 50, 63, 64.
  * FUSED: the new point's stage fields and wave-uniform scalars against x + alpha dx of the reference; the residuals it stores against the reference's
    residuals AT THE POINT IT STORED (the pass keeps the new point in registers: what it stores is what it evaluated).
  * FUSED against TWO_PHASE, the LDS-resident segment fields against the workspace-resident ones, the wavefront shift against the second load
    (device only): every double of the arena bitwise, no tolerance.

Bars.  Every stored entry is a sum of n terms, each a product of at most three factors (mul * coef * w of a table row: two roundings; a dynamics
term: one).  Summed by n - 1 additions in any bracketing -- a chain, or per-lane chains under the six levels of the DPP tree of a wave sum, which is
shallower -- the longest path has at most n + 1 roundings: the bar is (n + 1) u T, u = 2^-53, T = the sum of the absolute values of the terms as the
reference has them (a fused multiply-add only removes roundings).  Counts:
    F_RZ       s, the row's terms (<= 3), its constant: n <= 5          F_RXD   wtrx, z_0: n = 2
    G_RY       NXV + 2 NUV + 4 (x_{k+1}, S sigma, nu, Z, and A x, B u, C u)
    F_RXW_j    the rows of G that carry w_j (<= 4) + NL terms of M' lam + NL (an input) or 1 (a state) of N' lam
    rzs 3, rzc 3, rxds 3, rxn1 2
    rz3        s3 - (n1 - sum nu_b): a lane's chain of NL terms, 6 tree levels, 2 subtractions: (NL + 8) u T
    rxs        w_t - zs - zc3_2 - sum S lam: a product, a lane's chain of NL, 6 tree levels, 3 subtractions: (NL + 10) u T
    gap        the longest lane's chain 2 NL + NS products, 6 tree levels, 5 scalar products: (2 NL + NS + 12) u T
    pcost      K terms under the tree (1 + 6) and three products: 11 u T;   mu = gap / D: the gap's bar / D + u |mu|
    pres, dres relative: half the relative bar of every sum of squares under a root (an entry r with bar b contributes 2 |r| b + b^2; the sum itself
               (2 NL + NS + NV + 15) u), plus 4 u for the roots, the sum and the quotient; of the two quotients of pres the larger bar.
    stepped fields  x + alpha dx: 2 u (|x| + |alpha dx|)
Each bar is also asserted to be at most 1e-6 of the largest entry of its field.

Masked reads.  Lane K - 1 has no segment and lane 0 no previous one: both read segment 0 through the clamped views (lam, nu, the dynamics row, and on
the emulator the C row) and multiply lam by the zero masks mk / mp; the row residual a lane without a segment forms from those reads is neither stored
nor summed.  Segment 0's data therefore must not reach stage K - 1 (K > 2) or lane 0's N' lam term.

The seven segment fields after the fused step (nu, nu_b, lam, s1, z1, s2, z2) against phase_reference.segment_step, the six Newton equations of the row
solved directly (ds, dz eliminated, the 2 x 2 system by Cramer's rule; not segRhsRow / segDirRow's condensed formulas).
    lam        lam + alpha_d (vl - bcl dsigma): n = 3 terms, 4 u T, on every population
    the others a quotient has no "sum of the terms"; the bar is the first-order running error bound of that direct solution, evaluated by the reference
               (phase_reference.Err): every + - * adds u |result|, every quotient 3 u |result| (the kernel forms it as a reciprocal within one ulp, 2 u,
               times the numerator), and the operands' bounds are carried on with the absolute values of the partial derivatives, never cancelling.
               The kernel's condensed formulas evaluate the same quantities (d_i = z_i / s_i, t_i = e_i, E^-1, q) in an order of their own, with fewer operations than
               the direct solution spends; the bound lets no error term cancel.
  Both populations are asserted.  On the late one the bars of z1, z2 alone are exempt from "at most 1e-6 of the field's largest entry" (they are 6e-5 ..
  9e-5 of it): with s = 1e-10 and sigma mu = 0.016 the step dz = (sigma mu - p) / s - ... passes through terms of 1e8 that cancel to O(1), in the direct
  solution as in any float64 evaluation -- a property of that point (no iterate of a solve pairs that mu with those slacks), stated by the bar itself.
What the step stores there is also pinned bitwise against phUpdate, and the residuals it forms are checked at the stored point."""
import ctypes
import os

import numpy as np
import pytest

import phase_reference as pr
from phase_reference import NV, U
from test_constraint_rows import Probe as RowsProbe

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
MODELS = ["RocketQuatSC", "Rocket2dSC", "Lander3dofSC", "ZeroOrderHold<RocketQuatSC>"]
OFF_N = 8
O_ST, O_SG, O_DY, O_SX, O_IP, O_GLOB, O_ITER, O_UNUSED = range(OFF_N)
OP_RES, OP_FUSED, OP_TWO_PHASE = range(3)
SENTINEL = np.uint64(0x7FF4DEADBEEF0000)  # a signalling NaN between and around the record blocks; the low 16 bits carry the position
PAYLOAD = np.uint64(0x7FF8000000000000)   # quiet NaNs inside the record blocks: (block << 32 | index in the block) + 1 in the low bits
SMALL_K, LARGE_K, NINST = (3, 4), (50, 63, 64), 5
SEG_STATE = ("NU", "NUB", "S1", "Z1", "S2", "Z2", "LAM")
GLOB_IN = ["sig", "dsg", "n1", "sigbar", "ss", "zs", "s3", "z3"] + ["sc3_%d" % i for i in range(3)] + ["zc3_%d" % i for i in range(3)]
GLOB_STEP = ["dsig", "ddsg", "dn1", "dss", "dzs", "ds3", "dz3"] + ["dsc3_%d" % i for i in range(3)] + ["dzc3_%d" % i for i in range(3)]
GLOB_OUT = [n for n in GLOB_IN if n != "sigbar"]  # what the step changes
ITER_IN = ["wtrx", "w_t", "w_trt", "w_vc", "resx0", "resy0", "resz0", "pres", "D", "bad", "bk_valid", "common_step"]
ITER_STEP = ["sigma_c", "alpha", "alpha_d", "mu"]
ITER_OUT = ["rzs", "rz3", "rzc_0", "rzc_1", "rzc_2", "rxs", "rxds", "rxn1", "gap", "mu", "pcost", "pres", "dres"]
ITER_BK = ["bk_sig", "bk_dsg", "bk_n1", "bk_valid"]


class Probe(RowsProbe):
    def __init__(self, path, backend):
        super().__init__(path, backend)
        self.glob_names = self.lib.phase_probe_glob_names().decode().split()
        self.iter_names = self.lib.phase_probe_iter_names().decode().split()
        self.lib.phase_probe_blown.restype = ctypes.c_double
        self.blown = self.lib.phase_probe_blown()

    def run(self, desc, offs, arena):
        assert desc.dtype == np.int32 and offs.dtype == np.int64 and arena.dtype == np.float64
        rc = self.lib.phase_probe_run(len(desc), desc.ctypes.data_as(ctypes.c_void_p), offs.ctypes.data_as(ctypes.c_void_p),
                                      arena.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(arena.size))
        assert rc == 0, rc


@pytest.fixture(scope="module", params=BACKENDS)
def probe(request):
    """the probe library of the emulation build or of the device build"""
    import __graft_entry__ as g

    if request.param == "emu":
        return Probe(os.environ.get("SCPP_PHASE_PROBE_EMU_LIBRARY") or g.build_phase_probe_emu(), "emu")
    lib = os.environ.get("SCPP_PHASE_PROBE_LIBRARY") or g.PHASE_PROBE_LIB
    if not os.path.exists(lib):
        g.build_phase_probe()
    return Probe(lib, "hip")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---------------------------------------------------------------- the instances (drawn once, shared by both backends)
def cone_point(rng, dim, tail_mask=None):
    """an interior point of a second-order cone with margin 10^U(-2, 0)"""
    t = rng.standard_normal(dim - 1)
    if tail_mask is not None:
        t = np.where(tail_mask, t, 0.)
    return np.concatenate([[np.sqrt((t ** 2).sum()) + 10. ** rng.uniform(-2., 0.)], t])


def draw(probe, model, K, scvx, pop, inst):
    """the inputs of one instance as float64 arrays (what they mean: phase_reference.py).  pop: 'benign' or 'late'"""
    lay = probe.layout(model)
    rng = np.random.default_rng([20261210, model, K, int(scvx), 0 if pop == "benign" else 1, inst])
    NL, NS, NX, NU, NXV, NVU = (lay[n] for n in ("NL", "NS", "NX", "NU", "NXV", "NVU"))
    masks = probe.masks(model, K)
    d = dict(model=model, K=K, scvx=scvx, lay=lay, act=[m[0] for m in masks], fm=[m[1] for m in masks], pop=pop)
    used = np.arange(NV) < NVU
    ip = rng.uniform(0.2, 2.0, lay["IP_N"]) * rng.choice([-1., 1.], lay["IP_N"])
    for name in ("IP_GS", "IP_TILT", "IP_WMAX", "IP_TMIN", "IP_TMAX", "IP_GIM", "IP_MDRY", "IP_TR"):
        ip[lay[name]] = abs(ip[lay[name]])
    ip[lay["IP_SCVX"]] = 1. if scvx else 0.
    d["ip"] = ip
    d["W"] = np.where(used, rng.standard_normal((K, NV)), 0.)
    d["WBAR"] = np.where(used, d["W"] + 0.3 * rng.standard_normal((K, NV)), 0.)
    d["DL"] = rng.uniform(0.5, 2., K)
    uh = rng.standard_normal((K, 3))
    d["UHAT"] = uh / np.linalg.norm(uh, axis=1, keepdims=True)
    # dynamics: the benign population of test_sweeps.py (sweep_reference.generate)
    scale = 0.1 if pop == "benign" else 0.1 / np.sqrt(NX)
    d["A"] = np.eye(NX)[None] + scale * rng.standard_normal((K - 1, NX, NX))
    d["B"] = scale * rng.standard_normal((K - 1, NX, NU))
    d["C"] = scale * rng.standard_normal((K - 1, NX, NU)) * (0. if model == 3 else 1.)
    # (late: a residual is 1e-8 of its terms and a bar (n + 1) u T must stay below 1e-6 of the field's largest entry, so the terms of one entry may
    #  exceed those of the field's largest by 1e-6 * 1e-8 / ((NL + 10) u) = 3.7 at most: the NL products S lam per lane are kept at the size of the others)
    d["Sc"], d["Zc"] = rng.standard_normal((K - 1, NX)) * (1. if pop == "benign" else 0.05), rng.standard_normal((K - 1, NX))
    S, Z = np.zeros((K, NS)), np.zeros((K, NS))
    for k in range(K):
        for c in range(lay["NCONES"]):
            if d["act"][k] & (1 << c):
                o, dim = lay["coneOff"][c], lay["coneDim"][c]
                tm = used if c == 0 else None
                S[k, o:o + dim], Z[k, o:o + dim] = cone_point(rng, dim, tm), cone_point(rng, dim, tm)
        for l in range(lay["NLP"]):
            if d["act"][k] & (1 << (lay["NCONES"] + l)):
                S[k, lay["LP0"] + l], Z[k, lay["LP0"] + l] = 10. ** rng.uniform(-2., 0., 2)
    if scvx:
        S[:, 1:1 + NXV] = Z[:, 1:1 + NXV] = 0.  # structural zeros: the record holds payloads there, the kernel reads zeros
    d["S"], d["Z"] = S, Z
    d["NU"], d["LAM"] = rng.standard_normal((K - 1, NL)), rng.standard_normal((K - 1, NL))
    d["NUB"] = np.abs(d["NU"]) + 10. ** rng.uniform(-2., 0., (K - 1, NL))
    for n in ("S1", "Z1", "S2", "Z2"):
        d[n] = 10. ** rng.uniform(-2., 0., (K - 1, NL))
    g = dict(sig=rng.uniform(1., 3.), dsg=0.3 * rng.standard_normal(), n1=rng.uniform(1., 5.), sigbar=rng.uniform(1., 3.))
    for n in ("ss", "zs", "s3", "z3"):
        g[n] = 10. ** rng.uniform(-2., 0.)
    for n in ("sc3", "zc3"):
        for i, v in enumerate(cone_point(rng, 3)):
            g["%s_%d" % (n, i)] = v
    for n in GLOB_STEP:
        g[n] = 0.1 * rng.standard_normal()
    d["glob"] = g
    it = dict(wtrx=rng.uniform(0.5, 2.), w_t=rng.uniform(0.5, 2.), w_trt=rng.uniform(0.5, 2.), w_vc=rng.uniform(0.5, 2.), resx0=rng.uniform(1., 10.),
              resy0=rng.uniform(1., 10.), resz0=rng.uniform(1., 10.), pres=rng.uniform(0.1, 1.), bad=0., bk_valid=0., common_step=0.,
              D=float(sum(bin(a).count("1") for a in d["act"]) + 2 * NL * (K - 1) + 3), sigma_c=rng.uniform(0.1, 0.5), mu=rng.uniform(0.01, 0.1),
              alpha=rng.uniform(0.3, 0.9))
    it["alpha_d"] = it["alpha"]
    d["alpha_d_split"] = rng.uniform(0.3, 0.9)
    d["iter"] = it
    # the pending step
    on = np.array([pr.active_rows(lay, a) for a in d["act"]])
    on[:, 1 + NVU:1 + NV] = False
    if scvx:
        on[:, 1:1 + NXV] = False
    d["DW"], d["DDL"] = np.where(used, rng.standard_normal((K, NV)), 0.), rng.standard_normal(K)
    d["DS"], d["DZ"] = np.where(on, 0.3 * rng.standard_normal((K, NS)), 0.), np.where(on, 0.3 * rng.standard_normal((K, NS)), 0.)
    d["P1"], d["P2"] = 1e-3 * rng.standard_normal((K - 1, NL)), 1e-3 * rng.standard_normal((K - 1, NL))
    d["VL"], d["BCL"] = rng.standard_normal((K - 1, NL)), rng.standard_normal((K - 1, NL))
    d["WBK"] = rng.standard_normal((K, NV + 1))  # a previous fall-back iterate (used by the fall-back cases only)
    if pop == "late":
        make_late(d, rng, on)
    return d


def make_late(d, rng, on):
    """s = saff(x) plus a perturbation of 1e-9 relative, s_i z_i about 1e-10, the multipliers such that every entry of rx that has a dual of its own to
    absorb it (SC mode: all; SCvx mode: all but the state columns, whose trust-region rows do not exist) cancels to 1e-8 of its terms.  Built with the
    reference in longdouble.  "Relative" is relative to the entry's TERMS T0 (those without the slack or dual that absorbs them), with a magnitude that
    is bounded below: (2 .. 4) 1e-9 T0 for a stage slack, (1 .. 2) 1e-8 T0 for an absorbing dual, random sign.  The reason is the requirement that a bar
    stay below 1e-6 of its field's largest entry: the absorbing term doubles T at most, so the largest bar of a field is 2 (n + 1) u max T0 -- 1.4e-15 max T0
    for rz (n <= 5) and 7.4e-15 max T0 for rx (n <= 2 NL + 5) -- against entries of at least 2e-9 T0 and 1e-8 T0.  A normal deviate in their place leaves
    the row with the largest terms an entry as small as it likes."""
    lay, K, scvx = d["lay"], d["K"], d["scvx"]
    NL, NS, NXV, NVU = lay["NL"], lay["NS"], lay["NXV"], lay["NVU"]
    used = np.arange(NV) < NVU
    pm = lambda shape=None: rng.choice([-1., 1.], shape) * rng.uniform(1., 2., shape)
    p9 = lambda shape=None: 1. + 1e-9 * pm(shape)
    p8 = lambda shape=None: 1. + 1e-8 * pm(shape)
    g, it = d["glob"], d["iter"]
    d["WBAR"] = np.where(used, d["W"] + 1e-10 * rng.standard_normal((K, NV)), 0.)
    d["DL"] = 1e-9 * rng.uniform(1., 2., K)
    d["ip"][lay["IP_TR"]] = 1e-9 * rng.uniform(1., 2.)
    # the LP pairs of the segment rows: z1 + z2 = z3 = w_vc, s z = 1e-10, lam = z1 - z2
    g["z3"] = it["w_vc"] * p8()
    t = rng.uniform(0.1, 0.9, (K - 1, NL))
    d["Z1"], d["Z2"] = g["z3"] * t * p8(t.shape), g["z3"] * (1. - t) * p8(t.shape)
    s1, s2 = 1e-10 / d["Z1"], 1e-10 / d["Z2"]
    d["NUB"], d["NU"] = 0.5 * (s1 + s2), 0.5 * (s2 - s1)
    d["S1"], d["S2"] = (d["NUB"] - d["NU"]) * p9(t.shape), (d["NUB"] + d["NU"]) * p9(t.shape)
    d["LAM"] = (d["Z1"] - d["Z2"]) * p8(t.shape)
    g["n1"] = float(d["NUB"].sum()) + 1e-10
    g["sigbar"] = g["sig"] - 1e-10 * rng.uniform(1., 2.)
    # slacks on the affine map
    d["S"], d["Z"] = np.zeros((K, NS)), np.zeros((K, NS))
    P = pr.Problem(d, pr.Num("ld"))
    sa, T0 = P.saff(), P.rz()
    for k in range(K):
        for i in range(NS):
            if on[k, i]:
                d["S"][k, i] = float(sa["st", k, i]) + 2e-9 * T0["st", k, i][1] * pm()
                d["Z"][k, i] = 1e-10 / d["S"][k, i] if d["S"][k, i] != 0. else 0.
    g["ss"], g["s3"] = float(sa["ss",]) * p9(), float(sa["s3",]) * p9()
    for i in range(3):
        g["sc3_%d" % i] = float(sa["sc", i]) * p9()
    # duals that absorb rx: the trust-region rows (coefficient +1 on w_j), row 0 (delta_k), zc3_2 (sigma), zc3_0 (delta_sigma); z3 is set above
    g["zs"], g["zc3_1"], g["zc3_0"], g["zc3_2"] = 0.2 * it["w_t"], 0.1, 0., 0.
    rows = [(k, j) for k in range(K) for j in range(NVU) if not (scvx and j < NXV)]
    for k, j in rows:
        d["Z"][k, 1 + j] = 0.
    terms = pr.Problem(d, pr.Num("ld")).rx_terms()
    absorb = lambda v: float(sum(v)) + 1e-8 * float(sum(abs(a) for a in v)) * pm()
    for k, j in rows:
        if ("w", k, j) in terms:
            d["Z"][k, 1 + j] = -absorb(terms["w", k, j])
    if not scvx:
        d["Z"][:, 0] = it["wtrx"] * p8(K)
    g["zc3_2"] = absorb(terms["sig",])
    g["zc3_0"] = (2. * it["w_trt"] + g["zc3_1"]) * p8()
    # such a point may meet the reduced tolerances; a backup whose pres_before it exceeds 500-fold keeps the fall-back rule out of these cases
    it["bk_valid"], it["pres"] = 1., 1e-300


CASES = {}


def get_case(probe, model, K, scvx, pop, inst):
    key = (model, K, scvx, pop, inst)
    if key not in CASES:
        CASES[key] = draw(probe, model, K, scvx, pop, inst)
    return CASES[key]


def case_keys(scvx, pop):
    return [(m, K, scvx, pop, i) for m in range(4) for K in SMALL_K for i in range(NINST)] + [(0, K, scvx, pop, 0) for K in LARGE_K]


REFS = {}


def reference(d, key):
    """Residuals of instance d: mpmath for K = 3, 4, longdouble beyond"""
    if key not in REFS:
        REFS[key] = pr.Residuals(d, "mp" if d["K"] <= 4 else "ld")
    return REFS[key]


def with_rule(d, split):
    if not split:
        return d
    e = dict(d)
    e["iter"] = dict(d["iter"], alpha_d=d["alpha_d_split"])
    return e


# ---------------------------------------------------------------- the arena
class Arena:
    """record blocks of the jobs as slices of one array of doubles: sentinels between and around them, quiet-NaN payloads in every double of a block
    that is not an input of the op"""

    def __init__(self, probe, jobs):
        """jobs: [(d, policy, op)]"""
        self.probe, self.jobs = probe, jobs
        rng = np.random.default_rng(7)
        offs, pos, self.sizes = np.zeros((len(jobs), OFF_N), dtype=np.int64), 16, []
        for q, (d, _, _) in enumerate(jobs):
            lay, K = d["lay"], d["K"]
            pitch = probe.lib.phase_probe_rec_pitch(K)
            size = [lay["STREC"] * pitch, lay["G_NFIELDS"] * lay["NL"] * pitch, lay["DYNREC"] * pitch, K * lay["XREC"], lay["IP_N"], lay["GLOB_N"],
                    lay["ITER_N"], 16]
            for f in range(OFF_N):
                if f in (O_ST, O_SX):
                    pos = (pos + 15) & ~15
                offs[q, f] = pos
                pos += size[f] + int(rng.integers(1, 24))
            self.sizes.append(size)
        self.offs = offs
        self.a = np.zeros(pos + 16)
        bits(self.a)[:] = SENTINEL | (np.arange(self.a.size, dtype=np.uint64) & np.uint64(0xFFFF))
        for q, (d, _, op) in enumerate(jobs):
            for f in range(OFF_N - 1):
                bits(self.block(q, f))[:] = PAYLOAD | (np.uint64(f) << np.uint64(32)) | (np.arange(self.sizes[q][f], dtype=np.uint64) + np.uint64(1))
            self.write_inputs(q, d, op)
        self.desc = np.array([[d["model"], policy, d["K"], op] for d, policy, op in jobs], dtype=np.int32)

    def block(self, q, f, a=None):
        return (self.a if a is None else a)[self.offs[q, f]:][:self.sizes[q][f]]

    def views(self, q, a=None):
        d = self.jobs[q][0]
        pitch = self.sizes[q][O_ST] // d["lay"]["STREC"]
        return (self.block(q, O_ST, a).reshape(-1, pitch), self.block(q, O_SG, a).reshape(-1, pitch), self.block(q, O_DY, a).reshape(-1, pitch),
                self.block(q, O_SX, a).reshape(d["K"], -1))

    def write_inputs(self, q, d, op):
        lay, K, scvx = d["lay"], d["K"], d["scvx"]
        NL, NS, NX, NU, NXV, NUV = (lay[n] for n in ("NL", "NS", "NX", "NU", "NXV", "NUV"))
        st, sg, dy, sx = self.views(q)
        step = op != OP_RES

        def put_pad(f, v):  # a stage vector that starts at the trust-region cone: SCvx keeps the payloads in rows 1 .. NXV
            for i in range(NS):
                if not (scvx and 1 <= i <= NXV):
                    st[f + i, :K] = v[:, i]

        st[lay["F_W"]:lay["F_W"] + NV, :K] = d["W"].T
        st[lay["F_DL"], :K] = d["DL"]
        st[lay["F_WBAR"]:lay["F_WBAR"] + NV, :K] = d["WBAR"].T
        st[lay["F_UHAT"]:lay["F_UHAT"] + 3, :K] = d["UHAT"].T
        put_pad(lay["F_S"], d["S"])
        put_pad(lay["F_Z"], d["Z"])
        if d.get("fallback"):
            st[lay["F_WBK"]:lay["F_WBK"] + NV + 1, :K] = d["WBK"].T
        if step:
            st[lay["F_DW"]:lay["F_DW"] + NV, :K] = d["DW"].T
            st[lay["F_DDL"], :K] = d["DDL"]
            put_pad(lay["F_DS"], d["DS"])
            put_pad(lay["F_DZ"], d["DZ"])
        for n in SEG_STATE + (("P1", "P2") if step else ()):
            f = lay["G_" + dict(P1="DS1", P2="DS2").get(n, n)] * NL
            sg[f:f + NL, :K - 1] = d[n].T
        for i in range(NL):
            for j in range(NXV):
                dy[lay["DY_A"] + i * NX + lay["XMAP"][j], :K - 1] = d["A"][:, i, lay["XMAP"][j]]
            for j in range(NUV):
                dy[lay["DY_B"] + i * NU + lay["UMAP"][j], :K - 1] = d["B"][:, i, lay["UMAP"][j]]
                dy[lay["DY_C"] + i * NU + lay["UMAP"][j], :K - 1] = d["C"][:, i, lay["UMAP"][j]]
            if not scvx:
                dy[lay["DY_S"] + i, :K - 1] = d["Sc"][:, i]
            dy[lay["DY_Z"] + i, :K - 1] = d["Zc"][:, i]
        if step:
            sx[:K - 1, lay["X_VL"]:lay["X_VL"] + NL] = d["VL"]
            if not scvx:
                sx[:K - 1, lay["X_BCL"]:lay["X_BCL"] + NL] = d["BCL"]
        self.block(q, O_IP)[:] = d["ip"]
        gl, it = self.block(q, O_GLOB), self.block(q, O_ITER)
        for n in GLOB_IN + (GLOB_STEP if step else []):
            gl[self.probe.glob_names.index(n)] = d["glob"][n]
        for n in ITER_IN + (ITER_STEP if step else []) + (ITER_BK if d.get("fallback") else []):
            it[self.probe.iter_names.index(n)] = d["iter"][n]

    def allowed(self, q, kept):
        """mask over the arena of the doubles job q may change"""
        d, _, op = self.jobs[q]
        lay, K, scvx = d["lay"], d["K"], d["scvx"]
        NL, NS, NXV = lay["NL"], lay["NS"], lay["NXV"]
        m = np.zeros(self.a.size, dtype=bool)
        st, sg, _, _ = self.views(q, m)

        def pad(f):
            for i in range(NS):
                if not (scvx and 1 <= i <= NXV):
                    st[f + i, :K] = True

        pad(lay["F_RZ"])
        st[lay["F_RXW"]:lay["F_RXW"] + NV, :K] = True
        st[lay["F_RXD"], :K] = True
        sg[lay["G_RY"] * NL:lay["G_RY"] * NL + NL, :K - 1] = True
        it = self.block(q, O_ITER, m)
        for n in ITER_OUT + (ITER_BK if kept else []):
            it[self.probe.iter_names.index(n)] = True
        if kept:
            st[lay["F_WBK"]:lay["F_WBK"] + NV + 1, :K] = True
        if op != OP_RES:
            st[lay["F_W"]:lay["F_W"] + NV, :K] = True
            st[lay["F_DL"], :K] = True
            pad(lay["F_S"])
            pad(lay["F_Z"])
            for n in SEG_STATE:
                sg[lay["G_" + n] * NL:lay["G_" + n] * NL + NL, :K - 1] = True
            gl = self.block(q, O_GLOB, m)
            for n in GLOB_OUT:
                gl[self.probe.glob_names.index(n)] = True
        return m

    def outputs(self, q, a):
        """what job q stored, from arena contents a: stage / segment fields as [k][entry] arrays, Glob and Iter as dicts"""
        d = self.jobs[q][0]
        lay, K = d["lay"], d["K"]
        NL, NS = lay["NL"], lay["NS"]
        st, sg, _, _ = self.views(q, a)
        o = {n: st[lay[n]:lay[n] + w, :K].T.copy() for n, w in (("F_RZ", NS), ("F_RXW", NV), ("F_S", NS), ("F_Z", NS), ("F_W", NV), ("F_WBK", NV + 1))}
        o["F_RXD"], o["F_DL"] = st[lay["F_RXD"], :K].copy(), st[lay["F_DL"], :K].copy()
        for n in ("RY",) + SEG_STATE:
            o["G_" + n] = sg[lay["G_" + n] * NL:lay["G_" + n] * NL + NL, :K - 1].T.copy()
        o["glob"] = dict(zip(self.probe.glob_names, self.block(q, O_GLOB, a)))
        o["iter"] = dict(zip(self.probe.iter_names, self.block(q, O_ITER, a)))
        return o


class Run:
    def __init__(self, probe, jobs):
        self.arena = Arena(probe, jobs)
        self.before = self.arena.a.copy()
        probe.run(self.arena.desc, self.arena.offs, self.arena.a)
        self.after = self.arena.a


RUNS = {}


def get_run(probe, scvx, pop, policy, op, split, tag=None):
    """all instances of one population and mode in ONE launch"""
    key = (tag or probe.backend, scvx, pop, policy, op, split)
    if key not in RUNS:
        RUNS[key] = Run(probe, [(with_rule(get_case(probe, *k), split), policy, op) for k in case_keys(scvx, pop)])
    return RUNS[key]


POPS = [(pop, scvx) for pop in ("benign", "late") for scvx in (False, True)]
POP_IDS = [f"{p}-{'SCvx' if s else 'SC'}" for p, s in POPS]
STEP_OPS = [(op, split) for op in (OP_FUSED, OP_TWO_PHASE) for split in (False, True)]


def ratio(got, ref, bar_):
    """worst |got - ref| / bar over the entries with a positive bar; entries with a zero bar must be exact; every entry must be finite"""
    got, ref, bar_ = np.atleast_1d(got), np.atleast_1d(ref), np.atleast_1d(bar_)
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), np.argwhere(~np.isfinite(np.asarray(got, dtype=np.float64)))[:8]
    worst = 0.
    for idx in np.ndindex(*got.shape):
        e = abs(float(type(ref[idx])(float(got[idx])) - ref[idx])) if not isinstance(ref[idx], float) else abs(got[idx] - ref[idx])
        if bar_[idx] == 0.:
            assert e == 0., (idx, got[idx], ref[idx])
        else:
            worst = max(worst, e / bar_[idx])
    return worst


def conv(ref_value, x):
    return type(ref_value)(float(x))


def check_residual_outputs(o, R, d, worst, label):
    """the stored residual fields and scalars `o` against the reference R of the point they were evaluated at; worst[field] collects error / bar"""
    lay, K, scvx = d["lay"], d["K"], d["scvx"]
    for n, (v, b) in R.fields.items():
        got = o[n]
        if n == "F_RZ" and scvx:  # rows 1 .. NXV are not stored in SCvx mode
            keep = np.r_[0, 1 + lay["NXV"]:lay["NS"]]
            got, v, b = got[:, keep], v[:, keep], b[:, keep]
        big = max(abs(float(t)) for t in v.ravel())
        assert b.max() <= 1e-6 * big, (label, n, b.max(), big)
        worst[n] = max(worst.get(n, 0.), ratio(got, v, b))
    for n, (v, b) in R.scalars.items():
        assert b <= 1e-6 * max(abs(float(v)), 1e-300) or n in ("rzs", "rz3", "rzc_0", "rzc_1", "rzc_2", "rxs", "rxds", "rxn1"), (label, n, b, v)
        worst[n] = max(worst.get(n, 0.), ratio(o["iter"][n], np.array([v], dtype=object), b))
    # the scalar rows are entries of the fields rz and rx: their bars against the largest entry of those
    rzmax = max(abs(float(t)) for t in R.fields["F_RZ"][0].ravel())
    rxmax = max([abs(float(t)) for t in R.fields["F_RXW"][0].ravel()] + [abs(float(R.scalars[n][0])) for n in ("rxs", "rxds", "rxn1")])
    for n in ("rzs", "rz3", "rzc_0", "rzc_1", "rzc_2"):
        assert R.scalars[n][1] <= 1e-6 * max(rzmax, abs(float(R.scalars["rz3"][0])), abs(float(R.scalars["rzs"][0]))), (label, n)
    for n in ("rxs", "rxds", "rxn1"):
        assert R.scalars[n][1] <= 1e-6 * rxmax, (label, n)


def label_of(d, inst=None):
    return f"{MODELS[d['model']]} K={d['K']} {'SCvx' if d['scvx'] else 'SC'} {d['pop']}" + ("" if inst is None else f" #{inst}")


def report(probe, what, worst):
    for model, w in sorted(worst.items()):
        print(f"[phase residuals] {probe.backend} {what} {MODELS[model]}: worst error / bar  " + "  ".join(f"{n} {v:.3f}" for n, v in w.items()))


# ---------------------------------------------------------------- the tests
@pytest.mark.parametrize("pop,scvx", POPS, ids=POP_IDS)
def test_populations_on_the_reference(probe, pop, scvx):
    """judged on the reference alone, before any kernel output is looked at: benign residuals are O(1) of their terms; late ones are differences of
    nearly equal numbers (|r| <= 1e-6 T on the median entry of rz and of the absorbable part of rx), and no instance meets the reduced tolerances"""
    for key in case_keys(scvx, pop):
        d = get_case(probe, *key)
        R = reference(d, key)
        rel = lambda res: np.array([abs(float(r[0])) / r[1] for r in res if r[1] > 0.])
        qz = rel([R.rz_[k] for k in R.rz_ if k[0] in ("s1", "s2", "ss", "s3", "sc")])
        qx = rel([R.rx_[k] for k in R.rx_ if k[0] in ("nu", "nub", "dsg", "n1") or (k[0] == "w" and not (scvx and k[2] < d["lay"]["NXV"]))])
        if pop == "benign":
            assert np.median(qz) > 1e-2 and np.median(qx) > 1e-2, label_of(d)
        else:
            assert np.median(qz) < 1e-6 and np.median(qx) < 1e-6, (label_of(d), np.median(qz), np.median(qx))
        pres, dres = float(R.scalars["pres"][0]), float(R.scalars["dres"][0])
        assert np.isfinite(pres) and np.isfinite(dres), (label_of(d), pres, dres)
        if pop == "benign":
            assert pres > 1e-3 or dres > 1e-3, (label_of(d), pres, dres)
        else:
            assert d["iter"]["bk_valid"] == 1. and pres > 10 * 500. * d["iter"]["pres"], (label_of(d), pres)


@pytest.mark.parametrize("pop,scvx", POPS, ids=POP_IDS)
def test_residuals_against_the_matrices(probe, pop, scvx):
    """RES: every stored entry within its bar of the exact value"""
    run = get_run(probe, scvx, pop, 0, OP_RES, False)
    worst = {}
    for q, key in enumerate(case_keys(scvx, pop)):
        d = get_case(probe, *key)
        check_residual_outputs(run.arena.outputs(q, run.after), reference(d, key), d, worst.setdefault(d["model"], {}), label_of(d, key[4]))
    report(probe, f"RES {pop} {'SCvx' if scvx else 'SC'}", worst)
    assert all(v <= 1. for w in worst.values() for v in w.values()), worst


@pytest.mark.parametrize("split", [False, True], ids=["common-step", "split-steps"])
@pytest.mark.parametrize("pop,scvx", POPS, ids=POP_IDS)
def test_fused_step_against_the_reference(probe, pop, scvx, split):
    """FUSED: the new point's stage fields and wave-uniform scalars within 2 u (|x| + |alpha dx|) of the reference's step, fixed variables bitwise
    unchanged; the seven segment fields within their bars of the row's Newton equations solved directly (phase_reference.segment_step); and the
    residuals it stores within their bars of the reference's residuals at the stored point"""
    run = get_run(probe, scvx, pop, 0, OP_FUSED, split)
    worst = {}
    for q, key in enumerate(case_keys(scvx, pop)):
        d = with_rule(get_case(probe, *key), split)
        lay, K = d["lay"], d["K"]
        o = run.arena.outputs(q, run.after)
        w = worst.setdefault(d["model"], {})
        fields, scalars = pr.stepped(d, "mp" if K <= 4 else "ld")
        for n, (v, b) in fields.items():
            got = o[n]
            if n == "F_W":  # fixed variables keep their bits; free ones take the step
                fx = np.array([[(d["fm"][k] >> j) & 1 for j in range(NV)] for k in range(K)], dtype=bool)
                assert (bits(got)[fx] == bits(d["W"])[fx]).all(), label_of(d, key[4])
                got, v, b = got[~fx], v[~fx], b[~fx]
            elif n in ("F_S", "F_Z") and scvx:
                keep = np.r_[0, 1 + lay["NXV"]:lay["NS"]]
                got, v, b = got[:, keep], v[:, keep], b[:, keep]
            w[n] = max(w.get(n, 0.), ratio(got, v, b))
        for n, (v, b) in scalars.items():
            w[n] = max(w.get(n, 0.), ratio(o["glob"][n], np.array([v], dtype=object), b))
        # the seven segment fields against the row's Newton equations solved directly
        seg, segbar = pr.segment_step(d, "mp" if K <= 4 else "ld"), pr.segment_bars(d)
        lam_T = np.abs(d["LAM"]) + abs(d["iter"]["alpha_d"]) * (np.abs(d["VL"]) + (0. if scvx else np.abs(d["BCL"] * d["glob"]["dsig"])))
        segbar["LAM"] = 4 * U * lam_T  # lam + alpha_d (vl - bcl dsigma): n = 3 terms
        for n in pr.SEG_OUT:
            big = max(abs(float(t)) for t in seg[n].ravel())
            if not (pop == "late" and n in ("Z1", "Z2")):
                assert segbar[n].max() <= 1e-6 * big, (label_of(d, key[4]), n, segbar[n].max(), big)
            w["G_" + n] = max(w.get("G_" + n, 0.), ratio(o["G_" + n], seg[n], segbar[n]))
        # the residuals of the point the pass stored
        so, zo = o["F_S"].copy(), o["F_Z"].copy()
        if scvx:  # rows 1 .. NXV hold the payloads there (the kernel reads zeros); a NaN anywhere else reaches the reference and fails the comparison
            so[:, 1:1 + lay["NXV"]] = zo[:, 1:1 + lay["NXV"]] = 0.
        e = dict(d, W=o["F_W"], DL=o["F_DL"], S=so, Z=zo,
                 glob=dict(d["glob"], **{n: o["glob"][n] for n in GLOB_OUT}), **{n: o["G_" + n] for n in SEG_STATE})
        R = pr.Residuals(e, "mp" if K <= 4 else "ld")
        check_residual_outputs(o, R, e, w, label_of(d, key[4]))
    report(probe, f"FUSED {pop} {'SCvx' if scvx else 'SC'} {'split' if split else 'common'}", worst)
    assert all(v <= 1. for w in worst.values() for v in w.values()), worst


@pytest.mark.parametrize("policy", [0, 1], ids=["lds", "workspace"])
@pytest.mark.parametrize("split", [False, True], ids=["common-step", "split-steps"])
@pytest.mark.parametrize("pop,scvx", POPS, ids=POP_IDS)
def test_fused_equals_two_phases_bitwise(probe, pop, scvx, split, policy):
    """phResiduals<P, true> == phUpdate ; phResiduals<P, false>: every double of the arena, Glob and Iter included"""
    a, b = get_run(probe, scvx, pop, policy, OP_FUSED, split), get_run(probe, scvx, pop, policy, OP_TWO_PHASE, split)
    assert (bits(a.before) == bits(b.before)).all()
    diff = np.flatnonzero(bits(a.after) != bits(b.after))
    assert diff.size == 0, (diff[:8], a.after[diff[:8]], b.after[diff[:8]])
    assert (bits(a.after) != bits(a.before)).sum() > 1000


@pytest.mark.parametrize("op,split", [(OP_RES, False), (OP_FUSED, False), (OP_FUSED, True)], ids=["RES", "FUSED-common", "FUSED-split"])
@pytest.mark.parametrize("pop,scvx", POPS, ids=POP_IDS)
def test_lds_equals_workspace_bitwise(probe, pop, scvx, op, split):
    """nu, nu_b, lam in LDS (SegInLds) or in the workspace (SegFieldsInWorkspace): the same arena"""
    a, b = get_run(probe, scvx, pop, 0, op, split), get_run(probe, scvx, pop, 1, op, split)
    diff = np.flatnonzero(bits(a.after) != bits(b.after))
    assert diff.size == 0, (diff[:8], a.after[diff[:8]], b.after[diff[:8]])


@pytest.fixture(scope="module")
def memory_probe():
    """the device build that loads the previous segment's C row instead of shifting it across the wavefront (-DRES_PREVLANE_MEMORY=1)"""
    import __graft_entry__ as g

    lib = os.environ.get("SCPP_PHASE_PROBE_PREVLANE_MEMORY_LIBRARY") or g.PHASE_PROBE_MEM_LIB
    if not os.path.exists(lib):
        g.build_phase_probe_prevlane_memory()
    return Probe(lib, "hip")


@pytest.mark.gpu
@pytest.mark.parametrize("pop,scvx", POPS, ids=POP_IDS)
def test_shifted_row_equals_loaded_row_bitwise(memory_probe, pop, scvx):
    """device only: the C row of the previous segment by DPP wave_shr:1 (shipped) or by a second load -- every case, K = 64 (all lanes are stages) included,
    both policies, RES and FUSED under both step rules"""
    import __graft_entry__ as g

    lib = os.environ.get("SCPP_PHASE_PROBE_LIBRARY") or g.PHASE_PROBE_LIB
    if not os.path.exists(lib):
        g.build_phase_probe()
    shipped = Probe(lib, "hip")
    assert shipped.lib.phase_probe_prevlane_memory() == 0 and memory_probe.lib.phase_probe_prevlane_memory() == 1
    for policy in (0, 1):
        for op, split in ((OP_RES, False), (OP_FUSED, False), (OP_FUSED, True)):
            a = get_run(shipped, scvx, pop, policy, op, split)
            b = get_run(memory_probe, scvx, pop, policy, op, split, tag="hip-memory")
            diff = np.flatnonzero(bits(a.after) != bits(b.after))
            assert diff.size == 0, (policy, op, split, diff[:8], a.after[diff[:8]], b.after[diff[:8]])


@pytest.mark.parametrize("op,split", [(OP_RES, False), (OP_FUSED, True)], ids=["RES", "FUSED"])
@pytest.mark.parametrize("pop,scvx", POPS, ids=POP_IDS)
def test_footprint(probe, pop, scvx, op, split):
    """everything that is not an input of the op holds a distinct quiet NaN (all `pitch` lanes): had the pass read one, an output would be NaN; it changes
    its documented outputs and nothing else -- sentinels, payloads, ip, the dynamics, in SCvx mode rows 1 .. NXV of the padded vectors, the S column and
    X_BCL -- and every documented output was written (none of these populations meets the reduced tolerances: no fall-back iterate is kept)"""
    for policy in (0, 1):
        run = get_run(probe, scvx, pop, policy, op, split)
        ar = run.arena
        changed = bits(run.after) != bits(run.before)
        may = np.zeros(ar.a.size, dtype=bool)
        for q in range(len(ar.jobs)):
            m = ar.allowed(q, kept=False)
            assert not np.isnan(run.after[m]).any(), (q, np.flatnonzero(m & np.isnan(run.after))[:8])
            # (an output that was a payload before is different now; the step's in-out fields may keep a value, e.g. a fixed variable)
            assert changed[m & np.isnan(run.before)].all(), q
            may |= m
        assert not (changed & ~may).any(), np.flatnonzero(changed & ~may)[:8]


@pytest.mark.parametrize("op,split", [(OP_RES, False), (OP_FUSED, True)], ids=["RES", "FUSED"])
def test_alone_equals_in_a_launch_of_five(probe, op, split):
    """an instance alone in a launch equals itself inside the launch of all the others: its record blocks, Glob and Iter bitwise (the payloads carry the
    position inside the block, not inside the arena)"""
    for pop, scvx in POPS:
        run = get_run(probe, scvx, pop, 0, op, split)
        for q in (2, 2 * NINST + 1, len(run.arena.jobs) - 1):
            alone = Run(probe, [run.arena.jobs[q]])
            for f in range(OFF_N - 1):
                assert (bits(alone.arena.block(0, f)) == bits(run.arena.block(q, f))).all(), (pop, scvx, q, f)


def test_masked_reads(probe):
    """segment 0's lam, dynamics row and C row replaced by other finite values: what depends on segment 0 changes (stages 0 and 1, segment 0's row
    residual, the sums), and at stage K - 1 and in the other segments' rows nothing does, although lane K - 1 and lane 0 read segment 0 through their
    clamped views.  The reference agrees: its stage K - 1 and later segments have no term of segment 0."""
    for scvx in (False, True):
        jobs, keys = [], [(m, 4, scvx, "benign", 1) for m in range(4)] + [(0, 64, scvx, "benign", 0)]
        for key in keys:
            d = get_case(probe, *key)
            rng = np.random.default_rng(3)
            e = dict(d, LAM=d["LAM"].copy(), A=d["A"].copy(), B=d["B"].copy(), C=d["C"].copy(), Zc=d["Zc"].copy())
            for n in ("LAM", "A", "B", "C", "Zc"):
                e[n][0] = rng.standard_normal(e[n][0].shape) * (0. if n == "C" and d["model"] == 3 else 1.)
            jobs += [(d, 0, OP_RES), (e, 0, OP_RES)]
        run = Run(probe, jobs)
        for i, key in enumerate(keys):
            a, b = run.arena.outputs(2 * i, run.after), run.arena.outputs(2 * i + 1, run.after)
            K = key[1]
            for n in ("F_RXW", "F_RZ", "F_RXD"):
                assert (bits(a[n][2:]) == bits(b[n][2:])).all(), (key, n)
            assert (bits(a["G_RY"][1:]) == bits(b["G_RY"][1:])).all(), key
            assert (a["F_RXW"][:2] != b["F_RXW"][:2]).any() and (a["G_RY"][0] != b["G_RY"][0]).all(), key
            # the reference: rx of stage K - 1 and ry of the later segments carry no term of segment 0
            P = pr.Problem(jobs[2 * i][0], pr.Num("ld"))
            for (terms, _) in [P.erows[k, r] for k in range(1, K - 1) for r in range(P.d["lay"]["NL"])]:
                assert all(var[0] == "sig" or var[1] >= 1 for var, _ in terms)
            assert all(k != 0 for (k, r), (terms, _) in P.erows.items() for var, _ in terms if var[0] == "w" and var[1] == K - 1)


# ---------------------------------------------------------------- the fall-back iterate
FALLBACK = ("kept", "pres_exploded", "negative_gap", "blown_cost", "blown_gap", "nan_slack")


def reference_new_point(d):
    """the instance at the point the pending step leads to, by the reference alone (longdouble, rounded to float64): x + alpha dx on the stage fields and
    the scalars, the segment rows' corrector directions from their Newton equations (phase_reference.segment_step)"""
    fields, scalars = pr.stepped(d, "ld")
    seg = pr.segment_step(d, "ld")
    tof = lambda a: np.array(a, dtype=np.longdouble).astype(np.float64)
    fx = np.array([[(d["fm"][k] >> j) & 1 for j in range(NV)] for k in range(d["K"])], dtype=bool)
    return dict(d, W=np.where(fx, d["W"], tof(fields["F_W"][0])), DL=tof(fields["F_DL"][0]), S=tof(fields["F_S"][0]), Z=tof(fields["F_Z"][0]),
                glob=dict(d["glob"], **{n: float(v) for n, (v, _) in scalars.items()}), **{n: tof(v) for n, v in seg.items()})


def fallback_case(probe, model, K, scvx, kind, op):
    """an instance whose evaluated point (RES: the point it is handed; FUSED: the point its pending step leads to) meets the reduced tolerances (huge
    data norms make pres and dres tiny, a huge w_vc makes the gap small relative to the cost), with a previous fall-back iterate in place -- and, but for
    `kept`, ONE thing that breaks it.  Returns (instance, instance at the evaluated point as the reference has it)."""
    d = get_case(probe, model, K, scvx, "benign", 3)
    d = dict(d, fallback=True, glob=dict(d["glob"]), S=d["S"].copy(),
             iter=dict(d["iter"], resx0=1e40, resy0=1e8, resz0=1e8, w_vc=1e9, bk_valid=1., pres=1., bk_sig=7., bk_dsg=-3., bk_n1=11., alpha=0.05, alpha_d=0.04))
    at = (lambda: d) if op == OP_RES else (lambda: reference_new_point(d))
    if kind == "pres_exploded":
        d["iter"]["pres"] = float(pr.Residuals(at(), "ld").scalars["pres"][0]) / 5e5
    elif kind == "negative_gap":
        # zs such that the gap of the evaluated point is -1e-8: ss zs = -(the other products + 1e-8)
        e, ld = at(), np.longdouble
        rest = pr.Residuals(e, "ld").scalars["gap"][0] - ld(e["glob"]["ss"]) * ld(e["glob"]["zs"])
        zs = -(rest + ld(1e-8)) / ld(e["glob"]["ss"])
        d["glob"]["zs"] = float(zs if op == OP_RES else zs - ld(d["iter"]["alpha_d"]) * ld(d["glob"]["dzs"]))
    elif kind == "blown_cost":
        d["iter"]["w_vc"] = 1e32
    elif kind == "blown_gap":
        d["glob"]["zs"] = -1e33  # finite and blown up: gap = -1e32 < 5e-5 and pres, dres stay tiny -- the shape of the round-5 iterate
    elif kind == "nan_slack":
        d["S"][1, d["lay"]["LP0"]] = np.nan
    return d, at()


@pytest.mark.parametrize("scvx", [False, True], ids=["SC", "SCvx"])
def test_fall_back_rule(probe, scvx):
    """keep the iterate if it meets the reduced tolerances, unless it is broken.  Kept: F_WBK is the new W, delta bitwise, bk_sig / bk_dsg / bk_n1 the new
    scalars, bk_valid 1.  Broken (pres > 500 pres_before with a backup, a negative gap with a backup, |pcost| > IPM_BLOWN, a finite gap of -1e32, a NaN in
    one slack): F_WBK and bk_* untouched bit for bit -- a previously valid backup stays in place.  The first four of these meet the reduced tolerances
    and are held back by the `broken` test alone (the round-5 bug: a blown-up iterate with pres = 0 and a hugely negative gap overwrote the backup;
    blown_gap is that shape); the NaN case does not depend on it -- pres is NaN and `pres < 1e-4` is false already -- and pins that a NaN leaves the backup
    in place.  The reference places every case on the intended side of every comparison by a factor of at least 10.  RES, and FUSED: there the new point is what is judged (by the reference's own step) and what is kept."""
    for op in (OP_RES, OP_FUSED):
        cases = [fallback_case(probe, model, K, scvx, kind, op) for model in range(4) for K in (3, 4) for kind in FALLBACK]
        jobs = [(d, 0, op) for d, _ in cases]
        # judged on the reference first
        for q, (d, e) in enumerate(cases):
            kind = FALLBACK[q % len(FALLBACK)]
            if kind == "nan_slack":
                continue
            S, it = pr.Residuals(e, "ld").scalars, d["iter"]
            pres, dres, gap, pcost = (float(S[n][0]) for n in ("pres", "dres", "gap", "pcost"))
            assert pres < 1e-5 and dres < 1e-5 and pres < 1e299 and dres < 1e299, (kind, pres, dres)
            if kind == "blown_gap":  # gap < 5e-5 holds trivially: nothing but the `broken` test holds this iterate back
                assert gap < -10 * probe.blown and pres * 10 < 500. * it["pres"] and abs(pcost) * 10 < probe.blown, (gap, pres, pcost)
                continue
            assert abs(gap) / abs(pcost) < 5e-6 and abs(gap) < probe.blown / 10, (kind, gap, pcost)
            if kind == "kept":
                assert pres * 10 < 500. * it["pres"] and gap > 1e-5 and abs(pcost) * 10 < probe.blown
            elif kind == "pres_exploded":
                assert pres > 10 * 500. * it["pres"] and gap > 1e-5 and abs(pcost) * 10 < probe.blown
            elif kind == "negative_gap":
                assert -1e-7 < gap < -1e-9 and 10 * S["gap"][1] < abs(gap) and pres * 10 < 500. * it["pres"] and abs(pcost) * 10 < probe.blown
            else:
                assert abs(pcost) > 10 * probe.blown and pres * 10 < 500. * it["pres"] and gap > 1e-5
        run = Run(probe, jobs)
        ar = run.arena
        for q, (d, _, _) in enumerate(jobs):
            kind = FALLBACK[q % len(FALLBACK)]
            o, lay, K = ar.outputs(q, run.after), d["lay"], d["K"]
            m = ar.allowed(q, kept=True) & ~ar.allowed(q, kept=False)  # F_WBK and the four bk_*
            if kind == "kept":
                assert (bits(o["F_WBK"][:, :NV]) == bits(o["F_W"])).all() and (bits(o["F_WBK"][:, NV]) == bits(o["F_DL"])).all(), (q, kind)
                for n, gname in (("bk_sig", "sig"), ("bk_dsg", "dsg"), ("bk_n1", "n1")):
                    assert bits(np.array(o["iter"][n])) == bits(np.array(o["glob"][gname])), (q, n)
                assert o["iter"]["bk_valid"] == 1.
                if op == OP_FUSED:
                    assert (o["F_W"] != d["W"]).any() and o["glob"]["sig"] != d["glob"]["sig"]
            else:
                assert (bits(run.after[m]) == bits(run.before[m])).all(), (q, kind)
                assert (o["F_WBK"] == d["WBK"]).all() and o["iter"]["bk_valid"] == 1. and o["iter"]["bk_sig"] == 7., (q, kind)
            changed = bits(run.after) != bits(run.before)
            own = np.zeros(ar.a.size, dtype=bool)
            for f in range(OFF_N):
                own[ar.offs[q, f]:ar.offs[q, f] + ar.sizes[q][f]] = True
            assert not (changed & own & ~ar.allowed(q, kept=kind == "kept")).any(), (q, kind)

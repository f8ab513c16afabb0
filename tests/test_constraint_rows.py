"""The constraint operators of the interior-point solver (csrc/ipm_kernel.h: saff, Lmul, LTmul), alone: every row is EVALUATED and compared, on the wave
emulator (`emu`) and on the device (`hip`, marked gpu), through tests/phase_probe/phase_probe.cpp (one lane per item).

The reference shares nothing with the template machinery: the probe hands the constraint table over as data (cones, rows, up to three terms
(var, coef, mul) and a constant (hpar, hmul) per row), and the test assembles from it the literal matrices G [NS][17] and h [NS] of one stage on the
variables (w_0 .. w_15, delta), in mpmath at 50 digits:
    saff(x) = h - G x        Lmul(d) = -G d        LTmul(v) = -G' v   (the w part; its delta part is v_0)
with the rows of inactive cones / LP rows, the padding rows and, in SCvx mode, the state rows 1 .. NXV of the trust-region cone set to zero, and the
columns of fixed variables zero in LTmul.  SCvx mode: delta is a constant (row 0 of saff is ip[IP_TR], row 0 of Lmul is 0).

Bars.  An entry is a sum of n terms, each a product of at most three factors (mul * coef * w: two roundings); summing n terms takes n - 1 additions, so
the longest path has c = n + 1 roundings and the bar is c u T, u = 2^-53, T = the sum of the absolute values of the terms as the reference has them.
(A fused multiply-add only removes roundings.)  n: trust-region rows 2 (wbar - w), a table row its terms and its constant (<= 4), an entry of L'v the
rows that carry the variable plus the trust-region row (<= 4).

Adjointness, the property the Newton system rests on, is checked on the kernel's outputs alone, in longdouble: <Lmul(d), v> = <d, LTmul(v)> + ddelta v_0
(SC mode; in SCvx mode delta is no variable and the last term is absent), with d zero on the fixed variables and v zero on inactive rows as the header
of LTmul requires.  The IDENTITY uses no table: both sides are the kernel's outputs.  Its BAR does: it is the sum of the two sides' bars from the reference, sum_i |v_i| bar(Lmul_i) + sum_j |d_j| bar(LTmul_j), plus the longdouble sums' own 2 (NS + 17) 2^-64 T.

The table against the models' constraints as stated: the margins of RocketQuat, Rocket2D (rocketQuat / rocket2d application
constraints) and Lander3dof are written again in numpy from the states and inputs -- glide slope, tilt, angular rate, thrust bounds,
gimbal cone, the minimum thrust linearised about uhat, mass floor, Rocket2D's boxes -- and every active cone's margin s_0 - |s_1| and every active LP
row of saff(x) must equal them."""
import ctypes
import os

import mpmath
import numpy as np
import pytest

BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
MODELS = ["RocketQuatSC", "Rocket2dSC", "Lander3dofSC", "ZeroOrderHold<RocketQuatSC>"]
NV = 16
U = 2.0 ** -53
mpmath.mp.dps = 50
NITEMS = 64


class Probe:
    def __init__(self, path, backend):
        self.backend = backend
        self.lib = lib = ctypes.CDLL(path)
        for f in ("layout_names", "glob_names", "iter_names"):
            getattr(lib, "phase_probe_" + f).restype = ctypes.c_char_p
        self._lay = {}

    def layout(self, model):
        if model not in self._lay:
            out = np.zeros(self.lib.phase_probe_layout_count(), dtype=np.int32)
            assert self.lib.phase_probe_layout(model, out.ctypes.data_as(ctypes.c_void_p)) == 0
            names = self.lib.phase_probe_layout_names().decode().split()
            lay = {n: int(out[i]) for i, n in enumerate(names)}
            p = len(names)
            assert p + 80 == len(out)
            for i, n in enumerate(("XMAP", "UMAP", "XINV", "coneOff", "coneDim")):
                lay[n] = out[p + 16 * i:p + 16 * i + 16].tolist()
            rmax = self.lib.phase_probe_table_rows_max()
            ri, rd = np.zeros((rmax, 9), dtype=np.int32), np.zeros((rmax, 4))
            n = self.lib.phase_probe_table(model, ri.ctypes.data_as(ctypes.c_void_p), rd.ctypes.data_as(ctypes.c_void_p))
            assert 0 < n <= rmax
            lay["rows"] = [dict(slot=int(r[0]), cone=int(r[1]), hpar=int(r[2]), hmul=float(d[0]),
                                terms=[(int(r[3 + 2 * t]), int(r[4 + 2 * t]), float(d[1 + t])) for t in range(3) if r[3 + 2 * t] >= 0])
                           for r, d in zip(ri[:n], rd[:n])]
            self._lay[model] = lay
        return self._lay[model]

    def masks(self, model, K):
        return [(self.lib.phase_probe_active_mask(model, k, K), self.lib.phase_probe_fixed_mask(model, k, K)) for k in range(K)]

    def operators(self, model, ip, masks, w, delta, wbar, uhat, v):
        lay = self.layout(model)
        n, NS = len(w), lay["NS"]
        ins = [np.ascontiguousarray(a, dtype=t) for a, t in ((ip, np.float64), (masks, np.uint32), (w, np.float64), (delta, np.float64), (wbar, np.float64),
                                                             (uhat, np.float64), (v, np.float64))]
        assert ins[0].shape == (n, lay["IP_N"]) and ins[1].shape == (n, 2) and ins[6].shape == (n, NS)
        outs = [np.full((n, NS), np.nan), np.full((n, NS), np.nan), np.full((n, NV), np.nan), np.full(n, np.nan)]
        rc = self.lib.phase_probe_operators(model, n, *[a.ctypes.data_as(ctypes.c_void_p) for a in ins + outs])
        assert rc == 0, rc
        return outs


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


# ---------------------------------------------------------------- the items (drawn once per model and mode, shared by the backends' references)
def distinct_masks(probe, model):
    seen = []
    for K in (3, 4, 5):
        for m in probe.masks(model, K):
            if m not in seen:
                seen.append(m)
    return seen


def draw(lay, masks, scvx, seed):
    """64 items: O(1) variables, positive parameters, a unit uhat; v zero on the rows of inactive cones / LP rows, d (= w) is masked by the caller"""
    rng = np.random.default_rng(seed)
    n, NS = NITEMS, lay["NS"]
    ip = rng.uniform(0.2, 2.0, (n, lay["IP_N"])) * rng.choice([-1., 1.], (n, lay["IP_N"]))
    for name in ("IP_GS", "IP_TILT", "IP_WMAX", "IP_TMIN", "IP_TMAX", "IP_GIM", "IP_MDRY", "IP_TR"):
        ip[:, lay[name]] = np.abs(ip[:, lay[name]])
    ip[:, lay["IP_SCVX"]] = 1. if scvx else 0.
    w, wbar = rng.normal(size=(n, NV)), rng.normal(size=(n, NV))
    delta = rng.uniform(0.1, 2.0, n)
    uhat = rng.normal(size=(n, 3))
    uhat /= np.linalg.norm(uhat, axis=1, keepdims=True)
    v = rng.normal(size=(n, NS))
    mk = np.array([masks[q % len(masks)] for q in range(n)], dtype=np.uint32)
    for q in range(n):
        v[q, ~active_rows(lay, int(mk[q, 0]))] = 0.
    return dict(ip=ip, masks=mk, w=w, delta=delta, wbar=wbar, uhat=uhat, v=v, scvx=scvx)


def active_rows(lay, act):
    """[NS] bool: the slack rows of active cones / LP rows (the trust-region cone, bit 0, is always active)"""
    a = np.zeros(lay["NS"], dtype=bool)
    for c in range(lay["NCONES"]):
        if act & (1 << c):
            a[lay["coneOff"][c]:lay["coneOff"][c] + lay["coneDim"][c]] = True
    for l in range(lay["NLP"]):
        if act & (1 << (lay["NCONES"] + l)):
            a[lay["LP0"] + l] = True
    return a


def structural_zero_rows(lay, scvx):
    """rows of the trust-region cone that are zero whatever the data: padding variables, and the state rows in SCvx mode"""
    z = np.zeros(lay["NS"], dtype=bool)
    z[1 + lay["NVU"]:1 + NV] = True
    if scvx:
        z[1:1 + lay["NXV"]] = True
    return z


def coef_mp(lay, coef, ip, uhat):
    if coef == lay["CF_ONE"]:
        return mpmath.mpf(1)
    for j, name in enumerate(("CF_UHAT0", "CF_UHAT1", "CF_UHAT2")):
        if coef == lay[name]:
            return mpmath.mpf(float(uhat[j]))
    assert coef >= 0
    return mpmath.mpf(float(ip[coef]))


def matrices(lay, ip, uhat, wbar, act, scvx):
    """G [NS][17] (columns: w_0 .. w_15, delta), h [NS], and nterms_h [NS] (1 where h is a term of the row) of one stage, as the problem states them"""
    NS = lay["NS"]
    G, h = mpmath.zeros(NS, NV + 1), mpmath.zeros(NS, 1)
    hterm = np.zeros(NS, dtype=int)
    zero, on = structural_zero_rows(lay, scvx), active_rows(lay, act)
    # trust-region cone: (delta ; wbar - w), delta a constant ip[IP_TR] in SCvx mode
    if scvx:
        h[0], hterm[0] = mpmath.mpf(float(ip[lay["IP_TR"]])), 1
    else:
        G[0, NV] = -1
    for j in range(NV):
        if not zero[1 + j]:
            G[1 + j, j], h[1 + j], hterm[1 + j] = 1, mpmath.mpf(float(wbar[j])), 1
    for r in lay["rows"]:
        if not on[r["slot"]]:
            continue
        for var, coef, mul in r["terms"]:
            G[r["slot"], var] -= mpmath.mpf(mul) * coef_mp(lay, coef, ip, uhat)
        if r["hpar"] >= 0:
            h[r["slot"]], hterm[r["slot"]] = mpmath.mpf(r["hmul"]) * mpmath.mpf(float(ip[r["hpar"]])), 1
    return G, h, hterm


class Ref:
    """what the matrices give for one population: values, T (sum of |terms|) and n (number of terms) per entry"""

    def __init__(self, lay, pop):
        n, NS = NITEMS, lay["NS"]
        self.s, self.l, self.g = np.zeros((n, NS), dtype=object), np.zeros((n, NS), dtype=object), np.zeros((n, NV), dtype=object)
        self.Ts, self.Tl, self.Tg = np.zeros((n, NS)), np.zeros((n, NS)), np.zeros((n, NV))
        self.ns, self.nl, self.ng = (np.zeros((n, NS), dtype=int), np.zeros((n, NS), dtype=int), np.zeros((n, NV), dtype=int))
        for q in range(n):
            act, fm = int(pop["masks"][q, 0]), int(pop["masks"][q, 1])
            G, h, hterm = matrices(lay, pop["ip"][q], pop["uhat"][q], pop["wbar"][q], act, pop["scvx"])
            x = [mpmath.mpf(float(t)) for t in pop["w"][q]] + [mpmath.mpf(float(pop["delta"][q]))]
            v = [mpmath.mpf(float(t)) for t in pop["v"][q]]
            for i in range(NS):
                terms = [G[i, j] * x[j] for j in range(NV + 1) if G[i, j] != 0]
                self.s[q, i] = h[i] - mpmath.fsum(terms)
                self.l[q, i] = -mpmath.fsum(terms)
                self.Ts[q, i] = float(mpmath.fsum([abs(t) for t in terms]) + abs(h[i]))
                self.Tl[q, i] = float(mpmath.fsum([abs(t) for t in terms]))
                self.nl[q, i] = len(terms)
                self.ns[q, i] = len(terms) + hterm[i]
            for j in range(NV):
                terms = [] if fm & (1 << j) else [-G[i, j] * v[i] for i in range(NS) if G[i, j] != 0]
                self.g[q, j] = mpmath.fsum(terms)
                self.Tg[q, j] = float(mpmath.fsum([abs(t) for t in terms]))
                self.ng[q, j] = len(terms)


POPS = {}


def population(probe, model, scvx):
    key = (model, scvx)
    if key not in POPS:
        lay = probe.layout(model)
        pop = draw(lay, distinct_masks(probe, model), scvx, [20261201, model, int(scvx)])
        POPS[key] = (pop, Ref(lay, pop))
    return POPS[key]


OUTS = {}


def outputs(probe, model, scvx):
    key = (probe.backend, model, scvx)
    if key not in OUTS:
        pop, _ = population(probe, model, scvx)
        OUTS[key] = probe.operators(model, pop["ip"], pop["masks"], pop["w"], pop["delta"], pop["wbar"], pop["uhat"], pop["v"])
    return OUTS[key]


def worst(got, ref, T, n):
    """the worst |got - ref| in units of its bar (n + 1) u T; entries whose T is zero must be exact"""
    err = np.array([[abs(mpmath.mpf(float(g)) - r) for g, r in zip(gr, rr)] for gr, rr in zip(got, ref)], dtype=object)
    bar = (n + 1) * U * T
    assert all(float(e) == 0. for e in err[bar == 0.])
    q = np.array([float(e) for e in err[bar > 0.]]) / bar[bar > 0.]
    return float(q.max()) if q.size else 0.


CASES = [(m, scvx) for m in range(4) for scvx in (False, True)]
IDS = [f"{MODELS[m]}-{'SCvx' if s else 'SC'}" for m, s in CASES]


def is_pos_zero(a):
    return np.ascontiguousarray(a).view(np.uint64) == 0


# ---------------------------------------------------------------- the tests
def test_population_covers_every_mask(probe):
    """every distinct (activeMask, fixedMask) of K = 3 .. 5 is among the 64 items, an inactive cone or LP row among them where the model has one, and
    the items' values are O(1): a bar cannot be vacuous (T <= 1e2, so c u T <= 1e-13)"""
    for model in range(4):
        masks = distinct_masks(probe, model)
        assert 3 <= len(masks) <= NITEMS
        pop, ref = population(probe, model, False)
        assert {tuple(m) for m in pop["masks"].tolist()} == set(masks)
        assert max(ref.Ts.max(), ref.Tl.max(), ref.Tg.max()) < 1e2
        full = masks[1][0]
        assert any(a != full for a, _ in masks), "no node drops a cone: the inactive branch would not run"


@pytest.mark.parametrize("model,scvx", CASES, ids=IDS)
def test_rows_against_matrices(probe, model, scvx):
    """saff = h - G x, Lmul = -G d, LTmul = -G'v (+ v_0 for delta), every entry within (n + 1) u T of the 50-digit value"""
    pop, ref = population(probe, model, scvx)
    s, l, gw, gdl = outputs(probe, model, scvx)
    ws, wl, wg = worst(s, ref.s, ref.Ts, ref.ns), worst(l, ref.l, ref.Tl, ref.nl), worst(gw, ref.g, ref.Tg, ref.ng)
    print(f"[constraint rows] {probe.backend} {MODELS[model]} {'SCvx' if scvx else 'SC'}: worst error / bar  saff {ws:.3f}  Lmul {wl:.3f}  LTmul {wg:.3f}")
    assert ws <= 1. and wl <= 1. and wg <= 1., (ws, wl, wg)
    assert (gdl.view(np.uint64) == pop["v"][:, 0].view(np.uint64)).all()  # the delta part of L'v is v_0, copied


@pytest.mark.parametrize("model,scvx", CASES, ids=IDS)
def test_masks(probe, model, scvx):
    """inactive cones and LP rows, the rows of padding variables and, in SCvx mode, the state rows of the trust-region cone come out +0. bitwise in saff
    and Lmul; fixed and padding variables come out +0. in LTmul; row 0 of saff is delta, or ip[IP_TR] in SCvx mode, copied"""
    lay = probe.layout(model)
    pop, _ = population(probe, model, scvx)
    s, l, gw, _ = outputs(probe, model, scvx)
    zero = structural_zero_rows(lay, scvx)
    n_inactive = 0
    for q in range(NITEMS):
        act, fm = int(pop["masks"][q, 0]), int(pop["masks"][q, 1])
        off = ~active_rows(lay, act) | zero
        n_inactive += int((~active_rows(lay, act)).sum())
        assert is_pos_zero(s[q, off]).all() and is_pos_zero(l[q, off]).all(), q
        fixed = np.array([bool(fm & (1 << j)) or j >= lay["NVU"] for j in range(NV)])
        assert is_pos_zero(gw[q, fixed]).all(), q
        # and nothing else is masked: a row that is on and has a term differs from zero on these random items
        live = ~off
        live[0] = False
        assert (s[q, live] != 0.).all(), q
    assert n_inactive > 0
    row0 = pop["ip"][:, lay["IP_TR"]] if scvx else pop["delta"]
    assert (s[:, 0].view(np.uint64) == np.ascontiguousarray(row0).view(np.uint64)).all()
    if scvx:
        assert is_pos_zero(l[:, 0]).all()


@pytest.mark.parametrize("model,scvx", CASES, ids=IDS)
def test_adjointness(probe, model, scvx):
    """<Lmul(d), v> = <d, LTmul(v)> + ddelta v_0 on the kernel's outputs alone (longdouble), d masked by the fixed variables"""
    lay = probe.layout(model)
    pop, ref = population(probe, model, scvx)
    d = pop["w"].copy()
    for q in range(NITEMS):
        fm = int(pop["masks"][q, 1])
        d[q, [j for j in range(NV) if fm & (1 << j)]] = 0.
    _, l, _, _ = probe.operators(model, pop["ip"], pop["masks"], d, pop["delta"], pop["wbar"], pop["uhat"], pop["v"])
    _, _, gw, gdl = outputs(probe, model, scvx)
    # the bars of the masked d: a row's terms on fixed variables are exactly zero, so T only shrinks; the reference's T (unmasked d) bounds it
    ld = np.longdouble
    v, dl = pop["v"].astype(ld), d.astype(ld)
    lhs = (l.astype(ld) * v).sum(axis=1)
    rhs = (dl * gw.astype(ld)).sum(axis=1) + (0. if scvx else pop["delta"].astype(ld) * gdl.astype(ld))
    bar = (np.abs(pop["v"]) * (ref.nl + 1) * U * ref.Tl).sum(axis=1) + (np.abs(d) * (ref.ng + 1) * U * ref.Tg).sum(axis=1)
    T = (np.abs(l) * np.abs(pop["v"])).sum(axis=1) + (np.abs(d) * np.abs(gw)).sum(axis=1) + (0. if scvx else np.abs(pop["delta"] * gdl))
    bar = bar + 2 * (lay["NS"] + NV + 1) * 2.0 ** -64 * T
    q = np.abs(lhs - rhs).astype(np.float64) / bar
    print(f"[constraint rows] {probe.backend} {MODELS[model]} {'SCvx' if scvx else 'SC'}: adjointness, worst error / bar {q.max():.3f}")
    assert (bar < 1e-12 * np.maximum(T, 1e-3)).all()
    assert (q <= 1.).all(), q.max()


# ---------------------------------------------------------------- the table against the constraints as the models state them
def restated_margins(model, lay, x, u, ip, uhat):
    """(cone margins, LP rows) of one node in the order of the model's table, from the full state x [NX] and input u [NU] (longdouble): >= 0 is feasible.
    RocketQuat: x = (m, r(3), v(3), q = (w, x, y, z), omega(3)), u = (T(3), tau_z); Rocket2D: x = (r(2), v(2), eta, omega), u = (gimbal angle, thrust);
    Lander3dof: x = (m, r(3), v(3)), u = T(3).  The parameters are those of the instance block (tan gamma_gs, sqrt((1 - cos theta_max) / 2) or theta_max,
    w_B_max, T_min, T_max, tan gimbal_max or gimbal_max, m_dry)."""
    p = {n: np.longdouble(ip[lay["IP_" + n]]) for n in ("GS", "TILT", "WMAX", "TMIN", "TMAX", "GIM", "MDRY")}
    norm = lambda a: np.sqrt((np.asarray(a, dtype=np.longdouble) ** 2).sum())
    uh = uhat.astype(np.longdouble)
    if model in (0, 3):
        r, q, om, T = x[1:4], x[7:11], x[11:14], u[0:3]
        cones = [p["GS"] * r[2] - norm(r[:2]), p["TILT"] - norm(q[1:3]), p["WMAX"] - norm(om), p["TMAX"] - norm(T), p["GIM"] * T[2] - norm(T[:2])]
        lps = [x[0] - p["MDRY"], (uh * T).sum() - p["TMIN"]]
    elif model == 1:
        cones = [p["GS"] * x[1] - abs(x[0])]
        lps = [p["TILT"] - x[4], x[4] + p["TILT"], p["WMAX"] - x[5], x[5] + p["WMAX"], p["GIM"] - u[0], u[0] + p["GIM"], u[1] - p["TMIN"], p["TMAX"] - u[1]]
    else:
        r, T = x[1:4], u[0:3]
        cones = [p["GS"] * r[2] - norm(r[:2]), p["TMAX"] - norm(T), p["GIM"] * T[2] - norm(T[:2])]
        lps = [x[0] - p["MDRY"], (uh * T).sum() - p["TMIN"]]
    return cones, lps


def stated(lay, model, pop):
    """per item: {slack offset of the cone or LP row: restated margin}, active ones only"""
    out = []
    for q in range(NITEMS):
        x, u = np.zeros(lay["NX"], dtype=np.longdouble), np.zeros(lay["NU"], dtype=np.longdouble)
        for j in range(lay["NXV"]):
            x[lay["XMAP"][j]] = pop["w"][q, j]
        for j in range(lay["NUV"]):
            u[lay["UMAP"][j]] = pop["w"][q, lay["NXV"] + j]
        cones, lps = restated_margins(model, lay, x, u, pop["ip"][q], pop["uhat"][q])
        assert len(cones) == lay["NCONE_APP"] and len(lps) == lay["NLP"]
        act, m = int(pop["masks"][q, 0]), {}
        for c, v in enumerate(cones):
            if act & (1 << (c + 1)):
                m[lay["coneOff"][c + 1]] = (lay["coneDim"][c + 1], v)
        for l, v in enumerate(lps):
            if act & (1 << (lay["NCONES"] + l)):
                m[lay["LP0"] + l] = (1, v)
        out.append(m)
    return out


@pytest.mark.parametrize("model", range(4), ids=MODELS)
def test_table_against_stated_constraints(probe, model):
    """every active cone's margin s_0 - |s_1| and every active LP row of saff(x) equal the margin of the constraint as the model states it; the bar of a
    margin is the sum of the bars of the rows it is formed from (| |a| - |b| | <= |a - b|).  A population with a restated margin below 1e-9 of its terms
    is drawn again with the next seed (no item is left out): the comparison is of values, not of roundings of a cancelled difference."""
    lay = probe.layout(model)
    for bump in range(8):
        pop = draw(lay, distinct_masks(probe, model), False, [20261202 + bump, model])
        ref = Ref(lay, pop)
        st = stated(lay, model, pop)
        if all(abs(float(v)) >= 1e-9 * ref.Ts[q, off:off + dim].sum() for q, m in enumerate(st) for off, (dim, v) in m.items()):
            break
    else:
        raise AssertionError("no admissible population")
    s = probe.operators(model, pop["ip"], pop["masks"], pop["w"], pop["delta"], pop["wbar"], pop["uhat"], pop["v"])[0]
    worst_q, n = 0., 0
    for q, m in enumerate(st):
        for off, (dim, v) in m.items():
            rows = s[q, off:off + dim].astype(np.longdouble)
            got = rows[0] - np.sqrt((rows[1:] ** 2).sum())
            bar = ((ref.ns[q, off:off + dim] + 1) * U * ref.Ts[q, off:off + dim]).sum()
            assert bar <= 1e-12 * ref.Ts[q, off:off + dim].sum()
            worst_q = max(worst_q, float(abs(got - v)) / bar)
            n += 1
    print(f"[constraint rows] {probe.backend} {MODELS[model]}: {n} stated margins, worst error / bar {worst_q:.3f}")
    assert n >= NITEMS and worst_q <= 1., worst_q

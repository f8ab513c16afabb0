"""Reference for tests/test_phase_residuals.py that shares nothing with phResiduals / phUpdate of scpp_amd/csrc/ipm_solve.h: from the SAME inputs the
phases read it assembles the literal cone program of one sub-problem as explicit (sparse) matrices,

    minimise c'x   subject to   G x + s = h,  s in the cones,   E x = e,

on the stacked variables x = (w_k [16], delta_k per stage; nu_k, nu_b_k [NL] per segment; sigma, delta_sigma, n1), and forms

    rz = s - (h - G x)        ry = E x - e        rx = c + G'z + E'y

as matrix-vector products, then maps the entries to the kernel's fields.  Arithmetic: mpmath at 50 digits (K = 3, 4) or numpy longdouble (larger K).
Only interface constants come from the code (the probe's layout, the constraint table as data, fixedMask / activeMask); M_k and N_k of the equality
rows come from sweep_reference.blocks.

Sign conventions, read off the header comments of phResiduals and saff (ipm_kernel.h):
  * stage rows: s_k = saff(x) = h - G x: row 0 of the trust-region cone is delta_k (SCvx: the constant ip[IP_TR]), rows 1 + j are wbar_j - w_j (SCvx: the
    state rows are absent), then the table's rows; rows of inactive cones / LP rows are absent (s = 0 there);
  * segment rows: s1 = nu_b - nu, s2 = nu_b + nu;   scalar rows: ss = sigma - 0.001, s3 = n1 - sum nu_b,
    sc3 = (0.5 + 0.5 dsg, 0.5 - 0.5 dsg, sigma - sigbar);
  * equality rows (multiplier lam_k): x_{k+1} - A x_k - B u_k - C u_{k+1} - S sigma - nu_k = Z  (SCvx: S = 0), pinned states / inputs are 0 and FIXED
    variables take part with their values;
  * cost: w_t sigma + w_trt dsg + w_vc n1 + wtrx sum delta_k;
  * rx is formed for the FREE variables only (fixed ones are constants: the kernel stores 0); SCvx: delta_k is no variable (F_RXD = 0);
  * |x|^2 counts the free w, every delta_k (also in SCvx mode, where it is a constant: the kernel's convention), nu, nu_b and the three scalars.
  * termination quantities (ECOS's relative measures): pres = max(|ry| / max(1, resy0 + |x|), |rz| / max(1, resz0 + |x| + |s|)),
    dres = |rx| / max(1, resx0 + |y| + |z|), gap = s'z, mu = gap / D.

Every value comes with T, the sum of the absolute values of the terms of its defining expression, and n, the number of those terms."""
import mpmath
import numpy as np

import sweep_reference as sr

NV = 16
U = 2.0 ** -53
mpmath.mp.dps = 50


class Num:
    """the arithmetic of a reference: 'mp' or 'ld'"""

    def __init__(self, kind):
        self.kind = kind
        self.f = (lambda v: mpmath.mpf(float(v))) if kind == "mp" else (lambda v: np.longdouble(v))
        self.sqrt = mpmath.sqrt if kind == "mp" else np.sqrt
        self.zero = self.f(0.)


def term_coef(lay, coef, d, k, num):
    if coef == lay["CF_ONE"]:
        return num.f(1.)
    for j, name in enumerate(("CF_UHAT0", "CF_UHAT1", "CF_UHAT2")):
        if coef == lay[name]:
            return num.f(d["UHAT"][k, j])
    return num.f(d["ip"][coef])


def active_rows(lay, act):
    a = np.zeros(lay["NS"], dtype=bool)
    for c in range(lay["NCONES"]):
        if act & (1 << c):
            a[lay["coneOff"][c]:lay["coneOff"][c] + lay["coneDim"][c]] = True
    for l in range(lay["NLP"]):
        if act & (1 << (lay["NCONES"] + l)):
            a[lay["LP0"] + l] = True
    return a


def dynamics_blocks(d, masked):
    """M_k, N_k [K-1][NL][16] from sweep_reference.blocks (its Hessian inputs are dummies here); masked: the columns of fixed variables are zero"""
    lay, K = d["lay"], d["K"]
    s = sr.System(d["model"], dict(lay, PAT=-np.ones((NV, NV), dtype=np.int64), HS_N=0), d["fm"] if masked else [0] * K, K, d["scvx"])
    s.A, s.B, s.C = d["A"], d["B"], d["C"]
    s.e2, s.cc, s.wbt, s.hs, s.einv = np.ones(K), np.zeros(K), np.zeros((K, NV)), np.zeros((K, 1)), np.ones((K, NV))
    b = sr.blocks(s)
    return b.M, b.N


class Problem:
    """the literal problem of one instance `d` (see test_phase_residuals.py: the fields of d) as sparse rows"""

    def __init__(self, d, num):
        self.d, self.num = d, num
        lay, K, scvx, f = d["lay"], d["K"], d["scvx"], num.f
        NL, NS, NXV, NVU = lay["NL"], lay["NS"], lay["NXV"], lay["NVU"]
        g, ip = d["glob"], d["ip"]
        x, free, cost = {}, {}, {}
        for k in range(K):
            for j in range(NV):
                x["w", k, j], free["w", k, j] = f(d["W"][k, j]), not (d["fm"][k] >> j) & 1
            x["dl", k], free["dl", k] = f(d["DL"][k]), not scvx
            cost["dl", k] = f(d["iter"]["wtrx"])
        for k in range(K - 1):
            for i in range(NL):
                x["nu", k, i], x["nub", k, i] = f(d["NU"][k, i]), f(d["NUB"][k, i])
                free["nu", k, i] = free["nub", k, i] = True
        for n_, c_ in (("sig", "w_t"), ("dsg", "w_trt"), ("n1", "w_vc")):
            x[n_,], free[n_,], cost[n_,] = f(g[n_]), True, f(d["iter"][c_])
        self.x, self.free, self.cost = x, free, cost
        # G x + s = h: rows[key] = (terms [(var, coef)], h or None); s, z per key
        rows, s, z = {}, {}, {}
        for k in range(K):
            on = active_rows(lay, d["act"][k])
            for i in range(NS):
                rows["st", k, i] = ([], None)
                s["st", k, i], z["st", k, i] = f(d["S"][k, i]), f(d["Z"][k, i])
            rows["st", k, 0] = ([], f(ip[lay["IP_TR"]])) if scvx else ([(("dl", k), f(-1.))], None)
            for j in range(NVU):
                if scvx and j < NXV:
                    s["st", k, 1 + j] = z["st", k, 1 + j] = num.zero  # absent rows: the kernel reads zeros whatever the record holds
                else:
                    rows["st", k, 1 + j] = ([(("w", k, j), f(1.))], f(d["WBAR"][k, j]))
            for r in lay["rows"]:
                if on[r["slot"]]:
                    rows["st", k, r["slot"]] = ([(("w", k, var), -f(mul) * term_coef(lay, coef, d, k, num)) for var, coef, mul in r["terms"]],
                                                f(r["hmul"]) * f(ip[r["hpar"]]) if r["hpar"] >= 0 else None)
        for k in range(K - 1):
            for i in range(NL):
                rows["s1", k, i] = ([(("nub", k, i), f(-1.)), (("nu", k, i), f(1.))], None)
                rows["s2", k, i] = ([(("nub", k, i), f(-1.)), (("nu", k, i), f(-1.))], None)
                s["s1", k, i], z["s1", k, i], s["s2", k, i], z["s2", k, i] = f(d["S1"][k, i]), f(d["Z1"][k, i]), f(d["S2"][k, i]), f(d["Z2"][k, i])
        rows["ss",] = ([(("sig",), f(-1.))], f(-0.001))
        rows["s3",] = ([(("n1",), f(-1.))] + [(("nub", k, i), f(1.)) for k in range(K - 1) for i in range(NL)], None)
        rows["sc", 0] = ([(("dsg",), f(-0.5))], f(0.5))
        rows["sc", 1] = ([(("dsg",), f(0.5))], f(0.5))
        rows["sc", 2] = ([(("sig",), f(-1.))], -f(g["sigbar"]))
        s["ss",], z["ss",], s["s3",], z["s3",] = f(g["ss"]), f(g["zs"]), f(g["s3"]), f(g["z3"])
        for i in range(3):
            s["sc", i], z["sc", i] = f(g["sc3_%d" % i]), f(g["zc3_%d" % i])
        self.rows, self.s, self.z = rows, s, z
        # E x = e, multiplier lam
        M, N = dynamics_blocks(d, masked=False)
        erows, y = {}, {}
        for k in range(K - 1):
            for i in range(NL):
                t = [(("w", k, j), f(M[k, i, j])) for j in range(NVU) if M[k, i, j] != 0.] + [(("w", k + 1, j), f(N[k, i, j])) for j in range(NVU) if N[k, i, j] != 0.]
                if not scvx:
                    t.append((("sig",), -f(d["Sc"][k, i])))
                t.append((("nu", k, i), f(-1.)))
                erows[k, i], y[k, i] = (t, f(d["Zc"][k, i])), f(d["LAM"][k, i])
        self.erows, self.y = erows, y

    # every result: key -> (value, T, n)
    def rz(self):
        out = {}
        for key, (terms, h) in self.rows.items():
            v = [c * self.x[var] for var, c in terms] + [self.s[key]] + ([-h] if h is not None else [])
            out[key] = (sum(v, self.num.zero), float(sum((abs(t) for t in v), self.num.zero)), len(v))
        return out

    def saff(self):
        """h - G x per row"""
        return {key: (h if h is not None else self.num.zero) - sum((c * self.x[var] for var, c in terms), self.num.zero) for key, (terms, h) in self.rows.items()}

    def ry(self):
        out = {}
        for key, (terms, e) in self.erows.items():
            v = [c * self.x[var] for var, c in terms] + [-e]
            out[key] = (sum(v, self.num.zero), float(sum((abs(t) for t in v), self.num.zero)), len(v))
        return out

    def rx_terms(self, skip=()):
        """per free variable the terms of c + G'z + E'y; skip: slack keys whose term is left out (the caller solves for that dual)"""
        t = {var: ([self.cost[var]] if var in self.cost else []) for var, fr in self.free.items() if fr}
        for key, (terms, _) in self.rows.items():
            if key in skip:
                continue
            for var, c in terms:
                if var in t:
                    t[var].append(c * self.z[key])
        for key, (terms, _) in self.erows.items():
            for var, c in terms:
                if var in t:
                    t[var].append(c * self.y[key])
        return t

    def rx(self):
        return {var: (sum(v, self.num.zero), float(sum((abs(a) for a in v), self.num.zero)), len(v)) for var, v in self.rx_terms().items()}


def bar(n, T, extra=0):
    """(n + 1 + extra) u T: n terms, each a product of at most three factors (two roundings), summed by n - 1 additions in any bracketing"""
    return (n + 1 + extra) * U * T


class Residuals:
    """what the residual pass must store for instance d: fields[name] = (value array (object), bar array), scalars[name] = (value, bar)"""

    def __init__(self, d, kind):
        self.p = p = Problem(d, Num(kind))
        num, lay, K = p.num, d["lay"], d["K"]
        NL, NS = lay["NL"], lay["NS"]
        rz, ry, rx = p.rz(), p.ry(), p.rx()
        self.rz_, self.ry_, self.rx_ = rz, ry, rx
        F, it = {}, d["iter"]

        def arr(shape, get):
            v, b = np.zeros(shape, dtype=object), np.zeros(shape)
            for idx in np.ndindex(*shape):
                r = get(*idx)
                v[idx], b[idx] = (r[0], bar(r[2], r[1])) if r is not None else (num.zero, 0.)
            return v, b

        F["F_RZ"] = arr((K, NS), lambda k, i: rz["st", k, i])
        F["F_RXW"] = arr((K, NV), lambda k, j: rx.get(("w", k, j)))
        F["F_RXD"] = arr((K,), lambda k: rx.get(("dl", k)))
        F["G_RY"] = arr((K - 1, NL), lambda k, i: ry[k, i])
        self.fields = F
        S = {}
        # the scalar rows: a wave sum is its per-lane terms plus the six levels of the DPP tree, i.e. fewer roundings than the n - 1 of bar()
        for name, key in (("rzs", ("ss",)), ("rz3", ("s3",)), ("rzc_0", ("sc", 0)), ("rzc_1", ("sc", 1)), ("rzc_2", ("sc", 2))):
            S[name] = (rz[key][0], bar(rz[key][2], rz[key][1]))
        for name, key in (("rxs", ("sig",)), ("rxds", ("dsg",)), ("rxn1", ("n1",))):
            S[name] = (rx[key][0], bar(rx[key][2], rx[key][1]))
        # rz3 = s3 - (n1 - sum nu_b): a lane's chain of NL terms, six tree levels, two subtractions; rxs = w_t - zs - zc3_2 - sum S lam: a product, a lane's
        # chain of NL, six tree levels, three subtractions
        S["rz3"] = (rz["s3",][0], (NL + 8) * U * rz["s3",][1])
        S["rxs"] = (rx["sig",][0], (NL + 10) * U * rx["sig",][1])
        prods = [p.s[key] * p.z[key] for key in p.s]
        gap = sum(prods, num.zero)
        S["gap"] = (gap, bar(2 * NL + NS + 6 + 5, float(sum((abs(t) for t in prods), num.zero))))
        S["mu"] = (gap / it["D"], S["gap"][1] / it["D"] + U * abs(float(gap / it["D"])))
        pc = [p.cost[var] * p.x[var] for var in p.cost]
        S["pcost"] = (sum(pc, num.zero), bar(1 + 6 + 3, float(sum((abs(t) for t in pc), num.zero))))

        # sums of squares: (value, relative bar) -- each entry r with bar b contributes 2 |r| b + b^2, the sum itself (n terms + 1) u
        def sumsq(entries):
            tot = sum((r * r for r, _ in entries), num.zero)
            err = sum((2. * abs(float(r)) * b + b * b for r, b in entries), 0.)
            n = 2 * NL + NS + NV + 2 + 6 + 6  # the longest lane's terms, the tree, the scalar rows
            return tot, (err / float(tot) if tot != 0 else 0.) + (n + 1) * U

        ex = lambda r: (r[0], bar(r[2], r[1]))
        nrz = sumsq([ex(r) for r in rz.values()])
        nry = sumsq([ex(r) for r in ry.values()])
        nrx = sumsq([ex(r) for r in rx.values()])
        nxx = sumsq([(p.x[var], 0.) for var, fr in p.free.items() if fr or var[0] == "dl"])
        nss = sumsq([(v, 0.) for v in p.s.values()])
        nzz = sumsq([(v, 0.) for v in p.z.values()])
        nyy = sumsq([(v, 0.) for v in p.y.values()])
        self.sums = dict(nrz=nrz, nry=nry, nrx=nrx, nxx=nxx, nss=nss, nzz=nzz, nyy=nyy)
        f, sq = num.f, num.sqrt
        nx_, ns_, ny_, nz_ = sq(nxx[0]), sq(nss[0]), sq(nyy[0]), sq(nzz[0])
        one = f(1.)
        d1, d2, d3 = max(f(it["resy0"]) + nx_, one), max(f(it["resz0"]) + nx_ + ns_, one), max(f(it["resx0"]) + ny_ + nz_, one)
        pa, pb = sq(nry[0]) / d1, sq(nrz[0]) / d2
        # relative: half the relative bar of each sum of squares under a root, plus 4 u (two roots, a sum, a quotient)
        ra, rb = 0.5 * (nry[1] + nxx[1]) + 4 * U, 0.5 * (nrz[1] + nxx[1] + nss[1]) + 4 * U
        S["pres"] = (max(pa, pb), max(float(pa) * ra, float(pb) * rb))
        dr = sq(nrx[0]) / d3
        S["dres"] = (dr, float(dr) * (0.5 * (nrx[1] + nyy[1] + nzz[1]) + 4 * U))
        self.scalars = S


def stepped(d, kind):
    """the new point x + alpha dx, s + alpha ds, z + alpha_d dz of the stage fields and the wave-uniform scalars: {name: (value array, bar array)} with
    the bar 2 u (|x| + |alpha dx|) of a product and a sum"""
    num = Num(kind)
    f = num.f
    a, ad = f(d["iter"]["alpha"]), f(d["iter"]["alpha_d"])

    def ax(x, dx, al):
        v = np.zeros(x.shape, dtype=object)
        b = np.zeros(x.shape)
        for idx in np.ndindex(*x.shape):
            t = al * f(dx[idx])
            v[idx], b[idx] = f(x[idx]) + t, 2 * U * (abs(x[idx]) + abs(float(t)))
        return v, b

    out = dict(F_W=ax(d["W"], d["DW"], a), F_DL=ax(d["DL"], d["DDL"], a), F_S=ax(d["S"], d["DS"], a), F_Z=ax(d["Z"], d["DZ"], ad))
    g = d["glob"]
    sc = {}
    for x, dx, al in (("sig", "dsig", a), ("dsg", "ddsg", a), ("n1", "dn1", a), ("ss", "dss", a), ("zs", "dzs", ad), ("s3", "ds3", a), ("z3", "dz3", ad)) + tuple(
            ("sc3_%d" % i, "dsc3_%d" % i, a) for i in range(3)) + tuple(("zc3_%d" % i, "dzc3_%d" % i, ad) for i in range(3)):
        t = al * f(g[dx])
        sc[x] = (f(g[x]) + t, 2 * U * (abs(g[x]) + abs(float(t))))
    return out, sc


SEG_IN = ("NU", "NUB", "S1", "Z1", "S2", "Z2", "LAM", "P1", "P2", "VL", "BCL")         # per row
SEG_UNI = ("dsig", "sigma_c", "mu", "z3", "dz3", "alpha", "alpha_d")                      # wave-uniform
SEG_OUT = ("NU", "NUB", "LAM", "S1", "Z1", "S2", "Z2")


def segment_row(nu, nub, s1, z1, s2, z2, lam, p1, p2, vl, bcl, dsig, sigma_c, mu, z3, dz3, a, ad):
    """the corrector step of one segment row from its Newton equations, solved directly: with L1 = dnub - dnu, L2 = dnub + dnu,
        ds1 - L1 = -om rz1            s1 dz1 + z1 ds1 = sigmu - p1 - s1 z1         -dlam + dz1 - dz2 = -om (-lam + z1 - z2)
        ds2 - L2 = -om rz2            s2 dz2 + z2 ds2 = sigmu - p2 - s2 z2         -dz1 - dz2 + dz3  = -om (-z1 - z2 + z3)
    (om = 1 - sigma_c, sigmu = sigma_c mu, dlam = vl - bcl dsigma from the block solve): ds, dz eliminated, the 2 x 2 system in (dnu, dnub) by Cramer's rule.
    Only + - * /: the arguments are mpmath numbers or longdouble arrays.  Returns the new (nu, nub, lam, s1, z1, s2, z2)."""
    om, sigmu = 1 - sigma_c, sigma_c * mu
    dlam = vl - bcl * dsig
    rz1, rz2 = s1 - (nub - nu), s2 - (nub + nu)
    # dz_i = (c_i - z_i ds_i) / s_i with ds_i = -om rz_i + L_i:  dz_i = e_i - D_i L_i
    D1, D2 = z1 / s1, z2 / s2
    e1, e2 = (sigmu - p1 - s1 * z1 + z1 * om * rz1) / s1, (sigmu - p2 - s2 * z2 + z2 * om * rz2) / s2
    # (e1 - D1 (dnub - dnu)) - (e2 - D2 (dnub + dnu)) = dlam - om (-lam + z1 - z2)
    # (e1 - D1 (dnub - dnu)) + (e2 - D2 (dnub + dnu)) = dz3 + om (-z1 - z2 + z3)
    a11, a12, b1 = D1 + D2, D2 - D1, dlam - om * (-lam + z1 - z2) - e1 + e2
    a21, a22, b2 = D1 - D2, -(D1 + D2), dz3 + om * (-z1 - z2 + z3) - e1 - e2
    det = a11 * a22 - a12 * a21
    dnu, dnub = (b1 * a22 - a12 * b2) / det, (a11 * b2 - a21 * b1) / det
    L1, L2 = dnub - dnu, dnub + dnu
    ds1, ds2 = -om * rz1 + L1, -om * rz2 + L2
    dz1, dz2 = e1 - D1 * L1, e2 - D2 * L2
    return nu + a * dnu, nub + a * dnub, lam + ad * dlam, s1 + a * ds1, z1 + ad * dz1, s2 + a * ds2, z2 + ad * dz2


def segment_inputs(d):
    """the 18 arguments of segment_row as float64 (arrays [K-1][NL] and scalars); SCvx: the border column is absent (the kernel reads zeros)"""
    row = [d[n] if not (n == "BCL" and d["scvx"]) else np.zeros_like(d[n]) for n in SEG_IN]
    return row + [d["glob"][n] if n in d["glob"] else d["iter"][n] for n in SEG_UNI]


def segment_step(d, kind):
    """{name: new value array [K-1][NL]} of the seven segment fields"""
    args = segment_inputs(d)
    if kind == "ld":
        out = segment_row(*[np.asarray(a, dtype=np.longdouble) for a in args])
        return {n: np.array(v, dtype=object) for n, v in zip(SEG_OUT, out)}
    f = Num("mp").f
    K1, NL = args[0].shape
    out = {n: np.zeros((K1, NL), dtype=object) for n in SEG_OUT}
    for k in range(K1):
        for i in range(NL):
            for n, v in zip(SEG_OUT, segment_row(*[f(a[k, i]) for a in args[:len(SEG_IN)]], *[f(a) for a in args[len(SEG_IN):]])):
                out[n][k, i] = v
    return out


class Err:
    """a longdouble value with a first-order running bound on the rounding error a float64 evaluation of the same expression accumulates: every
    operation adds r u |result| (r = 1 for + - *, 3 for a quotient: the kernel forms it as a reciprocal within one ulp = 2 u, times the numerator) and
    carries its operands' bounds on with the absolute values of its partial derivatives.  Errors are never allowed to cancel: an upper bound on
    sum_k |d out / d v_k| |v_k| r_k u over the intermediate results v_k."""

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.longdouble)
        self.e = np.zeros(self.v.shape, dtype=np.longdouble) if e is None else e

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def _new(self, v, e, r):
        return Err(v, e + r * U * np.abs(v))

    def __neg__(self):
        return Err(-self.v, self.e)

    def __add__(self, o):
        o = Err.of(o)
        return self._new(self.v + o.v, self.e + o.e, 1)

    def __sub__(self, o):
        o = Err.of(o)
        return self._new(self.v - o.v, self.e + o.e, 1)

    def __rsub__(self, o):
        return Err.of(o) - self

    __radd__ = __add__

    def __mul__(self, o):
        o = Err.of(o)
        return self._new(self.v * o.v, np.abs(o.v) * self.e + np.abs(self.v) * o.e, 1)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Err.of(o)
        q = self.v / o.v
        return self._new(q, self.e / np.abs(o.v) + np.abs(q / o.v) * o.e, 3)


def segment_bars(d):
    """{name: bar array [K-1][NL]} of the seven stepped segment fields: the running error bound of segment_row, evaluated by the reference"""
    out = segment_row(*[Err(a) for a in segment_inputs(d)])
    return {n: o.e.astype(np.float64) for n, o in zip(SEG_OUT, out)}

"""Reference for tests/test_newton_step.py that shares nothing with the direction phases of scpp_amd/csrc/ipm_solve.h (phScalings, phRhs, phDirStage,
phDirSeg, buildHs, kktPrep, kktFinish, segRhsRow, segDirRow) and does not use the Hessian pattern PAT: from the SAME inputs the phases read it takes the
literal cone program of phase_reference.Problem,

    minimise c'x   subject to   G x + s = h,  s in the cones,   E x = e,

and states one Mehrotra iteration on it.  With rx, ry, rz of phase_reference (rz = s - (h - G x), ry = E x - e, rx = c + G'z + E'y), the Nesterov-Todd
scaling W of every cone (W z = W^-1 s = lambda), om = 1 - sigma:

    E dx = -om ry
    G'dz + E'dy = -om rx                         (free variables only; SCvx: delta_k is no variable)
    G dx + ds = -om rz
    lambda o (W dz + W^-1 ds) = -lambda o lambda + [corrector:  sigma mu e - (W^-1 ds_aff) o (W dz_aff)]

The predictor has sigma = 0 and no bracket; alpha_aff is the largest common step <= 1 that keeps s and z in their cones; sigma = clamp((1 - alpha_aff)^3,
1e-4, 1); alpha_p = clamp(min(gamma / ainv_p, 1), 1e-8, 0.999) with ainv_p the reciprocal of the largest step to the boundary of s + a ds over ALL cones
(stage cones and LP rows of active rows, the 2 NL (K - 1) segment LP rows, ss, s3, sc3), alpha_d likewise on z.  Signs are settled from the problem statement
(every equation is the linearisation of rx, ry, rz or of the complementarity s o z = sigma mu e in scaled form), not from the kernel's formulas.

How it is solved.  The last two equations give ds and dz in terms of dx cone by cone (ds = -om rz - G dx, dz = W^-1 (lambda \\ rhs) - W^-2 ds): substituted
into the second they leave the symmetric system [G'W^-2 G, E'; E, 0] (dx, dy) = rhs on ALL free variables at once -- no variable of the problem is
condensed (delta_k, nu, nu_b, sigma stay unknowns of the dense solve).  The matrix is assembled in longdouble from the sparse rows, factorised ONCE in float64
with partial pivoting, and the solution is refined with the residuals of the LITERAL second and first equations, formed in longdouble from the dz, ds the
current dx gives, until the correction is below 1e-17 relative.  All cone algebra (NT scaling from its definition, the arrow operator, its inverse) is in
longdouble here; test_newton_step.py checks it against cone_reference's mpmath versions.

The twin: the same system solved once in float64 by the same pivoted dense solve, unrefined, ds and dz recovered in float64.  Its error against the refined
solution measures the conditioning of that instance.

The start points.  Cold (ECOS, W = I): the primal start minimises |G x - h|^2 over the free variables subject to E x = e (optimality: G'(G x - h) + E'y = 0),
s = h - G x; the dual start minimises |z|^2 subject to G'z + E'y + c = 0 (optimality: z = G u, G'G u + E'y = -c, E u = 0); both are then brought into the
cone: alpha = -gamma, raised to the largest violation over all cones, plus 1, added to the first entry of every active cone and to every LP row.  Warm: s =
h - G x, z kept, both shifted by theta + the largest violation (never negative).  SCvx mode: the equality rows carry the sweeps' dual regularisation here too."""
import mpmath as mp
import numpy as np
import scipy.linalg

import cone_reference as cr
import phase_reference as pr
from sweep_reference import DUAL_REG

LD = np.longdouble
U = 2.0 ** -53


# ---------------------------------------------------------------- second-order cone algebra in longdouble, from the definitions
def jdot(x, y):
    return x[0] * y[0] - (x[1:] * y[1:]).sum()


def nt(s, z):
    """(W, W^-1, lambda) of one cone as dense matrices: wbar = (sbar + J zbar) / (2 gamma), eta = sqrt(|s|_J / |z|_J)"""
    sn, zn = np.sqrt(jdot(s, s)), np.sqrt(jdot(z, z))
    sb, zb = s / sn, z / zn
    gam = np.sqrt((1 + (sb * zb).sum()) / 2)
    w = np.concatenate([[sb[0] + zb[0]], sb[1:] - zb[1:]]) / (2 * gam)
    eta = np.sqrt(sn / zn)
    n = len(s)
    B = np.eye(n - 1, dtype=s.dtype) + np.outer(w[1:], w[1:]) / (1 + w[0])
    W, Wi = np.zeros((n, n), dtype=s.dtype), np.zeros((n, n), dtype=s.dtype)
    W[0, 0] = Wi[0, 0] = w[0]
    W[0, 1:] = W[1:, 0] = w[1:]
    Wi[0, 1:] = Wi[1:, 0] = -w[1:]
    W[1:, 1:] = Wi[1:, 1:] = B
    W, Wi = eta * W, Wi / eta
    return W, Wi, W @ z


def cprod(u, v):
    return np.concatenate([[(u * v).sum()], u[0] * v[1:] + v[0] * u[1:]])


def cdiv(lam, d):
    """x with lam o x = d"""
    x0 = (lam[0] * d[0] - (lam[1:] * d[1:]).sum()) / jdot(lam, lam)
    return np.concatenate([[x0], (d[1:] - x0 * lam[1:]) / lam[0]])


def step_inv(s, ds):
    """1 / (the largest a with s + a ds in the cone), 0 if the ray never leaves it: the smallest positive root of |s + a ds|_J^2 = 0"""
    c2, c1, c0 = jdot(ds, ds), jdot(s, ds), jdot(s, s)
    if len(s) == 1:
        return max(-ds[0] / s[0], s.dtype.type(0))
    # in t = 1 / a: c0 t^2 + 2 c1 t + c2 = 0, the LARGEST root t (c0 > 0)
    disc = c1 * c1 - c0 * c2
    roots = [(-c1 + sg * np.sqrt(max(disc, disc * 0))) / c0 for sg in (1, -1)]
    # a root belongs to the cone's boundary (not its mirror image's) when s0 t + ds0 >= 0 for t > 0
    ok = [t for t in roots if t > 0 and s[0] * t + ds[0] >= 0]
    return max(ok) if ok else s.dtype.type(0)


def violation(v):
    """-(v0 - |v1|): positive outside the cone"""
    return -(v[0] - np.sqrt((v[1:] * v[1:]).sum()))


# ---------------------------------------------------------------- the problem as cones over dense local blocks
class Literal:
    """kind 'ld': longdouble throughout; 'mp': phase_reference's mpmath numbers in object arrays (the same rows, the same order)"""

    def __init__(self, d, kind="ld"):
        self.d = d
        self.DT = DT = LD if kind == "ld" else object
        num = LD if kind == "ld" else mp.mpf
        lay, K, scvx = d["lay"], d["K"], d["scvx"]
        NL, NS, NXV, NVU, NV = lay["NL"], lay["NS"], lay["NXV"], lay["NVU"], pr.NV
        self.P = P = pr.Problem(d, pr.Num(kind))
        self.vars = [v for v, fr in P.free.items() if fr]
        self.vi = {v: i for i, v in enumerate(self.vars)}
        self.n = len(self.vars)
        self.ekeys = list(P.erows)
        self.p = len(self.ekeys)
        on = np.array([pr.active_rows(lay, a) for a in d["act"]])
        on[:, 1 + NVU:1 + NV] = False
        if scvx:
            on[:, 1:1 + NXV] = False
        self.on = on
        cones = []  # (kind, [row keys])
        for k in range(K):
            for c in range(lay["NCONES"]):
                if d["act"][k] & (1 << c):
                    o, dim = lay["coneOff"][c], lay["coneDim"][c]
                    cones.append(("stage cone", [("st", k, o + i) for i in range(dim) if on[k, o + i]]))
            for l in range(lay["NLP"]):
                if d["act"][k] & (1 << (lay["NCONES"] + l)):
                    cones.append(("stage LP row", [("st", k, lay["LP0"] + l)]))
        for k in range(K - 1):
            for i in range(NL):
                cones += [("segment LP row", [("s1", k, i)]), ("segment LP row", [("s2", k, i)])]
        cones += [("wave-uniform row", [("ss",)]), ("wave-uniform row", [("s3",)]), ("wave-uniform row", [("sc", 0), ("sc", 1), ("sc", 2)])]
        self.cones = cones
        self.D = len(cones)
        # local blocks: columns of the free variables a cone touches and its rows of G on them
        self.loc = []
        for _, keys in cones:
            cols = sorted({self.vi[v] for key in keys for v, _ in P.rows[key][0] if v in self.vi})
            pos = {c: j for j, c in enumerate(cols)}
            Gl = np.zeros((len(keys), len(cols)), dtype=DT)
            for r, key in enumerate(keys):
                for v, c in P.rows[key][0]:
                    if v in self.vi:
                        Gl[r, pos[self.vi[v]]] += c
            self.loc.append((np.array(cols, dtype=np.int64), Gl))
        self.E = np.zeros((self.p, self.n), dtype=DT)
        for r, key in enumerate(self.ekeys):
            for v, c in P.erows[key][0]:
                if v in self.vi:
                    self.E[r, self.vi[v]] += c
        # SCvx mode: the static dual regularisation of the multiplier block (sweeps.h, stated by sweep_reference): E dx - reg dy = -om ry
        self.reg = num(DUAL_REG) if scvx else num(0)
        self.cvec = np.array([P.cost.get(v, num(0)) for v in self.vars], dtype=DT)

    def svec(self, which):
        src = self.P.s if which == "s" else self.P.z
        return [np.array([src[key] for key in keys], dtype=self.DT) for _, keys in self.cones]

    def residuals(self):
        rz, ry, rx = self.P.rz(), self.P.ry(), self.P.rx()
        return ([np.array([rz[key][0] for key in keys], dtype=self.DT) for _, keys in self.cones], np.array([ry[key][0] for key in self.ekeys], dtype=self.DT),
                np.array([rx[v][0] for v in self.vars], dtype=self.DT))

    def kkt(self, W2):
        """[G'W^-2 G, E'; E, 0] in longdouble; W2: per cone the matrix W^-2 (identity for the start points)"""
        N = self.n + self.p
        M = np.zeros((N, N), dtype=LD)
        for (cols, Gl), w2 in zip(self.loc, W2):
            if len(cols):
                M[np.ix_(cols, cols)] += Gl.T @ (w2 @ Gl)
        M[self.n:, :self.n] = self.E
        M[:self.n, self.n:] = self.E.T
        M[self.n:, self.n:] = -self.reg * np.eye(self.p, dtype=LD)
        return M

    def Gt(self, vs):
        """G'v for per-cone vectors"""
        out = np.zeros(self.n, dtype=vs[0].dtype)
        for (cols, Gl), v in zip(self.loc, vs):
            if len(cols):
                out[cols] += Gl.astype(v.dtype).T @ v
        return out

    def G(self, x):
        return [Gl.astype(x.dtype) @ x[cols] if len(cols) else np.zeros(Gl.shape[0], dtype=x.dtype) for cols, Gl in self.loc]


class Solver:
    """one factorisation in float64, refinement with residuals the caller forms in longdouble"""

    def __init__(self, M):
        self.M64 = M.astype(np.float64)
        self.lu = scipy.linalg.lu_factor(self.M64)

    def solve64(self, b):
        return scipy.linalg.lu_solve(self.lu, np.asarray(b, dtype=np.float64))

    def refine(self, residual, N):
        """x with residual(x) = 0 for an affine residual whose linear part is -M"""
        x = np.zeros(N, dtype=LD)
        for _ in range(12):
            dx = self.solve64(residual(x)).astype(LD)
            x = x + dx
            if np.abs(dx).max() <= 1e-17 * max(np.abs(x).max(), LD(1e-300)):
                # one pass more: the criterion looks at the largest entry, a field of small entries is a pass behind it
                x = x + self.solve64(residual(x)).astype(LD)
                break
        else:
            raise AssertionError("refinement did not converge: the instance is too ill-conditioned for its float64 factorisation")
        return x


class Direction:
    """one direction of the literal Newton system: dx [n], dy [p], ds / dz per cone"""

    def __init__(self, dx, dy, ds, dz):
        self.dx, self.dy, self.ds, self.dz = dx, dy, ds, dz


class Newton:
    """predictor, sigma, corrector and step lengths of instance d (the state the probe's ITER ops start from); .ref and .twin"""

    def __init__(self, d, gamma, small_mp=True):
        self.L = L = Literal(d)
        self.d = d
        s, z = L.svec("s"), L.svec("z")
        self.s, self.z = s, z
        sc = [nt(a, b) for a, b in zip(s, z)]
        self.W, self.Wi, self.lam = [t[0] for t in sc], [t[1] for t in sc], [t[2] for t in sc]
        self.W2 = [wi @ wi for wi in self.Wi]
        self.rz, self.ry, self.rx = L.residuals()
        self.mu = sum((a * b).sum() for a, b in zip(s, z)) / L.D
        M = L.kkt(self.W2)
        self.M, self.solver = M, Solver(M)
        self.aff = self.solve(LD(0), None)
        # the small horizons: the system stated and solved in mpmath, handed on rounded to longdouble; the refined longdouble solve (the large
        # horizons' reference) is kept next to it as .aff_ld / .ref_ld, and test_populations_on_the_reference holds the two together
        self.mp = MpNewton(self) if small_mp and d["K"] <= MP_MAX_K else None
        if self.mp:
            self.aff_ld, aff_mp = self.aff, self.mp.solve(LD(0), None, self.aff)
            self.aff = rounded(aff_mp)
        self.aff64 = self.solve64(0., None)
        self.ainv_aff, _ = self.step_bounds(self.aff, both=True)
        a_aff = min(1 / self.ainv_aff, LD(1)) if self.ainv_aff > 0 else LD(1)
        self.sigma = min(max((1 - a_aff) ** 3, LD(1e-4)), LD(1))
        self.sigma_unclamped = (1 - a_aff) ** 3
        a64, _ = self.step_bounds(self.aff64, both=True)
        self.sigma_twin = min(max((1 - (min(1 / a64, LD(1)) if a64 > 0 else LD(1))) ** 3, LD(1e-4)), LD(1))  # (the twin's corrector uses the refined sigma)
        self.ref = self.solve(self.sigma, self.aff)
        if self.mp:  # (sigma: the mpmath predictor's, through the longdouble step bounds)
            self.ref_ld, self.ref = self.ref, rounded(self.mp.solve(self.sigma, aff_mp, self.ref))
        self.twin = self.solve64(float(self.sigma), self.aff64)
        (self.ainv_p, self.bind_p), (self.ainv_d, self.bind_d) = self.step_bounds(self.ref, both=False)
        self.alpha_p, self.alpha_d = clamp_step(gamma, self.ainv_p), clamp_step(gamma, self.ainv_d)  # split rule; common: the smaller of the two

    def cone_rhs(self, sigma, aff, dt):
        """per cone W^-1 (lambda \\ rhs) with rhs = -lambda o lambda [+ sigma mu e - (W^-1 ds_aff) o (W dz_aff)]"""
        out = []
        for i, lam in enumerate(self.lam):
            lam = lam.astype(dt)
            rhs = -cprod(lam, lam)
            if aff is not None:
                rhs = rhs - cprod(self.Wi[i].astype(dt) @ aff.ds[i], self.W[i].astype(dt) @ aff.dz[i])
                rhs[0] += dt(sigma) * dt(self.mu)
            out.append(self.Wi[i].astype(dt) @ cdiv(lam, rhs))
        return out

    def recover(self, dx, t, om, dt):
        G = self.L.G(dx)
        ds = [-om * rz.astype(dt) - g for rz, g in zip(self.rz, G)]
        dz = [ti - w2.astype(dt) @ dsi for ti, w2, dsi in zip(t, self.W2, ds)]
        return ds, dz

    def solve(self, sigma, aff):
        L, om = self.L, 1 - sigma
        t = self.cone_rhs(sigma, aff, LD)

        def residual(v):
            dx, dy = v[:L.n], v[L.n:]
            ds, dz = self.recover(dx, t, om, LD)
            return np.concatenate([-om * self.rx - L.Gt(dz) - L.E.T @ dy, -om * self.ry - L.E @ dx + L.reg * dy])

        v = self.solver.refine(residual, L.n + L.p)
        ds, dz = self.recover(v[:L.n], t, om, LD)
        return Direction(v[:L.n], v[L.n:], ds, dz)

    def solve64(self, sigma, aff):
        """the twin: the same system, one pivoted dense solve in float64, no refinement"""
        L, om, f = self.L, 1. - sigma, np.float64
        t = self.cone_rhs(sigma, aff, f)
        # at dx = 0: ds = -om rz, dz = t + om W^-2 rz
        ds0, dz0 = self.recover(np.zeros(L.n), t, om, f)
        b = np.concatenate([-om * self.rx.astype(f) - L.Gt(dz0), -om * self.ry.astype(f)])
        v = np.linalg.solve(self.solver.M64, b)
        ds, dz = self.recover(v[:L.n], t, om, f)
        return Direction(v[:L.n], v[L.n:], ds, dz)

    def schur_sigma(self):
        """(reference, twin) of the Schur complement of sigma in the system's matrix, stated without any elimination: 1 / (M^-1)[sigma, sigma]"""
        L = self.L
        i = next(j for j, v in enumerate(L.vars) if v[0] == "sig")
        b = np.zeros(L.n + L.p, dtype=LD)
        b[i] = 1
        v = self.solver.refine(lambda x: b - self.M @ x, L.n + L.p)
        return 1 / v[i], 1. / np.linalg.solve(self.solver.M64, b.astype(np.float64))[i]

    def step_bounds(self, dr, both):
        """both: one bound over s and z (the predictor's); else ((ainv_p, binding cone), (ainv_d, binding cone))"""
        bp = [step_inv(s, ds) for s, ds in zip(self.s, dr.ds)]
        bd = [step_inv(z, dz) for z, dz in zip(self.z, dr.dz)]
        if both:
            return max(max(bp), max(bd)), None
        ip_, id_ = int(np.argmax(bp)), int(np.argmax(bd))
        return (bp[ip_], ip_), (bd[id_], id_)


# ---------------------------------------------------------------- the small horizons: the same literal system in mpmath
MP_MAX_K = 4
MP_TOL = mp.mpf(10) ** -45 # (cone_reference sets 256 bits, 77 digits: the solve stops at 45 correct digits of the largest entry)


def to_mp(a):
    """longdouble -> mpf, exactly (two float64 pieces)"""
    out = []
    for x in np.asarray(a, dtype=LD).ravel():
        hi = float(x)
        out.append(mp.mpf(hi) + mp.mpf(float(x - LD(hi))))
    return np.array(out, dtype=object)


def to_ld(a):
    """mpf -> longdouble, rounded (two float64 pieces carry 64 bits and more)"""
    out = []
    for x in np.asarray(a, dtype=object).ravel():
        hi = float(x)
        out.append(LD(hi) + LD(float(x - mp.mpf(hi))))
    return np.array(out, dtype=LD)


def nt_mp(s, z):
    """(W, W^-1, lambda) of one cone as object matrices of mpf: (wbar, eta) from cone_reference.nt_scaling on the float64 data, the matrices from their
    definition W = eta [w0, w1'; w1, I + w1 w1' / (1 + w0)], W^-1 = (1 / eta) [w0, -w1'; -w1, I + w1 w1' / (1 + w0)]"""
    w, eta = cr.nt_scaling([float(a) for a in s], [float(a) for a in z])
    n = len(w)
    W, Wi = np.empty((n, n), dtype=object), np.empty((n, n), dtype=object)
    for i in range(n):
        for j in range(n):
            core = w[0] if i == j == 0 else w[max(i, j)] if min(i, j) == 0 else (1 if i == j else 0) + w[i] * w[j] / (1 + w[0])
            W[i, j], Wi[i, j] = eta * core, (-core if (i == 0) != (j == 0) else core) / eta
    return W, Wi, W @ z


class MpNewton:
    """The literal Newton system of instance N.d stated again in mpmath: phase_reference.Problem with its mpmath numbers for G, h, E, e, c and the
    residuals, cone_reference.nt_scaling for W.  Solved to MP_TOL: the float64 factorisation of the system's matrix serves as the approximate inverse,
    every residual is that of the LITERAL equations formed in mpmath, every correction is added in mpmath, so the iteration's fixed point is the
    solution of the mpmath system (each pass gains what the float64 solve is good for on that instance, six digits or more)."""

    def __init__(self, N):
        self.N, self.L = N, Literal(N.d, "mp")
        L = self.L
        assert L.vars == N.L.vars and L.ekeys == N.L.ekeys and L.cones == N.L.cones
        self.s, self.z = L.svec("s"), L.svec("z")
        sc = [nt_mp(a, b) for a, b in zip(self.s, self.z)]
        self.W, self.Wi, self.lam = [t[0] for t in sc], [t[1] for t in sc], [t[2] for t in sc]
        self.W2 = [wi @ wi for wi in self.Wi]
        self.rz, self.ry, self.rx = L.residuals()
        self.mu = sum((a * b).sum() for a, b in zip(self.s, self.z)) / L.D

    def cone_rhs(self, sigma, aff):
        out = []
        for i, lam in enumerate(self.lam):
            rhs = -cprod(lam, lam)
            if aff is not None:
                rhs = rhs - cprod(self.Wi[i] @ aff.ds[i], self.W[i] @ aff.dz[i])
                rhs[0] += sigma * self.mu
            out.append(self.Wi[i] @ cdiv(lam, rhs))
        return out

    def recover(self, dx, t, om):
        ds = [-om * rz - g for rz, g in zip(self.rz, self.L.G(dx))]
        return ds, [ti - w2 @ dsi for ti, w2, dsi in zip(t, self.W2, ds)]

    def solve(self, sigma, aff, start):
        """start: the longdouble solution (any start does: it only saves passes)"""
        L, sigma = self.L, to_mp(sigma)[0]
        om = 1 - sigma
        t = self.cone_rhs(sigma, aff)
        v = np.concatenate([to_mp(start.dx), to_mp(start.dy)])
        for _ in range(24):
            dx, dy = v[:L.n], v[L.n:]
            ds, dz = self.recover(dx, t, om)
            res = np.concatenate([-om * self.rx - L.Gt(dz) - L.E.T @ dy, -om * self.ry - L.E @ dx + L.reg * dy])
            dv = self.N.solver.solve64(np.array([float(x) for x in res]))
            v = v + np.array([mp.mpf(float(x)) for x in dv], dtype=object)
            if max(abs(float(x)) for x in dv) <= MP_TOL * max(abs(x) for x in v):
                break
        else:
            raise AssertionError("the mpmath refinement did not converge")
        ds, dz = self.recover(v[:L.n], t, om)
        return Direction(v[:L.n], v[L.n:], ds, dz)


def rounded(dr):
    return Direction(to_ld(dr.dx), to_ld(dr.dy), [to_ld(a) for a in dr.ds], [to_ld(a) for a in dr.dz])


def clamp_step(gamma, ainv):
    a = LD(gamma) / ainv if ainv > 0 else LD(1)
    return max(min(a, LD(1), LD(0.999)), LD(1e-8))


# ---------------------------------------------------------------- mapping to the kernel's fields
def fields_of(L, dr):
    """a Direction as the kernel's fields: F_DW [K][16], F_DDL [K], F_DS / F_DZ [K][NS], dnu / dnub / dlam / ds1 / dz1 / ds2 / dz2 [K-1][NL], and the wave-uniform scalars"""
    d = L.d
    lay, K = d["lay"], d["K"]
    NL, NS, NV = lay["NL"], lay["NS"], pr.NV
    dt = dr.dx.dtype
    F = dict(F_DW=np.zeros((K, NV), dtype=dt), F_DDL=np.zeros(K, dtype=dt), F_DS=np.zeros((K, NS), dtype=dt), F_DZ=np.zeros((K, NS), dtype=dt))
    for n in ("dnu", "dnub", "dlam", "ds1", "dz1", "ds2", "dz2"):
        F[n] = np.zeros((K - 1, NL), dtype=dt)
    g = {}
    for v, x in zip(L.vars, dr.dx):
        if v[0] == "w":
            F["F_DW"][v[1], v[2]] = x
        elif v[0] == "dl":
            F["F_DDL"][v[1]] = x
        elif v[0] in ("nu", "nub"):
            F["d" + v[0]][v[1], v[2]] = x
        else:
            g[{"sig": "dsig", "dsg": "ddsg", "n1": "dn1"}[v[0]]] = x
    for key, y in zip(L.ekeys, dr.dy):
        F["dlam"][key] = y
    for (_, keys), ds, dz in zip(L.cones, dr.ds, dr.dz):
        for key, a, b in zip(keys, ds, dz):
            if key[0] == "st":
                F["F_DS"][key[1], key[2]], F["F_DZ"][key[1], key[2]] = a, b
            elif key[0] in ("s1", "s2"):
                F["d" + key[0]][key[1], key[2]], F["dz" + key[0][1]][key[1], key[2]] = a, b
            elif key[0] == "ss":
                g["dss"], g["dzs"] = a, b
            elif key[0] == "s3":
                g["ds3"], g["dz3"] = a, b
            else:
                g["dsc3_%d" % key[1]], g["dzc3_%d" % key[1]] = a, b
    F["glob"] = g
    return F


# ---------------------------------------------------------------- the start points
def cone_shift(vs, start, extra):
    """ECOS bring2cone (start = -gamma, extra = 1: only violations count) or the warm start's shift (start = 0, extra = theta): alpha = start raised to the
    largest violation -(v0 - |v1|) over all cones, plus extra, added to the first entry of every cone.  Returns (shifted vectors, alpha, index of the cone with
    the largest violation or None)"""
    alpha, who = LD(start), None
    for i, v in enumerate(vs):
        viol = violation(v)
        if (viol >= 0 or start >= 0) and viol > alpha:
            alpha, who = viol, i
    alpha = alpha + LD(extra)
    out = []
    for v in vs:
        v = v.copy()
        v[0] += alpha
        out.append(v)
    return out, alpha, who


class ColdStart:
    """the ECOS start point of instance d, whose W, DL, NU, NUB, sig, dsg, n1 are the START values of the variables (fixed variables take part with their
    values): .x (dict var -> value), .s_pre / .z_pre per cone before the shift, .y, the shifted .s / .z with .alpha_s / .alpha_z; twin: the same in float64"""

    def __init__(self, d, gamma, dt=LD):
        self.L = L = Literal(d)
        P = L.P
        eye = [np.eye(len(keys), dtype=LD) for _, keys in L.cones]
        M = L.kkt(eye)
        sa = P.saff()
        s0 = [np.array([sa[key] for key in keys], dtype=LD) for _, keys in L.cones]  # h - G x0
        _, ry0, _ = L.residuals()
        x0 = np.array([P.x[v] for v in L.vars], dtype=LD)
        if dt is LD:
            solver = Solver(M)
            # minimise |G x - h|^2 s.t. E x = e:  G'(G x - h) + E'y = 0, E x - reg y = e  at x = x0 + dx
            v = solver.refine(lambda v: np.concatenate([L.Gt([s - g for s, g in zip(s0, L.G(v[:L.n]))]) - L.E.T @ v[L.n:], -ry0 - L.E @ v[:L.n] + L.reg * v[L.n:]]),
                              L.n + L.p)
            # minimise |z|^2 s.t. G'z + E'y + c = 0:  z = G u, G'G u + E'y = -c, E u - reg y = 0
            u = solver.refine(lambda u: np.concatenate([-L.cvec - L.Gt(L.G(u[:L.n])) - L.E.T @ u[L.n:], -L.E @ u[:L.n] + L.reg * u[L.n:]]), L.n + L.p)
        else:
            M64 = M.astype(np.float64)
            v = np.linalg.solve(M64, np.concatenate([L.Gt([s.astype(dt) for s in s0]), -ry0.astype(dt)]))
            u = np.linalg.solve(M64, np.concatenate([-L.cvec.astype(dt), np.zeros(L.p)]))
        self.x = dict(zip(L.vars, x0.astype(dt) + v[:L.n]))
        self.s_pre = [s.astype(dt) - g for s, g in zip(s0, L.G(v[:L.n]))]
        self.z_pre, self.y = L.G(u[:L.n]), dict(zip(L.ekeys, u[L.n:]))
        self.s, self.alpha_s, self.who_s = cone_shift([np.asarray(a, dtype=LD) for a in self.s_pre], -gamma, 1.)
        self.z, self.alpha_z, self.who_z = cone_shift([np.asarray(a, dtype=LD) for a in self.z_pre], -gamma, 1.)


class WarmStart:
    """s = h - G x re-evaluated (with T, the sum of the absolute values of its terms, and n their number), z kept; both shifted by theta + the largest
    violation (never below theta)"""

    def __init__(self, d, theta):
        self.L = L = Literal(d)
        P = L.P
        s, T, n = [], [], []
        for _, keys in L.cones:
            rows = [[c * P.x[v] for v, c in P.rows[key][0]] + ([P.rows[key][1]] if P.rows[key][1] is not None else []) for key in keys]
            s.append(np.array([(rows_h[-1] if P.rows[key][1] is not None else LD(0)) - sum(rows_h[:len(P.rows[key][0])], LD(0)) for rows_h, key in zip(rows, keys)], dtype=LD))
            T.append(np.array([float(sum(abs(t) for t in r)) for r in rows]))
            n.append(np.array([len(r) for r in rows]))
        self.s_pre, self.T, self.n = s, T, n
        self.s, self.alpha_s, _ = cone_shift(s, 0., theta)
        self.z, self.alpha_z, _ = cone_shift(L.svec("z"), 0., theta)

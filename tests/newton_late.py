"""The `late` population of tests/test_newton_step.py: an INTERIOR late iterate, built on an instance of the phase tests' `draw` -- every slack on the
affine map to 1e-9 of its terms (rz), the equality rows to 1e-8 (ry), every cone pair with s o z = (0.5 .. 2) 1e-10 and both strictly inside, and the
dual residual rx at 1e-8 of its terms wherever a dual of its own can absorb it (SC mode: everywhere; SCvx mode: all but the state columns, whose
trust-region rows do not exist).  test_phase_residuals.make_late cannot serve the Newton step: its slacks are saff(x) of a random x and its duals absorb
rx with whatever sign that takes, so neither lies in the cones (phScalings reports bad = 1).

How.  Data are chosen to fit the point, not the point to fit the data:
  * x: per stage a w_k with every application cone and LP row the stage has at a margin of (1 .. 4) 1e-2, found by minimising the convex penalty
    sum max(0, target - margin)^2 from draw's w_k (TMIN is set below TMAX and uhat near the gimbal axis so that such a point exists); the slacks are
    O(1), so the duals are mu s^-1 (perturbed): about 1e-10, and so are the cost weights, which are data (w_vc, w_trt, w_t, wtrx);
  * segment rows: z1 + z2 = z3 = w_vc, s = mu c / z, nu_b and nu from s1, s2, n1 from s3, lam from the nu column of rx;
  * scalars: dsg, sigbar put sc3 inside its cone, w_trt and w_t are what the dsg and sigma columns of rx ask for;
  * the trust-region cone: its dual's tail is what the w columns of rx ask for, its first entry wtrx (SC; one number for all stages, twice the largest
    tail) or the root that makes s0 = ip[IP_TR] (SCvx); its slack mu c z^-1 gives delta_k and the centre wbar;
  * Z of the dynamics is what the equality rows ask for.
Everything is formed in longdouble through phase_reference.Problem and rounded once."""
import numpy as np
import scipy.optimize

import phase_reference as pr
from phase_reference import NV

LD = np.longdouble
MU = 1e-10


def jinv(s):
    """s^-1 of the cone's algebra: (s0, -s1) / (s0^2 - |s1|^2)"""
    s = np.asarray(s, dtype=LD)
    return np.concatenate([[s[0]], -s[1:]]) / (s[0] * s[0] - (s[1:] * s[1:]).sum())


def stage_maps(d):
    """per stage (G [NS][NV], h [NS]) of the table's rows in float64: s = h - G w"""
    P = pr.Problem(d, pr.Num("ld"))
    lay, K = d["lay"], d["K"]
    out = []
    for k in range(K):
        G, h = np.zeros((lay["NS"], NV)), np.zeros(lay["NS"])
        for i in range(1 + NV, lay["NS"]):
            terms, hh = P.rows["st", k, i]
            for (_, _, j), c in terms:
                G[i, j] += float(c)
            h[i] = 0. if hh is None else float(hh)
        out.append((G, h))
    return out


def margins(d, k, s):
    lay = d["lay"]
    m = []
    for c in range(1, lay["NCONES"]):
        if d["act"][k] & (1 << c):
            o, dim = lay["coneOff"][c], lay["coneDim"][c]
            m.append(s[o] - np.sqrt((s[o + 1:o + dim] ** 2).sum() + 1e-300))
    for l in range(lay["NLP"]):
        if d["act"][k] & (1 << (lay["NCONES"] + l)):
            m.append(s[lay["LP0"] + l])
    return np.array(m)


def interior_w(d, k, G, h, w0, target):
    """w_k with every margin of stage k at `target` or more"""
    nvu = d["lay"]["NVU"]

    def phi(w):
        wf = np.zeros(NV)
        wf[:nvu] = w
        return (np.maximum(0., 2. * target - margins(d, k, h - G @ wf)) ** 2).sum()

    res = scipy.optimize.minimize(phi, w0[:nvu], method="BFGS", options=dict(gtol=1e-12, maxiter=2000))
    w = np.zeros(NV)
    w[:nvu] = res.x
    m = margins(d, k, h - G @ w)
    assert m.size == 0 or m.min() >= target, (k, m)
    return w


def make_interior_late(d, rng):
    lay, K, scvx = d["lay"], d["K"], d["scvx"]
    NL, NS, NXV, NVU = lay["NL"], lay["NS"], lay["NXV"], lay["NVU"]
    pm = lambda shape=None: rng.choice([-1., 1.], shape) * rng.uniform(1., 2., shape)
    p9 = lambda shape=None: 1. + 1e-9 * pm(shape)
    p8 = lambda shape=None: 1. + 1e-8 * pm(shape)
    cc = lambda shape=None: MU * rng.uniform(0.5, 2., shape)  # s o z of a pair
    d = dict(d, pop="late", glob=dict(d["glob"]), iter=dict(d["iter"]), ip=d["ip"].copy(), **{n: d[n].copy() for n in ("W", "WBAR", "DL", "UHAT", "S", "Z", "Zc")})
    g, it, ip = d["glob"], d["iter"], d["ip"]
    ip[lay["IP_TMIN"]] = rng.uniform(0.2, 0.5) * ip[lay["IP_TMAX"]]
    uh = np.concatenate([0.2 * rng.standard_normal((K, 2)), np.ones((K, 1))], axis=1)
    d["UHAT"] = uh / np.linalg.norm(uh, axis=1, keepdims=True)
    # the segment rows and n1
    it["w_vc"] = MU * rng.uniform(0.5, 2.)
    g["z3"] = it["w_vc"] * p8()
    t = rng.uniform(0.1, 0.9, (K - 1, NL))
    d["Z1"], d["Z2"] = g["z3"] * t * p8(t.shape), g["z3"] * (1. - t) * p8(t.shape)
    s1, s2 = cc(t.shape) / d["Z1"], cc(t.shape) / d["Z2"]
    d["NUB"], d["NU"] = 0.5 * (s1 + s2), 0.5 * (s2 - s1)
    d["S1"], d["S2"] = (d["NUB"] - d["NU"]) * p9(t.shape), (d["NUB"] + d["NU"]) * p9(t.shape)
    s3 = cc() / g["z3"]
    g["n1"] = float(d["NUB"].sum()) + s3
    g["s3"] = float(LD(g["n1"]) - np.asarray(d["NUB"], dtype=LD).sum()) * p9()
    # the scalars
    g["dsg"], g["sigbar"] = rng.uniform(0.2, 0.6), g["sig"] - rng.uniform(-0.3, 0.3)
    g["ss"] = (g["sig"] - 0.001) * p9()
    g["zs"] = cc() / g["ss"]
    sc = np.array([0.5 + 0.5 * g["dsg"], 0.5 - 0.5 * g["dsg"], g["sig"] - g["sigbar"]]) * p9(3)
    zc = cc() * jinv(sc) * np.array([1., 1. - 0.2 * rng.uniform(), 1. - 0.2 * rng.uniform()])
    for i in range(3):
        g["sc3_%d" % i], g["zc3_%d" % i] = float(sc[i]), float(zc[i])
    # the stage variables: inside every application cone; their slacks and duals
    d["S"], d["Z"] = np.zeros((K, NS)), np.zeros((K, NS))
    for k, (G, h) in enumerate(stage_maps(d)):
        d["W"][k] = interior_w(d, k, G, h, d["W"][k], rng.uniform(1e-2, 4e-2))
    P = pr.Problem(d, pr.Num("ld"))
    sa, T0 = P.saff(), P.rz()
    for k in range(K):
        for c in range(1, lay["NCONES"]):
            if d["act"][k] & (1 << c):
                o, dim = lay["coneOff"][c], lay["coneDim"][c]
                d["S"][k, o:o + dim] = [float(sa["st", k, o + i]) + 2e-9 * T0["st", k, o + i][1] * pm() for i in range(dim)]
                d["Z"][k, o:o + dim] = (cc() * jinv(d["S"][k, o:o + dim]) * np.concatenate([[1.], 1. - 0.2 * rng.uniform(size=dim - 1)])).astype(np.float64)
        for l in range(lay["NLP"]):
            if d["act"][k] & (1 << (lay["NCONES"] + l)):
                i = lay["LP0"] + l
                d["S"][k, i] = float(sa["st", k, i]) + 2e-9 * T0["st", k, i][1] * pm()
                d["Z"][k, i] = cc() / d["S"][k, i]
    # the multipliers: lam from the nu columns, w_trt and w_t from the dsg and sigma columns (the cost weights are data)
    absorb = lambda v: float(sum(v)) * p8()
    d["LAM"], it["w_trt"], it["w_t"], it["wtrx"] = np.zeros((K - 1, NL)), 0., 0., 0.
    terms = pr.Problem(d, pr.Num("ld")).rx_terms()
    for k in range(K - 1):
        for i in range(NL):
            d["LAM"][k, i] = absorb(terms["nu", k, i])  # (the row's coefficient on nu is -1)
    it["w_trt"] = -absorb(terms["dsg",])
    terms = pr.Problem(d, pr.Num("ld")).rx_terms()
    it["w_t"] = -absorb(terms["sig",])
    # the trust-region cone: the dual's tail from the w columns, then its slack, which gives delta_k and the centre
    used = [j for j in range(NVU) if not (scvx and j < NXV)]
    tail = np.zeros((K, NV))
    for k in range(K):
        for j in used:
            tail[k, j] = -absorb(terms["w", k, j]) if ("w", k, j) in terms else MU * rng.standard_normal()
    if not scvx:
        it["wtrx"] = 2. * np.sqrt((tail ** 2).sum(axis=1)).max() * rng.uniform(1., 1.5)
    tr = ip[lay["IP_TR"]]
    for k in range(K):
        c_k, tk = cc(), np.asarray(tail[k, used], dtype=LD)
        z0 = LD(it["wtrx"]) * p8() if not scvx else (c_k + np.sqrt(LD(c_k) ** 2 + 4 * LD(tr) ** 2 * (tk * tk).sum())) / (2 * LD(tr))
        s = c_k * jinv(np.concatenate([[z0], tk]))
        d["Z"][k, 0] = float(z0)
        for n_, j in enumerate(used):
            d["Z"][k, 1 + j] = tail[k, j]
            d["WBAR"][k, j] = float(LD(d["W"][k, j]) + s[1 + n_])
        if not scvx:
            d["DL"][k] = float(s[0])
    sa, T0 = (lambda P_: (P_.saff(), P_.rz()))(pr.Problem(d, pr.Num("ld")))
    for k in range(K):
        for i in [0] + [1 + j for j in used]:
            d["S"][k, i] = float(sa["st", k, i]) + 2e-9 * T0["st", k, i][1] * pm()
    # Z of the dynamics from the equality rows
    for (k, i), (v, T, _) in pr.Problem(d, pr.Num("ld")).ry().items():
        d["Zc"][k, i] = float(LD(d["Zc"][k, i]) + v - LD(1e-8 * T * pm()))
    return d

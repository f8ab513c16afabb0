"""Reference for tests/test_cone_math.py: the second-order-cone primitives of csrc/cone_math.h restated in mpmath (256 bits) FROM THEIR
DEFINITIONS -- the header comment of cone_math.h and the ECOS / CVXOPT papers (Domahidi, Chu, Boyd: ECOS, ECC 2013; Vandenberghe: The CVXOPT
linear and quadratic cone program solvers, 2010) -- not from the code: explicit d x d matrices for W, W^-1, W^-2 and the arrow matrix, a linear
solve for the conic division, the roots of a quadratic for the step bound.  Every function takes float64 inputs (exact) and returns mpf values.

Also here: kappa, the amplification factors of the accuracy bars (computed from the inputs only) and the input grid of the tests."""
import mpmath as mp
import numpy as np

mp.mp.prec = 256
U = mp.mpf(2) ** -53


def M(x):
    return [mp.mpf(float(v)) for v in x]


def jdot(x, y):
    """x' J y, J = diag(1, -1, .., -1)"""
    return x[0] * y[0] - sum(a * b for a, b in zip(x[1:], y[1:]))


def kappa(x):
    """(x0^2 + |x1|^2) / (x0^2 - |x1|^2): the condition number of x0^2 - |x1|^2 as a sum"""
    x = M(x)
    n1 = sum(a * a for a in x[1:])
    return (x[0] * x[0] + n1) / (x[0] * x[0] - n1)


# ---------------------------------------------------------------- the primitives, from their definitions
def nt_scaling(s, z):
    """(wbar, eta): sbar = s / |s|_J, zbar = z / |z|_J, gamma = sqrt((1 + sbar'zbar) / 2), wbar = (sbar + J zbar) / (2 gamma), eta = sqrt(|s|_J / |z|_J)"""
    s, z = M(s), M(z)
    sn, zn = mp.sqrt(jdot(s, s)), mp.sqrt(jdot(z, z))
    sbar, zbar = [a / sn for a in s], [a / zn for a in z]
    gamma = mp.sqrt((1 + sum(a * b for a, b in zip(sbar, zbar))) / 2)
    w = [(sbar[0] + zbar[0]) / (2 * gamma)] + [(a - b) / (2 * gamma) for a, b in zip(sbar[1:], zbar[1:])]
    return w, mp.sqrt(sn / zn)


def w_matrix(eta, w, inverse=False):
    """W = eta [w0, w1'; w1, I + w1 w1' / (1 + w0)] as rows of mpf; inverse: W^-1 = (1 / eta) [w0, -w1'; -w1, I + w1 w1' / (1 + w0)].
    (eta, w) are the exact inputs handed to the device: w is not assumed normalised, so W^-1 is the matrix the header defines, which is the inverse
    of W only for w0^2 - |w1|^2 = 1.)"""
    eta, w = mp.mpf(float(eta)), M(w)
    d = len(w)
    sg = -1 if inverse else 1
    rows = [[w[0]] + [sg * a for a in w[1:]]]
    for i in range(1, d):
        rows.append([sg * w[i]] + [(1 if i == j else 0) + w[i] * w[j] / (1 + w[0]) for j in range(1, d)])
    f = 1 / eta if inverse else eta
    return [[f * a for a in r] for r in rows]


def winv2_matrix(eta, w):
    """W^-2 = (2 vt vt' - J) / eta^2, vt = J w"""
    eta, w = mp.mpf(float(eta)), M(w)
    d = len(w)
    vt = [w[0]] + [-a for a in w[1:]]
    return [[(2 * vt[i] * vt[j] - (0 if i != j else (1 if i == 0 else -1))) / (eta * eta) for j in range(d)] for i in range(d)]


def arrow_matrix(u):
    """Arw(u) = [u0, u1'; u1, u0 I]: u o v = Arw(u) v"""
    u = M(u)
    d = len(u)
    rows = [list(u)]
    for i in range(1, d):
        rows.append([u[i]] + [u[0] if i == j else mp.mpf(0) for j in range(1, d)])
    return rows


def matvec(A, v):
    v = M(v)
    return [sum(a * b for a, b in zip(r, v)) for r in A]


def absmatvec(A, v):
    """per component, the sum of the absolute values of the terms"""
    v = M(v)
    return [sum(abs(a * b) for a, b in zip(r, v)) for r in A]


def apply_w(eta, w, v):
    return matvec(w_matrix(eta, w), v)


def apply_winv(eta, w, v):
    return matvec(w_matrix(eta, w, inverse=True), v)


def apply_winv2(eta, w, v):
    return matvec(winv2_matrix(eta, w), v)


def conic_product(u, v):
    return matvec(arrow_matrix(u), v)


def conic_division(lam, dd):
    """x with Arw(lam) x = dd, by Gaussian elimination on the dense d x d system"""
    x = mp.lu_solve(mp.matrix(arrow_matrix(lam)), mp.matrix(M(dd)))
    return [x[i] for i in range(len(lam))]


def step_roots(lam, v):
    """the two roots mu_1 <= mu_2 of (lam'J lam) mu^2 - 2 (lam'J v) mu + v'J v = 0 (real for lam in the interior: reversed Cauchy-Schwarz)"""
    lam, v = M(lam), M(v)
    a, b, c = jdot(lam, lam), jdot(lam, v), jdot(v, v)
    disc = b * b - a * c
    assert a > 0 and disc >= 0
    r = mp.sqrt(disc)
    return (b - r) / a, (b + r) / a


def step_inv(lam, v):
    """-mu_1: its reciprocal is the largest alpha with lam + alpha v in the cone when positive"""
    return -step_roots(lam, v)[0]


# ---------------------------------------------------------------- amplification factors (inputs only)
def amp_w_terms(eta, w, v, inverse=False):
    """terms of the header's W (or W^-1) row by row: eta (w_i v0 + v_i + w_i sum_j w_j v_j / (1 + w0)) has d + 1 terms in row i >= 1"""
    eta, w, v = mp.mpf(float(eta)), M(w), M(v)
    f = 1 / eta if inverse else eta
    zeta = sum(abs(a * b) for a, b in zip(w[1:], v[1:]))
    out = [f * (abs(w[0] * v[0]) + zeta)]
    for i in range(1, len(w)):
        out.append(f * (abs(v[i]) + abs(w[i]) * (abs(v[0]) + zeta / abs(1 + w[0]))))
    return out


def amp_winv2_terms(eta, w, v):
    """terms of (2 vt vt' - J) v / eta^2: 2 vt_i (vt_j v_j) for every j, and v_i"""
    eta, w, v = mp.mpf(float(eta)), M(w), M(v)
    tv = sum(abs(a * b) for a, b in zip(w, v))
    return [(2 * abs(w[i]) * tv + abs(v[i])) / (eta * eta) for i in range(len(w))]


def amp_product_terms(u, v):
    return absmatvec(arrow_matrix(u), v)


def amp_division_terms(lam, dd):
    """terms of x0 = (lam0 d0 - lam1'd1) / rho, x_i = (d_i - x0 lam_i) / lam0, times kappa(lam)"""
    k = kappa(lam)
    lam, dd = M(lam), M(dd)
    rho = jdot(lam, lam)
    a0 = sum(abs(a * b) for a, b in zip(lam, dd)) / rho
    return [k * a0] + [k * (abs(dd[i]) + a0 * abs(lam[i])) / lam[0] for i in range(1, len(lam))]


def amp_step(lam, v):
    m1, m2 = step_roots(lam, v)
    return kappa(lam) * (abs(m1) + abs(m2))


# ---------------------------------------------------------------- inputs
DELTAS = [0.5, 1e-2, 1e-5, 1e-8]


def cone_points(rng, n, d, deltas, zero_rows=0):
    """n points c (1, (1 - delta) u), |u| = 1 (up to rounding: 1 - delta keeps them inside), c = 10^U(-6, 6); rows 1 .. zero_rows of u exactly zero"""
    u = rng.standard_normal((n, d - 1))
    u[:, :zero_rows] = 0.
    u /= np.sqrt((u * u).sum(axis=1, keepdims=True))
    x = np.empty((n, d))
    x[:, 0] = 1.
    x[:, 1:] = (1. - np.asarray(deltas)[:, None]) * u
    return x * 10. ** rng.uniform(-6., 6., size=(n, 1))


def directions(rng, n, d, zero_rows=0):
    """entries +-10^U(-3, 3); rows 1 .. zero_rows exactly zero"""
    v = rng.choice([-1., 1.], size=(n, d)) * 10. ** rng.uniform(-3., 3., size=(n, d))
    v[:, 1:1 + zero_rows] = 0.
    return v


def to_f64(x):
    return np.array([float(a) for a in x])

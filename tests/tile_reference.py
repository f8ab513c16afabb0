"""References for tests/test_tile_engine.py that share nothing with the kernels of scpp_amd/csrc/tile_engine.h and common.h:
mpmath at 50 digits, 80-bit np.longdouble, and a plain float64 "twin" of the elimination that measures what double precision
itself costs on each matrix.  The lane index maps are written from the comments in common.h (what each move is SAID to do)."""
import mpmath
import numpy as np

EPS = float(np.finfo(np.float64).eps)  # 2^-52
FLOOR_REL = 1e-14  # the pivot floor of invCholImpl: max(d, 1e-14 A_jj)
mpmath.mp.dps = 50


# ---------------------------------------------------------------- lane moves: out[l] = in[SRC[l]]
def lane_maps():
    """name -> (op code of the probe, source lane of every lane; -1: the lane receives 0)"""
    l = np.arange(64)
    m = {
        "rowXor1": (0, l ^ 1),  # partner inside the quad
        "rowXor2": (1, l ^ 2),
        "rowHalfMirror": (2, (l // 8) * 8 + 7 - l % 8),  # lane 7 - i of the half row
        "rowMirror": (3, (l // 16) * 16 + 15 - l % 16),  # lane 15 - i of the row of 16 lanes
        "rowRor8": (4, l ^ 8),  # partner lane ^ 8
        "pairHead": (5, (l // 2) * 2),  # the even lane of each pair
        "prevLane": (6, l - 1),  # value of lane - 1, lane 0: 0 (crosses the rows of 16)
        "rowGroupDiag": (7, (l % 16 % 4) * 16 + l % 16),  # lane (g, i) receives lane (i & 3, i)
    }
    for gs in range(4):
        m["rowGroupBcast<%d>" % gs] = (8 + gs, gs * 16 + l % 16)  # lane (g, i) receives lane (GS, i)
    for j in range(16):
        m["rowBcast<%d>" % j] = (16 + j, (l // 16) * 16 + j)  # lane J of every row of 16 lanes to the whole row
    for s in range(64):
        m["readLane(%d)" % s] = (64 + s, np.full(64, s))  # one lane's value for the whole wave
    return m


def apply_map(v, src):
    out = v[np.maximum(src, 0)].copy()
    out[src < 0] = 0
    return out


def row_sum16_replay(v):
    """rowSum16 in float64, in the order of its source: the four butterflies xor 1, xor 2, half mirror, mirror"""
    m = lane_maps()
    v = np.asarray(v, dtype=np.float64).copy()
    for name in ("rowXor1", "rowXor2", "rowHalfMirror", "rowMirror"):
        v = v + v[m[name][1]]
    return v


def wave_sum_dpp_replay(v):
    """waveSumDpp as its comment states it: the row sums, then (r0 + r1) + (r2 + r3)"""
    r = row_sum16_replay(v)
    return (r[0] + r[16]) + (r[32] + r[48])


def mp_sum(v):
    return mpmath.fsum(mpmath.mpf(float(x)) for x in v)


def hi_lo(x):
    """an mpf as an unevaluated sum of two float64 (the correctly rounded value and the remainder)"""
    hi = float(x)
    return hi, float(x - mpmath.mpf(hi))


# ---------------------------------------------------------------- tiles
def v_elem(lane):
    """V layout of a 16-vector: lane l holds x[4 ((l >> 2) & 3) + (l >> 4)]"""
    lane = np.asarray(lane)
    return 4 * ((lane >> 2) & 3) + (lane >> 4)


def ld(a):
    return np.asarray(a, dtype=np.longdouble)


def matmul_ld(a, b):
    return ld(a) @ ld(b)


# ---------------------------------------------------------------- inverse Cholesky factor
def pad(A, n):
    """the padding of the callers in sweeps.h: ones on the diagonal for rows >= n, zeros elsewhere"""
    T = np.eye(16)
    T[:n, :n] = A
    return T


def spd_matrix(rng, n, kappa):
    """Q diag(lambda) Q' with lambda log-spaced in [1 / kappa, 1], scaled by s s' with s_i = 2^k, k uniform in [-20, 20]"""
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(-np.log10(kappa), 0., n) if n > 1 else np.ones(1)
    a = (q * lam) @ q.T
    a = 0.5 * (a + a.T)
    s = np.ldexp(1., rng.integers(-20, 21, n))
    return pad(a * np.outer(s, s), n)  # powers of two: the scaling is exact


def inv_chol_mp(A, n):
    """chol(A[:n, :n])^-1 in mpmath (Cholesky, then its inverse), padded with the identity; as mpmath matrix"""
    L = mpmath.cholesky(mpmath.matrix(A[:n, :n].tolist()))
    Li = mpmath.eye(16)
    inv = mpmath.inverse(L)
    for r in range(n):
        for c in range(n):
            Li[r, c] = inv[r, c] if c <= r else mpmath.mpf(0)
    return Li


def gauss_mp(A, n, floor):
    """Gaussian elimination on [A | I] in mpmath, with or without the floor max(d, 1e-14 A_jj); Li padded with the identity"""
    M = mpmath.matrix(A[:n, :n].tolist())
    R = mpmath.eye(n)
    Li = mpmath.eye(16)
    piv = []
    for j in range(n):
        d = M[j, j]
        if floor:
            d = max(d, mpmath.mpf(FLOOR_REL) * mpmath.mpf(float(A[j, j])))
        piv.append(d)
        for r in range(j + 1, n):
            m = M[r, j] / d
            for c in range(n):
                M[r, c] -= m * M[j, c]
                R[r, c] -= m * R[j, c]
    for r in range(n):
        for c in range(n):
            Li[r, c] = R[r, c] / mpmath.sqrt(piv[r])
    return Li


def mp_to_f64(M):
    return np.array([[float(M[r, c]) for c in range(M.cols)] for r in range(M.rows)])


def twin(A, n, floor):
    """The same elimination in plain numpy float64, in the form the header of tile_engine.h describes it (a reciprocal per pivot, the
    multipliers column x reciprocal, rank-1 updates with row j, rows scaled by 1 / sqrt(pivot)): (Li padded with the identity, raw pivots
    before the floor).  No fused multiply-add, correctly rounded reciprocals: what double precision itself costs on this matrix."""
    with np.errstate(all="ignore"):
        M = np.array(A[:n, :n], dtype=np.float64)
        R = np.eye(n)
        piv = np.zeros(n)
        raw = np.zeros(n)
        for j in range(n):
            d = raw[j] = M[j, j]
            if floor:
                d = max(d, FLOOR_REL * A[j, j])
            piv[j] = d
            p = 1. / d
            for r in range(j + 1, n):
                m = M[r, j] * p
                M[r, :] -= m * M[j, :]
                R[r, :] -= m * R[j, :]
        Li = np.eye(16)
        Li[:n, :n] = np.tril(R * (1. / np.sqrt(piv))[:, None])
    return Li, raw


def residual(Li, A):
    """max |Li A Li' - I| evaluated in longdouble"""
    with np.errstate(all="ignore"):
        return float(np.abs(ld(Li) @ ld(A) @ ld(Li).T - np.eye(16)).max())

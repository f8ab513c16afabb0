"""Reference for tests/test_sweeps.py that shares nothing with the kernels of scpp_amd/csrc/sweeps.h or with oracle/: from the SAME inputs
the sweeps read it assembles the symmetric block-tridiagonal system they claim to solve,

    H_k x_k + M_k' lam_k + N_{k-1}' lam_{k-1}                     = beta_k     k = 0 .. K-1
    M_k x_k + N_k x_{k+1} - (diag(Einv_k) + dual_reg I) lam_k     = rho_k      k = 0 .. K-2

(terms as the comments of sweeps.h and ipm_kernel.h state them), and solves it three ways: mpmath at 50 digits on the dense matrix, a
residual T x - b in 80-bit np.longdouble, and a plain float64 twin of the recursion in the header of tile_engine.h (no fused multiply-add: every
product is an elementwise multiply and a sum) that measures what double precision itself costs on each system.
Only interface constants come from the code (the layout the probe exports: record offsets, the Hessian pattern, the variable maps, fixedMask)."""
import mpmath
import numpy as np

EPS = float(np.finfo(np.float64).eps)  # 2^-52
DUAL_REG = 1e-9  # SCvx mode only (sweeps.h: the static dual regularisation of the multiplier block)
mpmath.mp.dps = 50
NV = 16


def ld(a):
    return np.asarray(a, dtype=np.longdouble)


class System:
    """the inputs of one system, as the sweeps read them: per stage e2, cc, wbt [16], hs [HS_N], einv / S / rho [16] (segment k, NL used),
    beta [16]; per segment A [NX][NX], B, C [NX][NU]; scvx; lay = the probe's layout of the model, fm[k] = fixedMask(k, K)"""

    def __init__(self, model, lay, fm, K, scvx):
        self.model, self.lay, self.fm, self.K, self.scvx = model, lay, list(fm), K, bool(scvx)

    def copy(self):
        s = System(self.model, self.lay, self.fm, self.K, self.scvx)
        for k, v in self.__dict__.items():
            if isinstance(v, np.ndarray):
                setattr(s, k, v.copy())
        return s

    def fixed(self, k):
        return np.array([(self.fm[k] >> j) & 1 for j in range(NV)], dtype=bool)


# ---------------------------------------------------------------- populations
def generate(model, lay, fm, K, scvx, late, rng):
    """A = I + 0.1 G, B = C = 0.1 G (zero-order hold: C = 0); e2 = 10^U(-3, 3); cc |wbt|^2 <= 0.9; Hs symmetric on the pattern, diagonally dominant,
    diagonal >= 0; Einv = 10^u per row, u in [-2, 2] (benign), [-8, 2] (late) and, late SCvx, u = -300 on a third of the rows; beta, rho, S
    standard normal on EVERY entry (fixed and padding variables too)"""
    s = System(model, lay, fm, K, scvx)
    NX, NU, HS_N = lay["NX"], lay["NU"], lay["HS_N"]
    s.A = np.eye(NX)[None] + 0.1 * rng.standard_normal((K - 1, NX, NX))
    s.B = 0.1 * rng.standard_normal((K - 1, NX, NU))
    s.C = 0.1 * rng.standard_normal((K - 1, NX, NU))
    if model == 3:
        s.C[:] = 0.
    s.e2 = 10. ** rng.uniform(-3., 3., K)
    s.wbt = rng.standard_normal((K, NV))
    s.cc = rng.uniform(0.1, 0.9, K) / (s.wbt ** 2).sum(axis=1)
    pat = lay["PAT"]
    s.hs = np.zeros((K, max(HS_N, 1)))
    for k in range(K):
        g = np.where(pat >= 0, rng.standard_normal((NV, NV)), 0.)
        g = np.triu(g, 1)
        g = g + g.T
        g[np.diag_indices(NV)] = np.where(np.diag(pat) >= 0, np.abs(g).sum(axis=1) + rng.uniform(0., 1., NV), 0.)
        g *= 10. ** rng.uniform(-2., 2.)
        assert (g[pat < 0] == 0.).all()
        s.hs[k, pat[pat >= 0]] = g[pat >= 0]
    u = rng.uniform(-8. if late else -2., 2., (K, NV))
    if late and scvx:
        u[rng.uniform(size=(K, NV)) < 1. / 3.] = -300.
    s.einv = 10. ** u
    s.S = rng.standard_normal((K, NV))
    s.beta = rng.standard_normal((K, NV))
    s.rho = rng.standard_normal((K, NV))
    return s


def new_rhs(s, rng):
    t = s.copy()
    t.beta = rng.standard_normal((s.K, NV))
    t.rho = rng.standard_normal((s.K, NV))
    t.S = rng.standard_normal((s.K, NV))
    return t


# ---------------------------------------------------------------- the system
class Blocks:
    pass


def blocks(s):
    """H [K][16][16], M [K-1][NL][16], N [K-1][NL][16], D [K-1][NL] in float64: entries are copies, sign flips or the one product
    e2 (delta - cc w w') + hs, which is formed in longdouble and rounded once"""
    lay, K = s.lay, s.K
    NL, NXV, NVU, pat = lay["NL"], lay["NXV"], lay["NVU"], lay["PAT"]
    b = Blocks()
    b.K, b.NL = K, NL
    b.H = np.zeros((K, NV, NV))
    b.M = np.zeros((K - 1, NL, NV))
    b.N = np.zeros((K - 1, NL, NV))
    b.D = s.einv[: K - 1, :NL] + (DUAL_REG if s.scvx else 0.)
    state = np.arange(NV) < NXV
    for k in range(K):
        w = ld(s.wbt[k])
        h = ld(s.e2[k]) * (np.eye(NV, dtype=np.longdouble) - ld(s.cc[k]) * np.outer(w, w))
        if s.scvx:
            h[state[:, None] | state[None, :]] = 0.
        h[pat >= 0] += ld(s.hs[k, pat[pat >= 0]])
        f = s.fixed(k)
        h[f, :] = 0.
        h[:, f] = 0.
        h[f, f] = 1.
        b.H[k] = h.astype(np.float64)
    for k in range(K - 1):
        f, fn = s.fixed(k), s.fixed(k + 1)
        for j in range(NVU):
            if j < NXV:
                b.M[k, :, j] = -s.A[k, :NL, lay["XMAP"][j]]
                b.N[k, lay["XMAP"][j], j] = 1.
            else:
                b.M[k, :, j] = -s.B[k, :NL, lay["UMAP"][j - NXV]]
                b.N[k, :, j] = -s.C[k, :NL, lay["UMAP"][j - NXV]]
        b.M[k][:, f] = 0.
        b.N[k][:, fn] = 0.
    return b


def rhs(s, border):
    """(beta [K][16], rho [K-1][NL]) of the regular column, or of the sigma border column (beta = 0, rho = -S)"""
    NL = s.lay["NL"]
    if border:
        return np.zeros((s.K, NV)), -s.S[: s.K - 1, :NL]
    return s.beta.copy(), s.rho[: s.K - 1, :NL].copy()


def dense(b):
    """the whole symmetric matrix, unknowns (x_0 .. x_{K-1}, lam_0 .. lam_{K-2}), and the index of the first multiplier"""
    K, NL = b.K, b.NL
    n0 = K * NV
    T = np.zeros((n0 + (K - 1) * NL,) * 2)
    for k in range(K):
        T[k * NV:(k + 1) * NV, k * NV:(k + 1) * NV] = b.H[k]
    for k in range(K - 1):
        r = slice(n0 + k * NL, n0 + (k + 1) * NL)
        T[r, k * NV:(k + 1) * NV] = b.M[k]
        T[r, (k + 1) * NV:(k + 2) * NV] = b.N[k]
        T[r, r] = -np.diag(b.D[k])
    T = np.tril(T) + np.tril(T, -1).T
    return T, n0


def pack(x, lam):
    return np.concatenate([x.ravel(), lam.ravel()])


def unpack(b, v):
    n0 = b.K * NV
    return v[:n0].reshape(b.K, NV), v[n0:].reshape(b.K - 1, b.NL)


def solve_mp(b, columns, lu=False):
    """50-digit solutions of T v = c for every (beta, rho) of `columns`, rounded to float64 at the end.
    The identity rows are taken out first, exactly: such a row reads x_j = beta_j and its column is zero everywhere else.  What remains is
    eliminated without pivoting (L D L') in the order x_0, lam_0, x_1, lam_1, ...: the pivots are then those of the blocks H_k + Z'Z (positive
    definite) and -Theta_k (negative definite), none of them zero; at 50 digits element growth is of no concern, and lu = True solves the
    same system by mpmath's pivoted LU instead (test_reference_agrees_with_itself compares the two)."""
    T, n0 = dense(b)
    n = T.shape[0]
    ident = np.array([T[j, j] == 1. and np.count_nonzero(T[j]) == 1 and np.count_nonzero(T[:, j]) == 1 for j in range(n)])
    order = np.concatenate([np.r_[k * NV:(k + 1) * NV, n0 + k * b.NL:min(n0 + (k + 1) * b.NL, n)] for k in range(b.K)])
    assert sorted(order.tolist()) == list(range(n))
    free = order[~ident[order]]
    m = len(free)
    A = [[mpmath.mpf(float(T[free[i], free[j]])) for j in range(i + 1)] for i in range(m)]  # (lower triangle; T is symmetric)
    if lu:
        full = mpmath.matrix(m, m)
        for i in range(m):
            for j in range(i + 1):
                full[i, j] = full[j, i] = A[i][j]
        LU, perm = mpmath.mp.LU_decomp(full)
    else:
        d = [None] * m
        for j in range(m):  # A[i][j] becomes L[i][j]; the trailing block is updated in its lower triangle only
            d[j] = A[j][j]
            col = [A[i][j] for i in range(j + 1, m)]
            for i in range(j + 1, m):
                l = col[i - j - 1] / d[j]
                Ai = A[i]
                for c in range(j + 1, i + 1):
                    Ai[c] -= l * col[c - j - 1]
                Ai[j] = l
    out = []
    for beta, rho in columns:
        c = pack(beta, rho)
        v = c.copy()
        if lu:
            y = mpmath.mp.U_solve(LU, mpmath.mp.L_solve(LU, mpmath.matrix(c[free].tolist()), perm))
        else:
            y = [mpmath.mpf(float(t)) for t in c[free]]
            for i in range(m):
                y[i] -= mpmath.fsum(A[i][j] * y[j] for j in range(i))
            y = [y[i] / d[i] for i in range(m)]
            for i in range(m - 1, -1, -1):
                y[i] -= mpmath.fsum(A[j][i] * y[j] for j in range(i + 1, m))
        v[free] = [float(t) for t in y]
        out.append(unpack(b, v))
    return out


def residual(b, beta, rho, x, lam):
    """|T v - c| / (|T| |v| + |c|) row by row in longdouble, stage by stage: (rx [K][16], rl [K-1][NL]); 0 / 0 = 0"""
    K = b.K
    H, M, N, D, x, lam, beta, rho = (ld(a) for a in (b.H, b.M, b.N, b.D, x, lam, beta, rho))
    rx, sx = np.zeros((K, NV), dtype=np.longdouble), np.zeros((K, NV), dtype=np.longdouble)
    rl, sl = np.zeros((K - 1, b.NL), dtype=np.longdouble), np.zeros((K - 1, b.NL), dtype=np.longdouble)
    for k in range(K):
        r, a = H[k] @ x[k] - beta[k], np.abs(H[k]) @ np.abs(x[k]) + np.abs(beta[k])
        if k < K - 1:
            r, a = r + M[k].T @ lam[k], a + np.abs(M[k]).T @ np.abs(lam[k])
        if k > 0:
            r, a = r + N[k - 1].T @ lam[k - 1], a + np.abs(N[k - 1]).T @ np.abs(lam[k - 1])
        rx[k], sx[k] = np.abs(r), a
    for k in range(K - 1):
        rl[k] = np.abs(M[k] @ x[k] + N[k] @ x[k + 1] - D[k] * lam[k] - rho[k])
        sl[k] = np.abs(M[k]) @ np.abs(x[k]) + np.abs(N[k]) @ np.abs(x[k + 1]) + np.abs(D[k] * lam[k]) + np.abs(rho[k])
    with np.errstate(all="ignore"):
        qx = np.where(rx == 0, 0, rx / sx).astype(np.float64)
        ql = np.where(rl == 0, 0, rl / sl).astype(np.float64)
    return qx, ql


def worst(qx, ql):
    return max(float(np.nan_to_num(qx, nan=np.inf).max()), float(np.nan_to_num(ql, nan=np.inf).max()))


def first_over(qx, ql, bar):
    """'stage k, row ..' of the first residual over the bar (stage by stage, the variable rows of a stage before its multiplier rows)"""
    for k in range(qx.shape[0]):
        for name, q in (("x", qx[k]), ("lam", ql[k] if k < ql.shape[0] else np.zeros(0))):
            bad = np.flatnonzero(~(q <= bar))
            if bad.size:
                return f"stage {k}, row {name}[{bad[0]}]: {q[bad[0]]:.3e} > {bar:.3e}"
    return None


# ---------------------------------------------------------------- the float64 twin
def mul(a, b):
    """a b in float64 without a fused multiply-add: elementwise products, then a sum"""
    a, b = np.atleast_2d(a), np.asarray(b)
    if b.ndim == 1:
        return (a * b[None, :]).sum(axis=1)
    return (a[:, :, None] * b[None, :, :]).sum(axis=1)


def inv_chol(A):
    """(chol(A)^-1, pivots): Cholesky by columns, then the inverse of the triangular factor by forward substitution"""
    n = A.shape[0]
    L = np.zeros((n, n))
    piv = np.zeros(n)
    with np.errstate(all="ignore"):
        for j in range(n):
            piv[j] = A[j, j] - (L[j, :j] * L[j, :j]).sum()
            L[j, j] = np.sqrt(piv[j])
            L[j + 1:, j] = (A[j + 1:, j] - (L[j + 1:, :j] * L[j, :j][None, :]).sum(axis=1)) / L[j, j]
        X = np.zeros((n, n))
        for i in range(n):
            e = np.zeros(n)
            e[i] = 1.
            X[i] = (e - (L[i, :i, None] * X[:i]).sum(axis=0)) / L[i, i]
    return X, piv


class Twin:
    """the recursion of tile_engine.h's header in float64: factor() once, solve() per right-hand side"""

    def __init__(self, b):
        self.b = b
        K = b.K
        self.Li, self.Yt, self.Ti, self.Z = [None] * K, [None] * K, [None] * K, [None] * K
        self.pivots_ok = True
        for k in range(K):
            Phi = b.H[k] if k == 0 else b.H[k] + mul(self.Z[k - 1].T, self.Z[k - 1])
            self.Li[k], p = inv_chol(Phi)
            self.pivots_ok &= bool((p > 0).all())
            if k == K - 1:
                break
            self.Yt[k] = mul(self.Li[k], b.M[k].T)
            Th = mul(self.Yt[k].T, self.Yt[k]) + np.diag(b.D[k])
            self.Ti[k], p = inv_chol(Th)
            self.pivots_ok &= bool((p > 0).all())
            self.Z[k] = mul(self.Ti[k], b.N[k])

    def solve(self, beta, rho):
        b, K = self.b, self.b.K
        a, c = [None] * K, [None] * K
        g = beta[0]
        for k in range(K):
            a[k] = mul(self.Li[k], g)
            if k == K - 1:
                break
            c[k] = mul(self.Ti[k], rho[k] - mul(self.Yt[k].T, a[k]))
            g = beta[k + 1] + mul(self.Z[k].T, c[k])
        x, lam = np.zeros((K, NV)), np.zeros((K - 1, b.NL))
        x[K - 1] = mul(self.Li[K - 1].T, a[K - 1])
        for k in range(K - 2, -1, -1):
            lam[k] = mul(self.Ti[k].T, mul(self.Z[k], x[k + 1]) - c[k])
            x[k] = mul(self.Li[k].T, a[k] - mul(self.Yt[k], lam[k]))
        return x, lam


def stage_error(x, ref):
    """max_i |x - ref| / max_i |ref| per stage (one number per stage of one output field)"""
    with np.errstate(all="ignore"):
        return np.abs(x - ref).max(axis=1) / np.abs(ref).max(axis=1)

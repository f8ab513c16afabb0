"""numpy twin of the process noise in the LQR tracking loop (TEST INFRASTRUCTURE, never imported by the product):

    philox4x32_10   the Philox4x32-10 block on Python ints
    normals         z[0..nx) of (seed, global flight, plant step): the uniforms and Box-Muller with `math`, as include/scpp_hip_lqr.h states them
    plant_step      fixed-step RKF78 over oracle_lib.flow(...) + d with oracle_lib.rkf78_tableau()
    track, fan      the tracking loop with d drawn after the input is decided: get_input, saturate, the latch and the feedforward term are
                    those of lqr_reference, lqr_saturation_reference, lqr_discrete_reference and lqr_affine_reference

It shares no code with scpp_amd/csrc/."""
import math

import numpy as np

import oracle_lib
from lqr_affine_reference import feedforward_at
from lqr_discrete_reference import segment_and_fraction
from lqr_reference import get_input
from lqr_saturation_reference import margin, saturate

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ten rounds; the key is bumped by the Weyl constants between rounds"""
    c0, c1, c2, c3 = (int(v) & MASK for v in ctr)
    k0, k1 = (int(v) & MASK for v in key)
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
    return c0, c1, c2, c3


def uniform(hi, lo):
    """52 bits -> (m + 0.5) 2^-52, exact, strictly inside (0, 1)"""
    return (float((hi << 20) | (lo >> 12)) + 0.5) * 2.0 ** -52


def normals(seed, g, n, nx):
    """z[0..nx) of global flight g at plant step n: counter (n, j, g lo32, g hi32), key (seed lo32, seed hi32), two normals per block"""
    z = []
    for j in range((nx + 1) // 2):
        c = philox4x32_10((n, j, g & MASK, g >> 32), (seed & MASK, seed >> 32))
        u1, u2 = uniform(c[0], c[1]), uniform(c[2], c[3])
        rho = math.sqrt(-2.0 * math.log(u1))
        phi = 2.0 * math.pi * u2
        z += [rho * math.cos(phi), rho * math.sin(phi)]
    return np.array(z[:nx])


def normals_block(seed, flights, steps, nx):
    """z [len(flights)][len(steps)][nx]"""
    return np.array([[normals(seed, g, n, nx) for n in steps] for g in flights])


_tableau = []


def plant_step(model, par, x, u, d, time_step, substeps):
    """x(t + time_step) of dx/dt = f(x, u) + d, u and d constant: `substeps` RKF78 steps, the 8th-order weights"""
    if not _tableau:
        _tableau.append(oracle_lib.rkf78_tableau())
    _, A, B = _tableau[0]
    S = B.shape[0]
    h = time_step / substeps
    y = np.array(x, dtype=np.float64)
    k = np.zeros((S, y.size))
    for _ in range(substeps):
        for s in range(S):
            k[s] = oracle_lib.flow(model, y + h * (A[s, :s] @ k[:s]), u, par)[0] + d
        y = y + h * (B @ k)
    return y


def track(model, par, X, U, G, t_max, x_start, x_final, w, seed, g, lim=None, hold=False, ff=None, time_step=0.01, substeps=20,
          max_steps=1 << 30):
    """One flight of the disturbed loop, global flight index g.  w None: no noise (d = 0).  hold: the correction is latched per segment
    (lqr_discrete_reference.track_held's rule); ff [K][nu]: the feedforward terms (lqr_affine_reference.track's rule); lim: the clip.
    Returns the flight outputs, n_sat, max_clip, min_margin (inf without limits), and the record of every step: rec_x (after the step),
    rec_u (applied), rec_t."""
    K, nU = X.shape[0], U.shape[0]
    foh = nU == K
    nx = X.shape[1]
    x = np.array(x_start, dtype=np.float64)
    x_final = np.asarray(x_final, dtype=np.float64)
    out = dict(err0=float(np.linalg.norm(x - x_final)), max_dev=0.0, status=0, steps=0, t=0.0, u=np.zeros(U.shape[1]), n_sat=0, max_clip=0.0,
               min_margin=math.inf)
    sd = None if w is None else np.array([math.sqrt(float(v) / time_step) for v in w])
    t, steps = 0.0, 0
    u = np.zeros(U.shape[1])
    latched, du = -1, np.zeros(U.shape[1])
    rx, ru, rt = [], [], []
    while t < t_max:
        if steps >= max_steps:
            out["status"] = 1
            break
        if hold:
            i, a = segment_and_fraction(K, t_max, t)
            j = i + 1 if foh else i
            x_ref = X[i] + a * (X[i + 1] - X[i])
            if i != latched:
                du = -(G[i] @ (x - x_ref))
                latched = i
            ucmd = du + (U[i] + a * (U[j] - U[i]))
        else:
            ucmd, x_ref = get_input(X, U, G, t_max, t, x)
            if ff is not None:
                ucmd = ucmd - feedforward_at(ff, K, nU, t_max, t)
        out["max_dev"] = max(out["max_dev"], float(np.linalg.norm(x - x_ref)))
        if not np.all(np.isfinite(ucmd)):
            out["status"] = -2
            break
        u = ucmd
        if lim is not None:
            u = saturate(model, ucmd, lim)
            out["min_margin"] = min(out["min_margin"], margin(model, ucmd, lim))
            if (u != ucmd).any():
                out["n_sat"] += 1
                out["max_clip"] = max(out["max_clip"], math.sqrt(sum(float(e) * float(e) for e in ucmd - u)))
        d = np.zeros(nx) if sd is None else sd * normals(seed, g, steps, nx)
        xn = plant_step(model, par, x, u, d, time_step, substeps)
        if not np.all(np.isfinite(xn)):
            out["status"] = -2
            break
        x = xn
        t += time_step
        rx.append(x)
        ru.append(np.array(u))
        rt.append(t)
        steps += 1
    out.update(x=x, u=u, t=t, steps=steps, err1=float(np.linalg.norm(x - x_final)), rec_x=np.array(rx).reshape(-1, nx),
               rec_u=np.array(ru).reshape(-1, U.shape[1]), rec_t=np.array(rt))
    return out


def fan(model, par, X, U, G, t, x_start, x_final, w, seed, flight_offset=0, samples=1, lim=None, hold=False, ff=None, time_step=0.01,
        substeps=20, max_steps=1 << 30):
    """F = B samples flights: flight f follows trajectory f // samples with that trajectory's parameter row, limits row and feedforward
    terms, and draws as the global flight flight_offset + f"""
    par = np.asarray(par, dtype=np.float64).reshape(-1, np.shape(par)[-1])
    lim = None if lim is None else np.asarray(lim, dtype=np.float64).reshape(-1, 3)
    x_start = np.asarray(x_start, dtype=np.float64).reshape(X.shape[0] * samples, -1)
    res = []
    for f in range(x_start.shape[0]):
        b = f // samples
        res.append(track(model, par[b if par.shape[0] > 1 else 0], X[b], U[b], G[b], float(t[b]), x_start[f], x_final, w, seed,
                         flight_offset + f, None if lim is None else lim[b if lim.shape[0] > 1 else 0], hold, None if ff is None else ff[b],
                         time_step, substeps, max_steps))
    return res

"""The tangent of the particle-mesh Ewald reciprocal sum in numpy float64: the CPU twin of the mesh tangent stage of csrc/pme.hip
(pme_tspread_kernel ... pme_tgather_kernel), on the mesh conventions of oracle/pme.py (its `bspline`, `bspline_moduli`, index
and transform conventions are imported, not restated).  TEST INFRASTRUCTURE ONLY.

The cell is fixed, the atoms move along v and the charges along t_q:

    primal    Q = sum_i q_i theta_i      pot = G Q       phi_i = sum_m theta_i pot     g_i = sum_m grad theta_i pot
    tangent   tQ = sum_i [t_q_i theta_i + q_i (grad theta_i . v_i)]                     tpot = G tQ
              tphi_i = sum_m theta_i tpot + g_i . v_i
              t_g_i  = sum_m grad theta_i tpot + T_i v_i,    T_i = sum_m grad grad theta_i pot

G (charge mesh -> potential mesh) is linear and depends on the cell alone.  grad grad theta needs the second derivative of the
order-p spline: in the recursion's own terms d2w[j] = w_{p-2}[j-2] - 2 w_{p-2}[j-1] + w_{p-2}[j] from the order p - 2 weights
(the derivative rule dw_p[j] = w_{p-1}[j-1] - w_{p-1}[j] applied twice).  Everything is WITHOUT the neutralising background: it
is a constant of the evaluation (sum t_q = 0)."""
from __future__ import annotations

import math

import numpy as np

from oracle import pme as OP


def bspline_d2(u_frac: np.ndarray, p: int):
    """(w, dw, d2w) [n, p]: oracle.pme.bspline's weights and first derivative, and the second derivative with respect to u."""
    w, dw = OP.bspline(u_frac, p)
    n = u_frac.shape[0]
    if p - 2 >= 2:
        w2, _ = OP.bspline(u_frac, p - 2)  # [n, p - 2]
    else:
        raise ValueError("second derivative needs order >= 4")
    pad = np.zeros((n, p + 2))
    pad[:, 2 : p] = w2                 # pad[:, j + 2] = w2[:, j]
    d2w = np.zeros((n, p))
    for j in range(p):                 # w2[j - 2] - 2 w2[j - 1] + w2[j], out-of-range entries zero
        d2w[:, j] = pad[:, j] - 2.0 * pad[:, j + 1] + pad[:, j + 2]
    return w, dw, d2w


def influence(cell: np.ndarray, alpha: float, mesh, order: int = OP.PME_ORDER) -> np.ndarray:
    """theta(m) of oracle.pme.pme_reciprocal on the full mesh (0 at m = 0)."""
    c = np.asarray(cell, dtype=np.float64)
    K = np.asarray(mesh, dtype=np.int64)
    inv = np.linalg.inv(c)
    vol = abs(np.linalg.det(c))
    mm = [np.where(np.arange(K[a]) <= K[a] // 2, np.arange(K[a]), np.arange(K[a]) - K[a]) for a in range(3)]
    m1, m2, m3 = np.meshgrid(*mm, indexing="ij")
    b = 2.0 * math.pi * inv.T
    kx = m1[..., None] * b[0] + m2[..., None] * b[1] + m3[..., None] * b[2]
    k2 = (kx * kx).sum(-1)
    k2[0, 0, 0] = 1.0
    mod = (OP.bspline_moduli(K[0], order)[:, None, None] * OP.bspline_moduli(K[1], order)[None, :, None] *
           OP.bspline_moduli(K[2], order)[None, None, :])
    theta = 4.0 * math.pi / vol * np.exp(-k2 / (4.0 * alpha * alpha)) / k2 * mod
    theta[0, 0, 0] = 0.0
    return theta


def pme_tangent(x, q, tq, v, cell, alpha: float, mesh, order: int = OP.PME_ORDER):
    """x [n, 3], q [n], tq [K, n], v [K, n, 3] -> dict(phi [n], g [n, 3], T [n, 3, 3], tphi [K, n], tg [K, n, 3]); no background."""
    x, q = np.asarray(x, dtype=np.float64), np.asarray(q, dtype=np.float64)
    tq, v = np.asarray(tq, dtype=np.float64), np.asarray(v, dtype=np.float64)
    c = np.asarray(cell, dtype=np.float64)
    n, nk, p = x.shape[0], v.shape[0], order
    K = np.asarray(mesh, dtype=np.int64)
    Kf = K.astype(np.float64)
    inv = np.linalg.inv(c)
    frac = x @ inv
    frac -= np.floor(frac)
    u = frac * K
    fl = np.floor(u).astype(np.int64)
    w, dw, d2w, idx = [], [], [], []
    for a in range(3):
        wa, dwa, d2wa = bspline_d2(u[:, a] - fl[:, a], p)
        w.append(wa), dw.append(dwa), d2w.append(d2wa)
        idx.append((fl[:, a, None] - (p - 1) + np.arange(p)[None, :]) % K[a])
    theta = influence(c, alpha, mesh, p)
    G = lambda mesh_q: np.fft.ifftn(theta * np.fft.fftn(mesh_q)).real * K.prod()  # noqa: E731
    outer = lambda a0, a1, a2: a0[:, None, None] * a1[None, :, None] * a2[None, None, :]  # noqa: E731
    Q = np.zeros(tuple(K))
    for i in range(n):
        Q[np.ix_(idx[0][i], idx[1][i], idx[2][i])] += q[i] * outer(w[0][i], w[1][i], w[2][i])
    pot = G(Q)
    phi, g, T = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3, 3))
    dot = lambda sub, a0, a1, a2: np.einsum("xyz,x,y,z->", sub, a0, a1, a2)  # noqa: E731

    def grad_u(sub, i):
        return np.array([dot(sub, dw[0][i], w[1][i], w[2][i]), dot(sub, w[0][i], dw[1][i], w[2][i]),
                         dot(sub, w[0][i], w[1][i], dw[2][i])]) * Kf

    for i in range(n):
        sub = pot[np.ix_(idx[0][i], idx[1][i], idx[2][i])]
        phi[i] = dot(sub, w[0][i], w[1][i], w[2][i])
        g[i] = inv @ grad_u(sub, i)    # d frac_a / d x_c = inv[c, a]
        Tu = np.zeros((3, 3))
        Tu[0, 0] = dot(sub, d2w[0][i], w[1][i], w[2][i])
        Tu[1, 1] = dot(sub, w[0][i], d2w[1][i], w[2][i])
        Tu[2, 2] = dot(sub, w[0][i], w[1][i], d2w[2][i])
        Tu[0, 1] = Tu[1, 0] = dot(sub, dw[0][i], dw[1][i], w[2][i])
        Tu[0, 2] = Tu[2, 0] = dot(sub, dw[0][i], w[1][i], dw[2][i])
        Tu[1, 2] = Tu[2, 1] = dot(sub, w[0][i], dw[1][i], dw[2][i])
        T[i] = inv @ (Tu * np.outer(Kf, Kf)) @ inv.T
    tphi, tg = np.zeros((nk, n)), np.zeros((nk, n, 3))
    for k in range(nk):
        du = (v[k] @ inv) * Kf         # velocity of the scaled coordinates [n, 3]
        tQ = np.zeros(tuple(K))
        for i in range(n):
            val = tq[k, i] * outer(w[0][i], w[1][i], w[2][i])
            val += q[i] * (du[i, 0] * outer(dw[0][i], w[1][i], w[2][i]) + du[i, 1] * outer(w[0][i], dw[1][i], w[2][i]) +
                           du[i, 2] * outer(w[0][i], w[1][i], dw[2][i]))
            tQ[np.ix_(idx[0][i], idx[1][i], idx[2][i])] += val
        tpot = G(tQ)
        for i in range(n):
            sub = tpot[np.ix_(idx[0][i], idx[1][i], idx[2][i])]
            tphi[k, i] = dot(sub, w[0][i], w[1][i], w[2][i]) + g[i] @ v[k, i]
            tg[k, i] = inv @ grad_u(sub, i) + T[i] @ v[k, i]
    return {"phi": phi, "g": g, "T": T, "tphi": tphi, "tg": tg}


def richardson(f, h: float):
    """d f(t) / dt at 0 from central differences at h and h / 2, extrapolated (error ~ h^4 f^(5)); returns (value, |D(h/2) - D(h)|)."""
    d1 = (f(h) - f(-h)) / (2.0 * h)
    d2 = (f(0.5 * h) - f(-0.5 * h)) / h
    return (4.0 * d2 - d1) / 3.0, np.abs(d2 - d1).max()

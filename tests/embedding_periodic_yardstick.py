"""fp64 yardstick of the periodic embedding (csrc/embed.hip, aimnet_engine_set_embedding_periodic): the Ewald potential of a
lattice of point-charge sites at the atoms, and of the atoms' charges at the sites, in numpy.  Per system, V the cell volume:

    phi_i / k_e =  sum_A sum_n Q_A erfc(alpha d) / d ,  d = |x_i - X_A + n C| < rc
                +  sum_{k in half space, |k| <= kc} A(k) Re[conj(S_ext(k)) e^{i k x_i}] ,  A = (8 pi / V) e^{-k^2 / 4 alpha^2} / k^2
                -  pi Q_ext / (V alpha^2)

No self term, no site-site term.  `erfc` comes from torch (no scipy).  Also an fp32 restatement of one real-space term and one k
term in the kernel's own formulas (the erfc polynomial of csrc/common.h included): the GPU test takes its rounding allowances from
the distance between that restatement and fp64 over its own inputs."""
from __future__ import annotations

import math

import numpy as np
import torch

KE = 27.211386024367243 * 0.5291772105638411  # Hartree * Bohr, eV A / e^2 (csrc/embed.hip)
U = 2.0**-24  # one fp32 rounding


def _erfc(x):
    return torch.erfc(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def params(cell, n_eff: int, accuracy: float):
    """(alpha, rc, kc) of the engine's Ewald rule: eta = (V^2 / n_eff)^(1/6) / sqrt(2 pi), alpha = 1 / (sqrt(2) eta), rc = f eta,
    kc = f / eta, f = sqrt(-2 ln accuracy)."""
    vol = abs(np.linalg.det(np.asarray(cell, np.float64)))
    eta = (vol * vol / max(int(n_eff), 1)) ** (1.0 / 6.0) / math.sqrt(2.0 * math.pi)
    f = math.sqrt(-2.0 * math.log(accuracy))
    return 1.0 / (math.sqrt(2.0) * eta), f * eta, f / eta


def params32(cell, n_eff: int, accuracy: float):
    """`params` as the kernels hold them: alpha, rc and kc^2 rounded to fp32 (EwaldSystem, csrc/kernels.h)."""
    al, rc, kc = params(np.asarray(cell, np.float32), n_eff, accuracy)
    return float(np.float32(al)), float(np.float32(rc)), math.sqrt(float(np.float32(kc * kc)))


def images(cell, rc: float):
    """Translations |n_a| <= m_a = floor(rc / h_a + 1/2), h_a the perpendicular widths: with the fractional difference of a pair
    reduced to [-1/2, 1/2]^3 they reach every image inside rc."""
    inv = np.linalg.inv(np.asarray(cell, np.float64))
    h = 1.0 / np.linalg.norm(inv, axis=0)
    return [int(math.floor(rc / ha + 0.5)) for ha in h]


def kvectors(cell, kc: float):
    """Integer triplets of the half space with |k| <= kc and their k vectors (rows)."""
    c = np.asarray(cell, np.float64)
    b = 2.0 * math.pi * np.linalg.inv(c).T  # rows: reciprocal vectors
    nmax = [int(math.floor(kc * np.linalg.norm(c[a]) / (2.0 * math.pi))) for a in range(3)]
    n = np.stack(np.meshgrid(np.arange(0, nmax[0] + 1), np.arange(-nmax[1], nmax[1] + 1), np.arange(-nmax[2], nmax[2] + 1),
                             indexing="ij"), -1).reshape(-1, 3)
    half = (n[:, 0] > 0) | ((n[:, 0] == 0) & ((n[:, 1] > 0) | ((n[:, 1] == 0) & (n[:, 2] > 0))))
    n = n[half]
    k = n @ b
    keep = (k * k).sum(-1) <= kc * kc
    return n[keep], k[keep]


def pair_vectors(x, X, cell, rc: float):
    """Every pair vector r = x_i - X_A + n C with |r| < rc: (i, A, r) - minimal image in fractional coordinates, then translations."""
    c = np.asarray(cell, np.float64)
    inv = np.linalg.inv(c)
    df = (np.asarray(x, np.float64) @ inv)[:, None, :] - (np.asarray(X, np.float64) @ inv)[None, :, :]
    df -= np.rint(df)
    base = df @ c
    m = images(c, rc)
    I, A, R = [], [], []
    for n0 in range(-m[0], m[0] + 1):
        for n1 in range(-m[1], m[1] + 1):
            for n2 in range(-m[2], m[2] + 1):
                r = base + np.array([n0, n1, n2], np.float64) @ c
                hit = (r * r).sum(-1) < rc * rc
                i, a = np.nonzero(hit)
                I.append(i), A.append(a), R.append(r[hit])
    return np.concatenate(I), np.concatenate(A), np.concatenate(R)


def field(x, X, Q, cell, alpha: float, rc: float, kc: float, ke: float = KE, q_total: float | None = None):
    """phi [N], g = grad phi [N, 3] of the site lattice (X, Q) at the points x, times `ke`; and the absolute sums of the terms, for
    the rounding gates, as a dict: `phi_real`, `phi_k` [N] and `g_real`, `g_k` [N] (per term the largest component bound: |t| |r|
    resp. A |S| |k|), times `ke` as well.  `q_total`: the charge the background neutralises (default: sum Q)."""
    x, X, Q, c = (np.asarray(v, np.float64) for v in (x, X, Q, cell))
    n = len(x)
    vol = abs(np.linalg.det(c))
    i, a, r = pair_vectors(x, X, c, rc)
    d = np.sqrt((r * r).sum(-1))
    ec = _erfc(alpha * d)
    p = Q[a] * ec / d
    t = Q[a] * (ec / d + 2.0 * alpha / math.sqrt(math.pi) * np.exp(-alpha * alpha * d * d)) / (d * d)
    phi = np.bincount(i, weights=p, minlength=n)
    g = -np.stack([np.bincount(i, weights=t * r[:, k], minlength=n) for k in range(3)], -1)
    abs_sums = {"phi_real": np.bincount(i, weights=np.abs(p), minlength=n), "g_real": np.bincount(i, weights=np.abs(t) * d, minlength=n)}
    _, k = kvectors(c, kc)
    k2 = (k * k).sum(-1)
    amp = 8.0 * math.pi / vol * np.exp(-k2 / (4.0 * alpha * alpha)) / k2
    S = (Q[None, :] * np.exp(1j * (k @ X.T))).sum(-1)  # [nk]
    ph = np.exp(1j * (x @ k.T))  # [N, nk]
    w = amp * np.conj(S)
    phi = phi + (w[None, :] * ph).real.sum(-1)
    g = g + ((1j * w[None, :] * ph).real[:, :, None] * k[None, :, :]).sum(1)
    abs_sums["phi_k"] = np.full(n, (amp * np.abs(S)).sum())
    abs_sums["g_k"] = np.full(n, (amp * np.abs(S) * np.sqrt(k2)).sum())
    phi = phi - math.pi * (Q.sum() if q_total is None else q_total) / (vol * alpha * alpha)
    return ke * phi, ke * g, {key: ke * v for key, v in abs_sums.items()}


def site_terms(x, q, X, Q, cell, alpha: float, rc: float, kc: float, ke: float = KE, q_total: float | None = None):
    """psi [M], the potential of the atoms' charges q (their images and background included) at the sites, the forces on the sites
    -Q grad psi [M, 3], and the absolute sums of `field` with the atoms and the sites exchanged (the force's times |Q|).  `q_total`:
    the system's charge as the caller states it - the engine's background neutralises that, not the sum of its fp32 charges,
    which misses it by their rounding (default: sum q)."""
    psi, grad, abs_sums = field(X, x, q, cell, alpha, rc, kc, ke, q_total)
    Q = np.asarray(Q, np.float64)
    abs_sums = dict(abs_sums, g_real=np.abs(Q) * abs_sums["g_real"], g_k=np.abs(Q) * abs_sums["g_k"])
    return psi, -Q[:, None] * grad, abs_sums


def sites(coord, cell, M: int, seed: int, dmin: float = 1.6):
    """M sites by rejection sampling in fractional coordinates: every site at least `dmin` from every atom image; charges
    uniform(-0.8, 0.8), with whatever net charge that draws (the background is to be exercised).  Returns (X, Q, draws)."""
    rng = np.random.default_rng(seed)
    c = np.asarray(cell, np.float64)
    inv = np.linalg.inv(c)
    fa = np.asarray(coord, np.float64) @ inv
    shifts = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    assert all(m <= 1 for m in images(c, dmin))  # 27 images of the minimal-image vector reach dmin
    out, draws = [], 0
    while len(out) < M:
        f = rng.uniform(0.0, 1.0, 3)
        draws += 1
        df = fa - f
        df -= np.rint(df)
        r = (df[:, None, :] + shifts[None, :, :]) @ c
        if ((r * r).sum(-1) >= dmin * dmin).all():
            out.append(f @ c)
    return np.asarray(out), rng.uniform(-0.8, 0.8, M), draws


# ---- the kernel's fp32 pair term and k term, restated in numpy float32 ----------------------------------------------------------
_ERFC_P = [2.672036890e-02, -2.020067459e-01, 6.150174393e-01, -9.195323909e-01, 6.300562657e-01, -2.111610618e-01, 2.648643249e-01,
           2.301390953e-01, 2.838921720e-01, 2.820105286e-01]  # csrc/common.h, erfc_walk


def real_term32(r, Q, alpha: float):
    """(Q erfc(alpha d) / d, -Q t r) of pair vectors r [n, 3] in float32 arithmetic, the formulas of embed_pbc_pair: reciprocal
    root, d = d2 / root, exp2, t = 1 / (1 + alpha d / 2), the degree-9 Horner form."""
    f = np.float32
    r = np.asarray(r, np.float64).astype(f)
    Q, al = np.asarray(Q, np.float64).astype(f), f(alpha)
    d2 = r[:, 2] * r[:, 2] + (r[:, 1] * r[:, 1] + r[:, 0] * r[:, 0])
    inv = (f(1.0) / np.sqrt(d2)).astype(f)
    d = d2 * inv
    ex = np.exp2(f(-1.4426950408889634) * al * al * d2).astype(f)
    tt = (f(1.0) / (f(0.5) * al * d + f(1.0))).astype(f)
    pe = np.full_like(d, f(_ERFC_P[0]))
    for coef in _ERFC_P[1:]:
        pe = pe * tt + f(coef)
    p = pe * tt * ex * inv
    t = (f(1.1283791670955126) * al * ex + p) * inv * inv * Q
    return (Q * p).astype(np.float64), -(t[:, None] * r).astype(np.float64)


def real_term64(r, Q, alpha: float):
    r, Q = np.asarray(r, np.float64), np.asarray(Q, np.float64)
    d = np.sqrt((r * r).sum(-1))
    ec = _erfc(alpha * d)
    t = Q * (ec / d + 2.0 * alpha / math.sqrt(math.pi) * np.exp(-alpha * alpha * d * d)) / (d * d)
    return Q * ec / d, -t[:, None] * r


def k_term32(frac, n, P, Qk):
    """cs P + sn Q and cs Q - sn P of points `frac` [m, 3] (fractional, double) and entries (n [nk, 3], P, Q [nk]): the phase in
    turns reduced in double, sin / cos of the float32 angle in float32, the products in double (embed_pbc_recip_kernel)."""
    ph = np.asarray(frac, np.float64) @ np.asarray(n, np.float64).T
    ph -= np.rint(ph)
    ang = (6.283185307179586 * ph).astype(np.float32)
    sn, cs = np.sin(ang).astype(np.float64), np.cos(ang).astype(np.float64)
    return cs * P + sn * Qk, cs * Qk - sn * P


def k_term64(frac, n, P, Qk):
    ph = 2.0 * math.pi * (np.asarray(frac, np.float64) @ np.asarray(n, np.float64).T)
    sn, cs = np.sin(ph), np.cos(ph)
    return cs * P + sn * Qk, cs * Qk - sn * P


def rounding_allowances(x, X, Q, cell, alpha: float, rc: float, kc: float):
    """(c_real, c_k): twice the largest deviation, in fp32 roundings, of the restated fp32 terms from fp64 over the pairs and the
    (atom, k) phases of these inputs - a real-space term against its own size, a k term against its amplitude A |S| (what the
    absolute sums of `field` add up) - and not below the 8 roundings of a bare 1 / d term (tests/test_gpu_embedding.py)."""
    x, X, Q, c = (np.asarray(v, np.float64) for v in (x, X, Q, cell))
    _, a, r = pair_vectors(x, X, c, rc)
    p32, v32 = real_term32(r, Q[a], alpha)
    p64, v64 = real_term64(r, Q[a], alpha)
    dev = max(float((np.abs(p32 - p64) / np.abs(p64)).max()), float((np.abs(v32 - v64).max(-1) / np.sqrt((v64 * v64).sum(-1))).max()))
    c_real = max(8.0, 2.0 * dev / U)
    n, k = kvectors(c, kc)
    S = (Q[None, :] * np.exp(1j * (k @ X.T))).sum(-1)
    frac = x @ np.linalg.inv(c)
    t32, d32 = k_term32(frac, n, S.real, S.imag)
    t64, d64 = k_term64(frac, n, S.real, S.imag)
    amp = np.abs(S)[None, :]
    dev = max(float((np.abs(t32 - t64) / amp).max()), float((np.abs(d32 - d64) / amp).max()))
    return c_real, max(8.0, 2.0 * dev / U)

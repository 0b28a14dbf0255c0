"""NumPy references for decomp_amd.template_matching.basis_pursuit on multichannel templates D [T, Ch, S]
(dcp_tm_mc_lasso_*, decomp_amd/csrc/template_mc_lasso.hpp) and the problems its tests share.  Test infrastructure only.

The oracle is oracle.lasso.solve_fastpath on the dense operator A [T C, Ch N] (tm_multichannel_ref.dense_operator) with
y.reshape(B, Ch N), in double.  ``gram_form`` states the iteration the library runs, in NumPy: the gradient from
alpha0 = y A^H and the banded Gram matrix, whose entry for the atoms (t', c'), (t, c) is the lag correlation
Corr[t', t, s (c' - c)] when either atom lies inside the signal, an explicit sum over the overlap inside [0, N) when
neither does, and zero beyond dh = (S - 1) // s.
"""
import functools
import os

import numpy as np

import tm_multichannel_ref as mc
from oracle import lasso as olasso
from oracle.common import gershgorin, real_dtype
from tm_pursuit_ref import _windows

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tm_basis_pursuit_golden.npz')

# name -> (B, T, Ch, S, N, stride, padding): the smallest shapes at which each piece of the step kernel can go wrong
GEOMS = {
    'tile_s1_same': (3, 3, 3, 5, 40, 1, 'SAME'),
    'tile_s2_same': (3, 3, 3, 5, 40, 2, 'SAME'),
    'tile_s3_same': (3, 3, 3, 5, 40, 3, 'SAME'),
    'tile_s1_valid': (3, 3, 3, 5, 40, 1, 'VALID'),
    'tile_s2_valid': (3, 3, 3, 5, 40, 2, 'VALID'),
    'tile_s3_valid': (3, 3, 3, 5, 40, 3, 'VALID'),
    'tiles_same': (2, 3, 3, 33, 300, 1, 'SAME'),         # two tiles of c, the halo crosses their boundary
    'tiles_valid': (2, 3, 3, 33, 300, 3, 'VALID'),       # dh = 10 at stride 3 (C = 90)
    'tiles_valid_s1': (2, 3, 3, 33, 300, 1, 'VALID'),    # C = 268: two tiles and no edge table
    'templates': (2, 9, 2, 5, 40, 1, 'SAME'),            # more templates than a block, ragged last block
    'channels': (2, 2, 9, 5, 40, 2, 'SAME'),             # more channels than a pass of the correlation kernel
    'diagonal': (3, 3, 3, 3, 40, 4, 'SAME'),             # dh = 0
    'none_inside': (3, 3, 3, 5, 6, 3, 'SAME'),           # every atom reaches outside the signal
    'one_channel': (3, 3, 1, 5, 40, 2, 'SAME'),
    # 2 dh + 1 = 5899 taps: with 8-byte elements and wider the tile's window of the iterate exceeds the LDS budget and
    # the step reads it from global memory
    'no_lds': (1, 2, 2, 2950, 3000, 1, 'VALID'),
}

METHODS = ('ista', 'acc_ista', 'fista')


@functools.lru_cache(maxsize=None)
def problem(name, cplx, seed=0):
    """(y [B, Ch, N], D [T, Ch, S], x0 [B, T, C], alpha) in double with single-exact entries: planted events plus
    noise, a non-zero start, and an alpha that leaves a share of the coefficients at zero."""
    B, T, Ch, S, N, stride, padding = GEOMS[name]
    return make_problem(1000 * seed + sorted(GEOMS).index(name), B, T, Ch, S, N, stride, padding, cplx)


def make_problem(seed, B, T, Ch, S, N, stride, padding, cplx):
    rng = np.random.RandomState(seed)

    def randn(*shape):
        v = rng.randn(*shape)
        return v + 1j * rng.randn(*shape) if cplx else v
    D = randn(T, Ch, S) * (0.5 + rng.rand(T, 1, 1))
    C, _, _ = _windows(S, N, stride, padding)
    xt = randn(B, T, C) * (rng.uniform(size=(B, T, C)) < 0.15)
    y = mc.predict(xt, D.astype(xt.dtype), N, stride, padding) + 0.1 * randn(B, Ch, N)
    x0 = 0.3 * randn(B, T, C) * (rng.uniform(size=(B, T, C)) < 0.5)
    single = np.complex64 if cplx else np.float32
    y, D, x0 = (np.ascontiguousarray(a.astype(single).astype(a.dtype)) for a in (y, D, x0))
    A = mc.dense_operator(D, N, stride, padding)
    rho = np.linalg.norm(A, axis=1)
    g = np.abs(y.reshape(B, -1) @ A.conj().T) / rho
    alpha = float(np.float32(0.3 * np.max(g) * np.median(rho) / (Ch * N)))
    for a in (y, D, x0):
        a.setflags(write=False)
    return y, D, x0, alpha


@functools.lru_cache(maxsize=None)
def operator(name, cplx, seed=0):
    _, _, Ch, S, N, stride, padding = GEOMS[name]
    A = mc.dense_operator(problem(name, cplx, seed)[1], N, stride, padding)
    A.setflags(write=False)
    return A


def oracle(y, D, alpha, x0, tol, maxiter, method, stride, padding, trace=None, A=None):
    """(it, x [B, T, C]) of oracle.lasso.solve_fastpath on the dense operator, in double."""
    B, Ch, N = y.shape
    if A is None:
        A = mc.dense_operator(D, N, stride, padding)
    dt = np.complex128 if np.iscomplexobj(A) else np.float64
    it, x = olasso.solve_fastpath(y.reshape(B, -1).astype(dt), A.astype(dt), alpha, x0.reshape(B, -1).astype(dt), tol,
                                  maxiter, method, trace=trace)
    return it, x.reshape(x0.shape)


@functools.lru_cache(maxsize=None)
def oracle_case(name, cplx, method, maxiter, seed=0):
    """The oracle on a shared problem with tol = 0, computed once."""
    y, D, x0, alpha = problem(name, cplx, seed)
    _, _, _, _, _, stride, padding = GEOMS[name]
    it, x = oracle(y, D, alpha, x0, 0.0, maxiter, method, stride, padding, A=operator(name, cplx, seed))
    x.setflags(write=False)
    return it, x


def rel_err(x, ref):
    """The relative max-norm error."""
    return float(np.max(np.abs(np.asarray(x) - ref)) / np.max(np.abs(ref)))


# ---- the Gram-form iteration ----------------------------------------------------------------------------------------
def lag_correlations(D):
    """Corr[t, t', m + S - 1] = sum_ch sum_k D[t, ch, k] conj(D[t', ch, k + m]), |m| < S."""
    T, Ch, S = D.shape
    corr = np.zeros((T, T, 2 * S - 1), dtype=D.dtype)
    for m in range(-(S - 1), S):
        k0, k1 = max(0, -m), min(S - 1, S - 1 - m)
        corr[:, :, m + S - 1] = np.einsum('tck,uck->tu', D[:, :, k0:k1 + 1], np.conj(D[:, :, k0 + m:k1 + m + 1]))
    return corr


def banded_gram(D, N, stride, padding):
    """G [T C, T C], G[(t', c'), (t, c)] = A_(t',c') . A_(t,c)^H by the rule of the step kernel, and the mask of the
    atoms that lie inside the signal."""
    T, Ch, S = D.shape
    C, base, valid = _windows(S, N, stride, padding)
    inside = valid.all(axis=1)
    dh = (S - 1) // stride
    corr = lag_correlations(D)
    G = np.zeros((T, C, T, C), dtype=D.dtype)
    for c in range(C):
        for cp in range(max(0, c - dh), min(C - 1, c + dh) + 1):
            m = stride * (cp - c)
            if inside[c] or inside[cp]:
                G[:, cp, :, c] = corr[:, :, m + S - 1]
                continue
            # the samples n of both atoms inside [0, N): n = base[cp] + k = base[c] + k + m
            k = np.arange(max(0, -m), min(S - 1, S - 1 - m) + 1)
            k = k[(base[cp] + k >= 0) & (base[cp] + k < N)]
            G[:, cp, :, c] = np.einsum('tck,uck->tu', D[:, :, k], np.conj(D[:, :, k + m]))
    return G.reshape(T * C, T * C), inside


def gram_form(y, D, alpha, x0, tol, maxiter, method, stride, padding):
    """(it, x [B, T, C]): the proximal-gradient iteration in Gram form, in the scaled variables x' = x rho."""
    positive = method.endswith('_pos')
    momentum = method[:-4] if positive else method
    B, Ch, N = y.shape
    T, _, S = D.shape
    dt = np.complex128 if np.iscomplexobj(D) else np.float64
    y, D, x0 = y.astype(dt), D.astype(dt), x0.astype(dt)
    C, _, valid = _windows(S, N, stride, padding)
    rho = np.sqrt(mc.rho2_of(D, valid)).reshape(-1)
    G, _ = banded_gram(D, N, stride, padding)
    Gs = G / rho[:, None] / rho[None, :]
    alpha0 = mc.correlate(y, D, N, stride, padding).reshape(B, -1) / rho
    thr_k = alpha * (Ch * N) / rho
    tol_k = tol * rho
    L_inv = 1.0 / gershgorin(Gs)
    shrink = olasso.shrink_positive if positive else (olasso.shrink_complex if dt == np.complex128 else
                                                      olasso.shrink_real)
    rdt = real_dtype(dt)

    def step(v):
        return shrink(v + L_inv * (alpha0 - v @ Gs), L_inv * thr_k)

    x_prev = x_new = v = x0.reshape(B, -1) * rho
    beta = 1.0
    for i in range(maxiter):
        if momentum == 'acc_ista':
            x_prev = x_new
        x_new = step(v)
        if momentum == 'acc_ista':
            v = x_new + rdt.type(i / (i + 3)) * (x_new - x_prev)
        if i % 10 == 0 and np.max(np.abs(x_new - x_prev) - tol_k) < 0.0:
            return i, (x_new / rho).reshape(x0.shape)
        if momentum == 'ista':
            x_prev = v = x_new
        elif momentum == 'fista':
            beta_new = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * beta * beta))
            v = x_new + rdt.type((beta - 1.0) / beta_new) * (x_new - x_prev)
            x_prev, beta = x_new, beta_new
    return maxiter - 1, (x_prev / rho).reshape(x0.shape)


# ---- the stop bookkeeping problem -----------------------------------------------------------------------------------
STOP_SHAPE = (3, 2, 3, 7, 48, 2, 'VALID')          # B, T, Ch, S, N, stride, padding
STOP_ALPHA = 0.007                                 # 0.02 / Ch: the threshold alpha Ch N of the one-channel test
STOP_MAXITER = (1, 2, 10, 11, 12, 21, 31)
STOP_TOL = (0.0, 3e-3, 1e3)
# the seed of each method's problem: every stop statistic of the oracle's trace is at least 1 % away from tol for every
# maxiter and tol above (test_tm_basis_pursuit_host.py checks that on the CPU)
STOP_SEED = {'ista': 6, 'acc_ista': 6, 'fista': 6}


@functools.lru_cache(maxsize=None)
def stop_problem(method):
    B, T, Ch, S, N, stride, padding = STOP_SHAPE
    rng = np.random.RandomState(STOP_SEED[method])
    C, _, _ = _windows(S, N, stride, padding)
    D = rng.randn(T, Ch, S)
    D /= np.linalg.norm(D.reshape(T, -1), axis=1)[:, None, None]
    xt = rng.randn(B, T, C) * (rng.uniform(size=(B, T, C)) < 0.1)
    y = mc.predict(xt, D, N, stride, padding) + 0.05 * rng.randn(B, Ch, N)
    A = mc.dense_operator(D, N, stride, padding)
    for a in (y, D, A):
        a.setflags(write=False)
    return y, D, A, C


def stop_margin_ok(stats, tol):
    """Every stop statistic max(|dx'| - tol rho) is at least 1 % of tol away from zero."""
    return all(abs(v) >= 0.01 * tol for v in stats)


# ---- golden vectors ---------------------------------------------------------------------------------------------------
# (name, dtype, method, stride, padding, maxiter, tol): outputs of the reference's own lasso.solve on the dense operator
GOLDEN_CASES = [
    ('a', 'float32', 'ista', 1, 'SAME', 4, 0.0),
    ('b', 'float64', 'acc_ista', 2, 'VALID', 12, 1e-3),
    ('c', 'complex64', 'fista', 2, 'SAME', 4, 0.0),
    ('d', 'complex128', 'acc_ista', 1, 'VALID', 5, 0.0),
    ('e', 'float64', 'fista_pos', 1, 'SAME', 5, 0.0),
    ('f', 'float32', 'acc_ista_pos', 2, 'SAME', 4, 0.0),
    ('g', 'complex128', 'ista', 2, 'SAME', 11, 1e-3),
]
GOLDEN_SHAPE = (2, 2, 3, 4, 14)                    # B, T, Ch, S, N


def golden_inputs(seed, dtype, stride, padding):
    """(y [B, Ch, N], D [T, Ch, S], x0 [B, T, C], alpha) of a golden case, in its dtype."""
    B, T, Ch, S, N = GOLDEN_SHAPE
    y, D, x0, alpha = make_problem(7000 + seed, B, T, Ch, S, N, stride, padding, np.dtype(dtype).kind == 'c')
    return y.astype(dtype), D.astype(dtype), x0.astype(dtype), alpha

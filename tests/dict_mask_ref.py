"""Float64 / complex128 NumPy restatement of ONE masked dictionary step's statistics and atom update, with the
elementwise magnitude bounds its rounding errors are measured against (test infrastructure only).

The step (reference dictionary_learning.py:205-225, restated as written in oracle/dictionary_learning.py:98-103):
  A3[k, f, j] = beta A3_old[k, f, j] + sum_n conj(x_nk) x_nj m_nf                           (:209-213)
  B[k, f]     = beta B_old[k, f]     + sum_n conj(x_nk) (y o m)_nf                          (:214)
  u_k         = (B_k - sum_j A3[k, :, j] D[j, :]) / sum_f (A3[k, f, k] + 1e-15) + D_k       (:218-222)
  D_new[k]    = u_k / sqrt(max(|u_k|^2, 1))                                                 (:223)
QUIRK: the contraction uses the OLD dictionary for every atom, so the atoms are independent.

The pair statistic is formed here as one matrix product, [K K, Nb] . [Nb, F], instead of the reference's broadcast
[Nb, K, F, K] tensor; test_dict_mask_ref_host.py pins every function to oracle.dictionary_learning.

Every function casts its inputs up (float32 -> float64, complex64 -> complex128) and works there: handed what a
single-precision stage read, it returns what that stage would have written without rounding.

Bounds (`u` = unit roundoff of the real type, eps / 2):
  bound_A[k, f, j] = |beta| |A3_old| + sum_n |x_nk| |x_nj| m_nf     a sequential sum of Nb terms and one scale-and-add
                                                                    is off by at most (Nb + 4) u bound_A
  bound_B[k, f]    = |beta| |B_old| + sum_n |x_nk| |(y o m)_nf|     the scale the GEMM tests use (gpu_util.gemm_bound)
  S[k, f]          = (|B_kf| + sum_j |A3_kfj| |D_jf|) / |A_kk| + |D_kf|
                     D_new is off by at most c_D u (S_kf + |u_kf|) / nrm_k: S carries the contraction, the
                     division and the add, |u_kf| the norm's relative error.
"""
import numpy as np

from oracle.common import JITTER, l2_strict

SUFFIX = {'float32': 'f32', 'float64': 'f64', 'complex64': 'c64', 'complex128': 'c128'}


def up(a):
    """The array in float64 / complex128."""
    a = np.asarray(a)
    return a.astype(np.complex128 if a.dtype.kind == 'c' else np.float64)


def unit_roundoff(dt):
    """u of dt's real type: 2^-24 (float32, complex64) or 2^-53."""
    return 0.5 * float(np.finfo(np.dtype(dt)).eps)


def is_single(dt):
    return np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64))


def _pairs(a, b, m):
    """out[k, f, j] = sum_n a_nk b_nj m_nf."""
    Nb, K = a.shape
    P = (a[:, :, None] * b[:, None, :]).reshape(Nb, K * K)
    return np.ascontiguousarray(P.T.dot(m).reshape(K, K, m.shape[1]).transpose(0, 2, 1))


def stats(x, y, m, A3_old, B_old, beta):
    """-> A3, B of the step whose LASSO returned x."""
    x, y, m, A3_old, B_old = up(x), up(y), up(m), up(A3_old), up(B_old)
    A3 = beta * A3_old + _pairs(np.conj(x), x, m)
    B = beta * B_old + np.conj(x.T).dot(y * m)
    return A3, B


def stats_bounds(x, y, m, A3_old, B_old, beta):
    """-> bound_A, bound_B (real, >= 0)."""
    ax, m = np.abs(up(x)), up(m)
    bound_A = abs(beta) * np.abs(up(A3_old)) + _pairs(ax, ax, m)
    bound_B = abs(beta) * np.abs(up(B_old)) + ax.T.dot(np.abs(up(y)) * m)
    return bound_A, bound_B


def atom_update(D, A3, B):
    """-> D_new, u (before the normalisation), nrm [K], S (the magnitude bound of u's terms)."""
    D, A3, B = up(D), up(A3), up(B)
    K = D.shape[0]
    AkD = np.einsum('kfj,jf->kf', A3, D)
    Akk = np.sum(A3[np.arange(K), :, np.arange(K)] + JITTER, axis=-1)          # [K]
    u = (B - AkD) / Akk[:, None] + D
    nrm = np.sqrt(np.maximum(np.sum(np.abs(u) ** 2, axis=-1), 1.0))
    S = (np.abs(B) + np.einsum('kfj,jf->kf', np.abs(A3), np.abs(D))) / np.abs(Akk)[:, None] + np.abs(D)
    return u / nrm[:, None], u, nrm, S


def step(x, y, m, D, A3_old, B_old, beta):
    """Everything behind the LASSO -> A3, B, D_new, max|D - D_new|."""
    A3, B = stats(x, y, m, A3_old, B_old, beta)
    D_new = atom_update(D, A3, B)[0]
    return A3, B, D_new, float(np.max(np.abs(up(D) - D_new)))


def maxdiff(D, D_new):
    """max|D - D_new| with the difference taken in the arrays' own precision (as the device takes it) and the
    modulus in double."""
    d = np.asarray(D) - np.asarray(D_new)
    return float(np.max(np.abs(up(d))))


class Problem(object):
    """One masked step's inputs in dtype `dt`:
      D          strictly normalised [K, F]
      y          x_true D + 0.1 noise
      x0         the warm start: x_true's support with perturbed values
      m          the mask, binary (uniform > 0.3) or fractional in (0, 1]
      A3_old, B_old   the statistics of a SECOND random sparse code matrix (with its own data and mask)
      kz         a code column that is zero in x_true, x0 and the old statistics
      fz         a channel masked in every row (of both masks)
    Row 0 of the codes holds a large entry, so that a sum which loses row 0 is wrong."""

    def __init__(self, dt, Nb, F, K, fractional, seed):
        rng = np.random.RandomState(seed)
        cplx = np.dtype(dt).kind == 'c'
        rdt = np.float32 if is_single(dt) else np.float64

        def randn(*s):
            return (rng.randn(*s) + 1j * rng.randn(*s)) if cplx else rng.randn(*s)
        self.kz, self.fz = K // 2, F // 2
        density = max(0.15, 1.5 / K)

        def codes():
            c = 3.0 * randn(Nb, K) * (rng.uniform(size=(Nb, K)) < density)
            c[0, (self.kz + 1) % K] = 8.0
            c[:, self.kz] = 0
            return c

        def mask():
            mm = (1.0 - rng.uniform(size=(Nb, F))) if fractional else (rng.uniform(size=(Nb, F)) > 0.3) * 1.0
            mm[:, self.fz] = 0
            return mm
        D = l2_strict(randn(K, F))
        x_true, x_old = codes(), codes()
        m, m_old = mask(), mask()
        y = x_true.dot(D) + 0.1 * randn(Nb, F)
        y_old = x_old.dot(D) + 0.1 * randn(Nb, F)
        A3_old, B_old = stats(x_old, y_old, m_old, np.zeros((K, F, K)), np.zeros((K, F)), 0.0)
        x0 = x_true * (1.0 + 0.2 * rng.randn(Nb, K))
        self.D, self.y, self.x0 = D.astype(dt), y.astype(dt), x0.astype(dt)
        self.m = m.astype(rdt)
        self.A3_old, self.B_old = A3_old.astype(dt), B_old.astype(dt)
        self.Nb, self.F, self.K, self.dt = Nb, F, K, np.dtype(dt)

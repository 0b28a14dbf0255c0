"""Approximate K-SVD on MI355X -- dictionary learning with a GIVEN sparsity,

    argmin_{x, D} |y - x D|^2   s.t.  |x_i|_0 <= n_nonzero_coefs,  |D_k| = 1

(Rubinstein, Zibulevsky & Elad 2008), the trainer that goes with the coder of ``decomp_amd.omp``.  Every iteration
codes all rows by orthogonal matching pursuit, forms the residual R = y - x D once and sweeps the atoms in order:
atom k and the coefficients of the rows that use it are replaced by one power step on those rows' residual, which
re-fits the coefficients on the support the coder found and never increases |y - x D|^2.  Batch only.  Shapes,
dtypes and the NumPy / torch convention are those of ``omp.solve``.  One iteration is one call into
libdecomp_hip.so (``dcp_ksvd_step_*``; decomp_amd/csrc/ksvd.hpp states the algorithm and the kernels).

With ``mask`` the training set itself may have holes: the objective is  sum_if m_if |y_if - (x D)_if|^2, the coder is
that of ``omp.solve(mask=...)`` and every inner product of the atom sweep is weighted per row
(``dcp_ksvd_mask_step_*``, decomp_amd/csrc/ksvd_mask.hpp); no atom step increases the weighted objective.

With ``replace_atoms`` every iteration that is followed by another one ends with a cleaning pass: atoms no row uses
and atoms nearly parallel to an earlier one are replaced by the worst-represented training rows
(``dcp_ksvd_clean_step_*``, decomp_amd/csrc/ksvd_clean.hpp states the rule and the kernels).
"""
import ctypes
import math
import numbers

import numpy as np

from . import _arrays, _hip, omp
from ._arrays import get_array_module
from .utils import assertion


def _check_loop(tol, maxiter):
    ok = isinstance(tol, numbers.Real) and not isinstance(tol, (bool, np.bool_)) and not math.isnan(tol)
    if not ok:
        raise ValueError('tol must be a number. Given {!r}'.format(tol))
    ok = isinstance(maxiter, numbers.Integral) and not isinstance(maxiter, (bool, np.bool_))
    if not ok or maxiter < 1:
        raise ValueError('maxiter must be a positive integer. Given {!r}'.format(maxiter))
    return float(tol), int(maxiter)


def _check_replace(replace_atoms, max_coherence):
    if not isinstance(replace_atoms, (bool, np.bool_)):
        raise ValueError('replace_atoms must be a bool. Given {!r}'.format(replace_atoms))
    if max_coherence is None:
        return bool(replace_atoms), 0.0
    ok = isinstance(max_coherence, numbers.Real) and not isinstance(max_coherence, (bool, np.bool_))
    if not ok or not 0.0 < max_coherence < 1.0:       # a NaN fails both comparisons
        raise ValueError('max_coherence must be a number in (0, 1) or None. Given {!r}'.format(max_coherence))
    return bool(replace_atoms), float(max_coherence)


def solve(y, D, n_nonzero_coefs, tol=1.0e-3, maxiter=1000, coef_tol=None, mask=None, replace_atoms=False,
          max_coherence=0.99):
    """
    Learn a dictionary for codes with at most n_nonzero_coefs atoms per row.

    y: [n_samples, n_channels], D: [n_features, n_channels] (atoms are rows; normalised to unit rows on entry);
    float or complex, both of one dtype; NumPy (results returned as NumPy) or torch CUDA tensors.
    n_nonzero_coefs: the sparsity (<= 64 real, <= 32 complex).
    coef_tol: the coder also stops a row once |y - x D|^2 <= coef_tol (None: no such stop).
    tol, maxiter: for it = 1 .. maxiter - 1, one iteration; stop once max|D_new - D_old| < tol.
    mask: real, non-negative weights m of the samples, y's shape or [n_channels]; None: the unweighted problem.
        With a mask the objective is  sum_if m_if |y_if - (x D)_if|^2  (coef_tol bounds a row's weighted residual):
        a sample with m = 0 is missing.  The weights enter linearly, as in ``omp.solve(mask=...)``; the mask is cast
        to the real dtype of y.  y must be finite at the hidden entries too; its values there do not influence the
        result.  x @ D fills the holes; a row without any observed sample gets x = 0.
    replace_atoms (bool): False: an atom that no row uses is left as it is, and so is a duplicate.  True: an
        iteration that is followed by another one (max|D_new - D_old| >= tol, and not the last that maxiter allows)
        ends with a cleaning pass.  For k = 0, 1, ... in order atom k is marked if no row uses it, or if
        |<D_k, D_j>| > max_coherence for an earlier atom j that is not marked itself (of a coherent pair the lower
        index survives).  The j-th marked atom becomes the normalised row of y with the j-th largest (weighted)
        residual  sum_f m_if |y_if - (x D)_if|^2,  ties to the lower row; hidden entries of the row are filled with
        x @ D.  A row with zero residual replaces nothing.  x is not touched, so the pass never runs on the iteration
        whose result is returned, and the jump of a replaced atom does not count towards max|D_new - D_old|.
    max_coherence: a number in (0, 1), or None to replace unused atoms only.  Checked, but without effect, when
        replace_atoms is False.
    Returns (it, D, x): x [n_samples, n_features] holds the coefficients re-fitted for the returned D.

    Not built: minibatches (online K-SVD), sharding, out-of-core y, exact (SVD) K-SVD, a minimum-use threshold for
    the replacement.
    """
    kind = get_array_module(y, D, mask)
    assertion.assert_dtypes(y=y, D=D)
    assertion.assert_mask(mask)
    assertion.assert_ndim('y', y, ndim=2)
    assertion.assert_ndim('D', D, ndim=2)
    assertion.assert_shapes('y', y, 'D', D, axes=[-1])
    assertion.assert_mask_shape(y, mask)
    K, F = int(D.shape[0]), int(D.shape[1])
    s = omp.check_sparsity(n_nonzero_coefs, K, _arrays.np_dtype(D))
    coef_tol_c = omp.check_tol(coef_tol, what='coef_tol')
    tol, maxiter = _check_loop(tol, maxiter)
    replace_atoms, mu = _check_replace(replace_atoms, max_coherence)

    import torch
    Dd = _arrays.to_device(D, copy=True)
    dev = Dd.device.index
    yd = _arrays.to_device(y, dev)
    N = int(yd.shape[0])
    xd = torch.zeros((N, K), dtype=Dd.dtype, device=Dd.device)
    it = 1
    if N > 0:
        _arrays.l2_normalize_(Dd, strict=True)
        maxdiff = ctypes.c_double(0.0)
        omp_it = ctypes.c_int(0)
        md, mask_ndim = _arrays.mask_to_device(mask, yd, N, F)
        n_marked = ctypes.c_int(0)
        if replace_atoms:
            name = 'dcp_ksvd_clean_step_' + _arrays.suffix(Dd)
            args = (_arrays.ptr(yd), _arrays.ptr(md), mask_ndim if md is not None else 0, _arrays.ptr(xd),
                    _arrays.ptr(Dd), N, F, K, s, coef_tol_c, 0)
        elif md is None:
            name = 'dcp_ksvd_step_' + _arrays.suffix(Dd)
            args = (_arrays.ptr(yd), _arrays.ptr(xd), _arrays.ptr(Dd), N, F, K, s, coef_tol_c)
        else:
            name = 'dcp_ksvd_mask_step_' + _arrays.suffix(Dd)
            args = (_arrays.ptr(yd), _arrays.ptr(md), mask_ndim, _arrays.ptr(xd), _arrays.ptr(Dd), N, F, K, s,
                    coef_tol_c, 0)
        try:
            for it in range(1, maxiter):
                lib, h = _arrays.lib_handle(Dd)
                out = (ctypes.byref(maxdiff), ctypes.byref(omp_it))
                if replace_atoms:     # no cleaning on the last iteration: the returned x belongs to the returned D
                    out += (mu, tol if it < maxiter - 1 else math.inf, ctypes.byref(n_marked))
                rc = getattr(lib, name)(h, *args, *out)
                _hip.check(h, rc, name)
                if maxdiff.value < tol:
                    break
            else:
                it = maxiter
        except KeyboardInterrupt:
            torch.cuda.synchronize(dev)
    else:
        it = maxiter
    return it, _arrays.to_caller(Dd, kind), _arrays.to_caller(xd, kind)

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


def solve(y, D, n_nonzero_coefs, tol=1.0e-3, maxiter=1000, coef_tol=None, mask=None):
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
    Returns (it, D, x): x [n_samples, n_features] holds the coefficients re-fitted for the returned D.

    Not built: minibatches (online K-SVD), sharding, out-of-core y, exact (SVD) K-SVD.  An atom that no row uses
    is left as it is: unused atoms are not replaced.
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
        if md is None:
            name = 'dcp_ksvd_step_' + _arrays.suffix(Dd)
            args = (_arrays.ptr(yd), _arrays.ptr(xd), _arrays.ptr(Dd), N, F, K, s, coef_tol_c)
        else:
            name = 'dcp_ksvd_mask_step_' + _arrays.suffix(Dd)
            args = (_arrays.ptr(yd), _arrays.ptr(md), mask_ndim, _arrays.ptr(xd), _arrays.ptr(Dd), N, F, K, s,
                    coef_tol_c, 0)
        try:
            for it in range(1, maxiter):
                lib, h = _arrays.lib_handle(Dd)
                rc = getattr(lib, name)(h, *args, ctypes.byref(maxdiff), ctypes.byref(omp_it))
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

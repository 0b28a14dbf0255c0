"""Batched orthogonal matching pursuit on MI355X -- the sparse coder with a GIVEN sparsity,

    argmin_x |y - x A|^2   s.t.  |x|_0 <= n_nonzero_coefs        (and / or until |y - x A|^2 <= tol)

next to the L1 family of ``decomp_amd.lasso``.  Shapes, dtypes and the NumPy / torch convention are those of
``lasso.solve``.  Everything after validation runs in libdecomp_hip.so (``dcp_omp_*``: both products on the GEMM
cores, then the greedy kernel of decomp_amd/csrc/omp.hpp, which also states the algorithm).

With ``mask`` every row is coded on its observed samples only (``dcp_omp_mask_*``, decomp_amd/csrc/omp_mask.hpp):
the same greedy algorithm with every inner product weighted by the mask.
"""
import ctypes
import math
import numbers

import numpy as np

from . import _arrays, _hip
from ._arrays import get_array_module
from .utils import assertion

# the largest sparsity the kernel takes (the LDS image of the triangular factor)
CAP_REAL = 64
CAP_COMPLEX = 32


def sparsity_cap(dtype):
    """Largest n_nonzero_coefs for a NumPy dtype: 64 real, 32 complex."""
    return CAP_COMPLEX if np.dtype(dtype).kind == 'c' else CAP_REAL


def check_sparsity(n_nonzero_coefs, K, dtype, what='n_nonzero_coefs'):
    """The integer sparsity, or ValueError naming the cap."""
    cap = sparsity_cap(dtype)
    ok = isinstance(n_nonzero_coefs, numbers.Integral) and not isinstance(n_nonzero_coefs, (bool, np.bool_))
    if not ok or not 1 <= int(n_nonzero_coefs) <= min(K, cap):
        raise ValueError('{0} must be an integer in [1, min(n_features, {1:d})] (the cap is {2:d} for real and '
                         '{3:d} for complex dtypes; n_features = {4:d}). Given {5!r}'.format(
                             what, cap, CAP_REAL, CAP_COMPLEX, K, n_nonzero_coefs))
    return int(n_nonzero_coefs)


def check_tol(tol, what='tol'):
    """tol as the float the library takes: None -> -1.0 (no residual stop); negative or non-finite: ValueError."""
    if tol is None:
        return -1.0
    ok = isinstance(tol, numbers.Real) and not isinstance(tol, (bool, np.bool_))
    if not ok or not math.isfinite(tol) or tol < 0:
        raise ValueError('{0} must be a finite non-negative number or None. Given {1!r}'.format(what, tol))
    return float(tol)


def solve(y, A, n_nonzero_coefs=None, tol=None, mask=None):
    """
    Greedy solution of  argmin_x |y - xA|^2  s.t. |x|_0 <= n_nonzero_coefs  for every row of y.

    y: [..., n_channels], A: [n_features, n_channels]; float or complex, both of one dtype.
    n_nonzero_coefs: at most this many atoms per row (<= 64 real, <= 32 complex).
    tol: stop a row once |y - xA|^2 <= tol.  With tol alone the sparsity is min(n_features, n_channels, cap).
    mask: real, non-negative weights m of the samples, y's shape or [n_channels]; None: the unweighted problem.
        With a mask the objective is  sum_f m_f |y_f - (xA)_f|^2  (and tol bounds that weighted residual): a sample
        with m_f = 0 is missing, an atom is scored by its observed part only, and a row without any observed
        sample gets x = 0.  The weights enter LINEARLY (m, not m^2): the convention of the 2-D masks of
        ``lasso.solve`` and of ``nmf.solve(method='em-hals')``; for 0 / 1 masks it coincides with the 1-D
        convention of ``lasso.solve``.  The mask is cast to the real dtype of y.
    Returns (it, x): x [..., n_features] with zeros off the support, it the largest number of atoms any row took.
    """
    kind = get_array_module(y, A, mask)
    assertion.assert_dtypes(y=y, A=A)
    assertion.assert_mask(mask)
    assertion.assert_ndim('A', A, ndim=2)
    assertion.assert_shapes('y', y, 'A', A, axes=[-1])
    assertion.assert_mask_shape(y, mask)
    if n_nonzero_coefs is None and tol is None:
        raise ValueError('Either n_nonzero_coefs or tol must be given.')
    K, F = int(A.shape[0]), int(A.shape[1])
    dt = _arrays.np_dtype(A)
    tol_c = check_tol(tol)
    if n_nonzero_coefs is None:
        s = min(K, F, sparsity_cap(dt))
    else:
        s = check_sparsity(n_nonzero_coefs, K, dt)

    import torch
    yd = _arrays.to_device(y)
    dev = yd.device.index
    Ad = _arrays.to_device(A, dev)
    batch_shape = tuple(yd.shape[:-1])
    y2 = yd.reshape(-1, F).contiguous()
    N = y2.shape[0]
    xd = torch.empty((N, K), dtype=yd.dtype, device=yd.device)
    it = ctypes.c_int(0)
    if N > 0:
        lib, h = _arrays.lib_handle(yd)
        md, mask_ndim = _arrays.mask_to_device(mask, yd, N, F)
        if md is None:
            name = 'dcp_omp_' + _arrays.suffix(yd)
            rc = getattr(lib, name)(h, _arrays.ptr(y2), _arrays.ptr(Ad), _arrays.ptr(xd), N, F, K, s, tol_c,
                                    ctypes.byref(it))
        else:
            name = 'dcp_omp_mask_' + _arrays.suffix(yd)
            rc = getattr(lib, name)(h, _arrays.ptr(y2), _arrays.ptr(md), mask_ndim, _arrays.ptr(Ad), _arrays.ptr(xd),
                                    N, F, K, s, tol_c, 0, ctypes.byref(it))
        _hip.check(h, rc, name)
    return it.value, _arrays.to_caller(xd.reshape(batch_shape + (K,)), kind)

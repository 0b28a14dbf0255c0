"""1-D convolutional template learning -- drop-in for ``decomp.template_matching`` on MI355X.

Same entry points, argument meaning, return convention and error behaviour as the reference's
decomp/template_matching.py.  The reference builds the convolution as dense im2col matrices
(``_temp2mat`` [T, C, N], ``_coef2mat`` [B, T, S, N]) and has no GPU path; here nothing of that
size is formed on the hot path (include/decomp_hip.h ``dcp_tm_*``, decomp_amd/csrc/template_impl.hpp):

  * the LASSO step with 'ista', 'acc_ista', 'fista' (and their '_pos' forms) runs on the structured
    operator: one iteration is a residual pass over the signal and a correlation pass over the
    coefficients, the proximal step fused into the second;
  * the dictionary step's statistics XXt [T S, T S] and yX [T S] are built from lag correlations of
    the coefficients, and D is updated by one fused chain of small kernels;
  * ``pursuit`` (not in the reference) is greedy matching pursuit on the same operator, the coder with a given
    number of events per signal: one correlation pass, then one workgroup per signal that keeps the correlations
    up to date from the lag correlations of the templates (decomp_amd/csrc/template_pursuit.hpp);
  * ``orthogonal_pursuit`` (not in the reference) is its re-fitting form, batch OMP on the same operator: the Gram
    entries of the support are single reads of the lag correlations, the factor an s x s Cholesky per signal
    (decomp_amd/csrc/template_omp.hpp);
  * ``solve(alpha=0, lasso_method='omp' | 'mp' | 'mp_pos', lasso_iter=s, lasso_tol=tol)`` learns the templates for
    the codes of those two coders: the coder replaces the LASSO step, and the dictionary step sums its statistics over
    per-row lists of the non-zero coefficients instead of all C of them, bit for bit the dense step's result
    (``dcp_tm_dstep_events_*``, decomp_amd/csrc/template_events.hpp);
  * ``pursuit``, ``orthogonal_pursuit`` and ``predict`` take multichannel templates D [T, Ch, S] (y [..., Ch, N], one
    coefficient per event for all channels): every correlation, rho2 and |y|^2 gains a sum over the channels, in the
    kernels the one-channel coders run too; only the correlation pass and ``predict`` are kernels of their own
    (``dcp_tm_mc_*``, decomp_amd/csrc/template_multichannel.hpp);
  * ``solve`` with one of those greedy coders learns multichannel templates D [T, Ch, S] too: x is shared by the
    channels, so XXt stays the one-channel [T S, T S], only yX [T, Ch, S] gains the channel axis, the gradient step is
    XXt times the [T S, Ch] columns of D and a template is normalised over its Ch S entries
    (``dcp_tm_mc_dstep_events_*``, the same step of decomp_amd/csrc/template_events.hpp with Ch channels);
  * ``basis_pursuit`` (not in the reference) is the L1 coder of ``solve`` as a call of its own, for fixed templates: for
    D [T, S] the LASSO step above, for multichannel templates D [T, Ch, S] the same proximal-gradient iteration in
    Gram form, one kernel per iteration on the lag correlations of the templates, whose cost does not depend on Ch
    (``dcp_tm_mc_lasso_*``, decomp_amd/csrc/template_mc_lasso.hpp).

A 2-D D calls the un-prefixed entries and a 3-D D (Ch = 1 included) the ``mc_`` ones; ``_entry`` is the one place that
says which, and both reach the same C++ functions apart from the correlation pass and ``predict``.

'cd', 'parallel_cd' and 'admm' have no structured form: for them ``_temp2mat`` is materialised on the
device and the dense ``dcp_lasso_*`` solvers of decomp_amd.lasso run on it.  That path is correct but
dense (memory T C N, work per iteration of the dense solvers).

The outer loop reads one number per iteration from the device, max|dD|, for the reference's stop test.
"""
import ctypes
import numbers

import numpy as np

from . import _arrays, _hip, lasso
from ._arrays import get_array_module
from .utils import assertion, normalize
from .utils.exceptions import DtypeMismatchError
from .utils.data import minibatch_index

_JITTER = 1.0e-15
_STRUCTURED = ('ista', 'acc_ista', 'fista')
_DENSE = ('cd', 'parallel_cd', 'admm')
# lasso_method -> (the coder's dcp_tm_<name>_*, its flags after tol)
_GREEDY = {'omp': ('omp', ()), 'mp': ('pursuit', (0,)), 'mp_pos': ('pursuit', (1,))}


def solve(y, D, alpha, stride=1, padding='SAME', x=None, tol=1.0e-4,
          minibatch=None, size_of_minibatch=None, maxiter=1000,
          lasso_method='acc_ista', lasso_iter=10, lasso_tol=1.0e-5,
          mask=None, random_seed=None):
    """
    Learn templates with lasso regularisation,
        argmin_{x, D} |y - x * D|^2 + alpha |x|   s.t. |D_t|^2 <= 1,
    where x * D is the 1-D convolution of the coefficients x [..., T, C] with the templates D [T, S].

    y: [N] or [B, N]; D: initial templates [T, S]; x: optional initial coefficients [T, C] / [B, T, C]
    with C = _coef_size(S, N, stride, padding).  float or complex, all of one dtype.
    minibatch: number of windows of ``size_of_minibatch`` samples drawn per iteration
    (RandomState(random_seed)); None solves on the whole batch.
    lasso_method 'omp', 'mp' or 'mp_pos' solves the sparsity-constrained problem instead,
        argmin_{x, D} |y - x * D|^2   s.t. |x_b|_0 <= lasso_iter, |D_t|^2 <= 1,
    with ``orthogonal_pursuit``, ``pursuit`` or ``pursuit(positive=True)`` as the coder: alpha must be 0, lasso_iter is
    the coder's n_nonzero_coefs (per signal, or per window with minibatch) and lasso_tol its tol, the residual energy
    at which a signal stops (None: none) -- the convention of dictionary_learning.solve(lasso_method='omp').  The
    coders start from zero, so an ``x`` passed in is not read.  y must be finite.
    With a greedy coder the templates may be multichannel, D [T, Ch, S] for y [B, Ch, N] or [Ch, N] (one signal): the
    model is that of ``pursuit``, y[b, ch, n] ~ sum x[b, t, c] D[t, ch, n - stride c + Q] with x [B, T, C] (or [T, C]),
    and the constraint |D_t|^2 <= 1 is on the Ch S entries of a template.  Everything else keeps its meaning; the
    LASSO coders have no multichannel form (NotImplementedError).
    Returns (it, D, x) as the reference does.  NumPy in -> NumPy out; torch GPU tensors stay on the device.
    """
    get_array_module(y, D, x)                                         # template_matching.py:48
    Ch = _learn_channels(y, D, lasso_method)
    if lasso_method in _GREEDY:                                       # (the rest of its checks: solve_fastpath)
        stride, _ = _geometry(int(D.shape[0]), int(D.shape[-1]), int(y.shape[-1]), stride, padding)
    rng = np.random.RandomState(random_seed)
    x_given = x
    if x is None:
        coef_size = _coef_size(D.shape[-1], y.shape[-1], stride=stride, padding=padding)
        if len(y.shape) == (2 if Ch is None else 3):
            shape = (y.shape[0], D.shape[0], coef_size)
        else:
            shape = (D.shape[0], coef_size)
        x = lasso._ZerosLike(shape, _arrays.np_dtype(y))

    assertion.assert_dtypes(y=y, D=D, x=x)
    assertion.assert_dtypes(mask=mask, dtypes='f')
    assertion.assert_shapes('y', y, 'mask', mask)

    if minibatch is not None and size_of_minibatch is None:
        raise ValueError('size_of_minibatch should be specified with '
                         'minibatch calculation.')

    return solve_fastpath(y, D, alpha, x_given if x_given is not None else x, stride, padding,
                          tol, minibatch, size_of_minibatch, maxiter,
                          lasso_method, lasso_iter, lasso_tol, rng, None, mask=mask)


def solve_fastpath(y, D, alpha, x, stride, padding, tol,
                   minibatch, size_of_minibatch, maxiter,
                   lasso_method, lasso_iter, lasso_tol, rng, xp,
                   mask=None):
    """No defaults and no validation (``x`` may be the zeros placeholder of ``solve``); ``xp`` is
    accepted for signature compatibility, the array kind is taken from ``y``."""
    if mask is not None:
        raise NotImplementedError('Template matching with mask is not '
                                  'yet implemented.')
    Ch = _learn_channels(y, D, lasso_method)
    if lasso_method in _GREEDY:
        N = y.shape[-1] if minibatch is None else int(size_of_minibatch)
        _greedy_args(lasso_method, alpha, lasso_iter, lasso_tol, D.shape[0], D.shape[-1], N, stride, padding,
                     _arrays.np_dtype(y))
    import torch
    kind = 'torch' if _arrays.is_torch(y) else 'numpy'
    yd = _arrays.to_device(y)
    one_d = yd.dim() == (1 if Ch is None else 2)
    y2 = yd.unsqueeze(0) if one_d else yd
    if isinstance(x, lasso._ZerosLike):
        xd = torch.zeros(((1,) if one_d else ()) + tuple(x.shape), dtype=yd.dtype, device=yd.device)
    else:
        xd = _arrays.to_device(x, yd.device.index, copy=True)
        if one_d:
            xd = xd.unsqueeze(0)
    Dd = _arrays.to_device(D, yd.device.index)

    if minibatch is None:
        it, Dn, xn = solve_batch(y2, Dd, alpha, xd, stride, padding, tol, maxiter,
                                 lasso_method, lasso_iter, lasso_tol, xp)
    else:
        it, Dn, xn = solve_minibatch(y2, Dd, alpha, xd, stride, padding, tol,
                                     minibatch, size_of_minibatch, maxiter,
                                     lasso_method, lasso_iter, lasso_tol, rng, xp)
    if one_d:
        xn = xn.squeeze(0)
    return it, _arrays.to_caller(Dn, kind), _arrays.to_caller(xn, kind)


def _coef_size(template_size, size, stride=1, padding='VALID'):
    """Number of coefficients per template for a signal of ``size`` samples."""
    if padding == 'VALID':
        pad = size - template_size
    else:  # 'SAME'
        pad = size - 1
    return int(np.floor((template_size + 2 * pad - size) / stride + 1))


def _pad_code(padding):
    return 0 if padding == 'VALID' else 1


def _call(t, name, *args):
    """dcp_tm_<name>_<dtype of t>.  Tensor arguments are passed as device pointers; every floating or complex
    one must have t's dtype and every one must live on t's device (the kernel reads them as t's dtype), which
    is checked here rather than trusted."""
    fn_name = 'dcp_tm_%s_%s' % (name, _arrays.suffix(t))
    conv = []
    for a in args:
        if _arrays.is_torch(a):
            if (a.is_floating_point() or a.is_complex()) and a.dtype != t.dtype:
                raise DtypeMismatchError('%s: an argument is %s, the problem is %s' % (fn_name, a.dtype, t.dtype))
            if a.device != t.device:
                raise ValueError('%s: arguments on %s and %s' % (fn_name, a.device, t.device))
            if not a.is_contiguous():
                raise ValueError('%s: arguments must be contiguous' % fn_name)
            a = _arrays.ptr(a)
        conv.append(a)
    lib, h = _arrays.lib_handle(t)
    _hip.check(h, getattr(lib, fn_name)(h, *conv), fn_name)


def _same_device(*tensors):
    devs = set(t.device for t in tensors if t is not None)
    if len(devs) > 1:
        raise ValueError('all arrays must live on one device, given %s' % sorted(str(d) for d in devs))


def _temp2mat(D, size, stride, padding, xp=None):
    """The im2col operator of the templates, [T, C, size] (A[(t, c), n] = D[t, n - stride c + Q])."""
    import torch
    kind = get_array_module(D)
    Dd = _arrays.to_device(D)
    T, S = Dd.shape
    C = _coef_size(S, size, stride, padding)
    out = torch.empty((T, C, size), dtype=Dd.dtype, device=Dd.device)
    _call(Dd, 'temp2mat', Dd, T, S, size, stride, _pad_code(padding), out)
    return _arrays.to_caller(out, kind)


def _coef2mat(x_orig, size, template_size, stride, padding, xp=None):
    """The im2col matrix of the coefficients: [T, S, size] for x [T, C], [B, T, S, size] for x [B, T, C]."""
    import torch
    kind = get_array_module(x_orig)
    xd = _arrays.to_device(x_orig)
    x3 = xd.unsqueeze(0) if xd.dim() == 2 else xd
    B, T, C = x3.shape
    if C != _coef_size(template_size, size, stride, padding):
        raise ValueError('x has %d coefficients per template, the geometry needs %d'
                         % (C, _coef_size(template_size, size, stride, padding)))
    out = torch.empty((B, T, template_size, size), dtype=xd.dtype, device=xd.device)
    _call(x3, 'coef2mat', x3, B, T, template_size, size, stride, _pad_code(padding),
          out)
    if xd.dim() == 2:
        out = out.squeeze(0)
    return _arrays.to_caller(out, kind)


def predict(x, D, size, stride=1, padding='SAME'):
    """The signal x * D: x [..., T, C], D [T, S] -> [..., size], or with multichannel templates D [T, Ch, S]
    -> [..., Ch, size] (mixed dtypes compute in the promoted one)."""
    import torch
    kind = get_array_module(x, D)
    Ch = _channels(D)
    xd = _arrays.to_device(x)
    Dd = _arrays.to_device(D, xd.device.index)
    _same_device(xd, Dd)
    # mixed dtypes compute in the promoted one, as the reference's tensordot does
    dt = torch.promote_types(xd.dtype, Dd.dtype)
    xd, Dd = xd.to(dt).contiguous(), Dd.to(dt).contiguous()
    T, S = int(Dd.shape[0]), int(Dd.shape[-1])
    C = _coef_size(S, size, stride, padding)
    if tuple(xd.shape[-2:]) != (T, C):
        raise ValueError('shape-mismatch for sum: x%s with templates [%d, %d] over %d samples'
                         % (tuple(xd.shape), T, S, size))
    lead = tuple(xd.shape[:-2])
    x3 = xd.reshape((-1, T, C))
    B = x3.shape[0]
    entry, dims = _entry('predict', T, Ch, S)
    chs = () if Ch is None else (Ch,)
    out = torch.empty((B,) + chs + (size,), dtype=xd.dtype, device=xd.device)
    if B > 0 or Ch is None:                                           # (templates [T, S]: the library refuses B = 0)
        _call(x3, entry, x3, Dd, B, *(dims + (size, stride, _pad_code(padding), out)))
    return _arrays.to_caller(out.reshape(lead + chs + (size,)), kind)


def pursuit(y, D, n_nonzero_coefs=None, tol=None, stride=1, padding='SAME', positive=False):
    """
    Greedy matching pursuit of every signal on the shift-invariant dictionary of the templates: peel off at most
    ``n_nonzero_coefs`` events per signal, or stop once the residual energy |y - x * D|^2 is <= ``tol``.

    y: [..., N]; D: templates [T, S], S <= N, used as given (not normalised); float or complex, both of one dtype.
    With A[(t, c), n] = D[t, n - stride c + Q] and rho2[t, c] = |A_(t,c)|^2 over the taps inside the signal, a step
    takes the atom with the largest |r . A_(t,c)^H|^2 / rho2 (the lowest flat index t C + c on ties) and adds
    r . A^H / rho2 to its coefficient; ``positive`` (real dtypes) takes only atoms that correlate positively.  A signal
    also stops when no atom scores above zero.
    This is matching pursuit, not OMP: there is no re-fit on the support, and an atom may be taken again (its
    coefficient accumulates), so ``n_nonzero_coefs`` bounds the STEPS and hence the non-zeros.  There is no sparsity
    cap; with ``tol`` alone the step limit is T C.
    Multichannel templates: a 3-D D [T, Ch, S] codes y [..., Ch, N] with one coefficient per event for all Ch channels,
    y[ch, n] ~ sum x[t, c] D[t, ch, n - stride c + Q]; correlations, rho2 and the residual energy (hence ``tol``) are
    sums over all channels, everything else is unchanged (``dcp_tm_mc_pursuit_*``, Ch = 1 included).
    Returns (it, x): x [..., T, C] in the layout of ``solve`` / ``predict`` (``predict(x, D, N, stride, padding)`` is
    the approximation), it the largest number of steps any signal took.  NumPy in -> NumPy out; torch GPU tensors
    stay on the device.  Runs in libdecomp_hip.so (``dcp_tm_pursuit_*``, decomp_amd/csrc/template_pursuit.hpp).
    """
    from . import omp
    kind, stride, T, S, N, C, Ch = _pursuit_geometry(y, D, n_nonzero_coefs, tol, stride, padding)
    tol_c = omp.check_tol(tol)
    n_steps = _pursuit_steps(n_nonzero_coefs, T, C)
    if not isinstance(positive, (bool, np.bool_)):
        raise ValueError('positive must be a bool. Given {0!r}'.format(positive))
    _check_positive(positive, _arrays.np_dtype(y))

    return _pursuit_call('pursuit', kind, y, D, T, S, N, C, Ch, stride, padding, n_steps, tol_c,
                         1 if positive else 0)


def orthogonal_pursuit(y, D, n_nonzero_coefs=None, tol=None, stride=1, padding='SAME'):
    """
    Orthogonal matching pursuit of every signal on the shift-invariant dictionary of the templates: take at most
    ``n_nonzero_coefs`` events per signal, re-fitting the coefficients of all events taken so far after each one, or
    stop once the residual energy |y - x * D|^2 is <= ``tol``.

    y: [..., N]; D: templates [T, S], S <= N, used as given (not normalised); float or complex, both of one dtype.
    With A[(t, c), n] = D[t, n - stride c + Q] and rho2[t, c] = |A_(t,c)|^2 over the taps inside the signal, a step
    takes the atom outside the support with the largest |r . A_(t,c)^H|^2 / rho2 (the lowest flat index t C + c on
    ties); x on the support is then the least-squares fit of y, so the residual is orthogonal to every atom taken and
    overlapping events are not biased as they are in ``pursuit``.  A signal also stops when no atom scores above zero
    or the best atom is numerically in the span of the support (its Cholesky pivot is <= 4096 eps rho2).
    ``n_nonzero_coefs`` is an integer in [1, min(T C, cap)], cap = 64 for real and 32 for complex dtypes (that of
    ``omp.solve``); with ``tol`` alone the limit is min(T C, cap).  Longer recordings are coded in windows.
    Multichannel templates: a 3-D D [T, Ch, S] codes y [..., Ch, N] as in ``pursuit`` (``dcp_tm_mc_omp_*``).
    Returns (it, x): x [..., T, C] in the layout of ``solve`` / ``predict`` / ``pursuit``, it the largest support any
    signal reached.  NumPy in -> NumPy out; torch GPU tensors stay on the device.  The dense operator and its Gram
    matrix are never formed: the Gram entries are read from the lag correlations of the templates
    (``dcp_tm_omp_*``, decomp_amd/csrc/template_omp.hpp).
    """
    from . import omp
    kind, stride, T, S, N, C, Ch = _pursuit_geometry(y, D, n_nonzero_coefs, tol, stride, padding)
    tol_c = omp.check_tol(tol)
    n_steps = _orthogonal_steps(n_nonzero_coefs, T, C, _arrays.np_dtype(y))
    return _pursuit_call('omp', kind, y, D, T, S, N, C, Ch, stride, padding, n_steps, tol_c)


def basis_pursuit(y, D, alpha, x=None, tol=1.0e-5, maxiter=10, method='acc_ista', stride=1, padding='SAME'):
    """
    L1 codes of every signal on the shift-invariant dictionary of the templates,
        argmin_x 1 / (2 n) |y - x * D|^2 + alpha |x|,
    the coder ``solve`` runs by default, for fixed templates: it needs no event count in advance.

    y: [..., N]; D: templates [T, S], S <= N, used as given; x: optional initial estimate [..., T, C] (copied, not
    overwritten; None: zero); float or complex, all of one dtype.  The result is
    ``lasso.solve(y, A, alpha, x, tol, method, maxiter)`` on the dense operator A[(t, c), n] = D[t, n - stride c + Q],
    which is never formed for 'ista', 'acc_ista', 'fista' and their '_pos' forms (``dcp_tm_lasso_*``: a residual pass
    and a correlation pass per iteration); 'cd', 'parallel_cd' and 'admm' run the dense solvers on it.
    Multichannel templates: a 3-D D [T, Ch, S] codes y [..., Ch, N] with one coefficient per event for all Ch channels
    (the model of ``pursuit``); the dense operator is A [T C, Ch N], n = Ch N.  The solver is proximal gradient in Gram
    form (``dcp_tm_mc_lasso_*``, decomp_amd/csrc/template_mc_lasso.hpp, Ch = 1 included): y is read once, by the
    correlation pass of the greedy coders, and an iteration is one kernel on the lag correlations of the templates whose
    cost does not depend on Ch.  'ista', 'acc_ista', 'fista' and their '_pos' forms only (NotImplementedError
    otherwise).  With 'SAME' the Gram entries of the atoms that reach outside the signal are tabulated per call; the
    library refuses templates so wide that this table exceeds 1 GiB.
    Returns (it, x): x [..., T, C] in the layout of ``solve`` / ``predict``, it the iteration count as ``lasso.solve``
    reports it.  NumPy in -> NumPy out; torch GPU tensors stay on the device.
    """
    import torch
    kind = get_array_module(y, D, x)
    Ch = _channels(D)
    if len(y.shape) < (1 if Ch is None else 2):
        raise assertion.DimInvalidError('y must have at least %d dimension%s' % ((1, '') if Ch is None else (2, 's')))
    _check_y_channels(y, D, Ch)
    T, S, N = int(D.shape[0]), int(D.shape[-1]), int(y.shape[-1])
    stride, C = _geometry(T, S, N, stride, padding)
    sig = (N,) if Ch is None else (Ch, N)                             # the dimensions of one signal
    lead = tuple(y.shape[:-len(sig)])
    if x is None:
        assertion.assert_dtypes(y=y, D=D)
    else:
        assertion.assert_dtypes(y=y, D=D, x=x)
        if tuple(x.shape) != lead + (T, C):
            raise ValueError('x{0} must be {1}: the batch dimensions of y{2}, then [T, C] = [{3:d}, {4:d}]'.format(
                tuple(x.shape), lead + (T, C), tuple(y.shape), T, C))
    if not isinstance(alpha, (int, float, np.integer, np.floating)) or isinstance(alpha, (bool, np.bool_)) \
            or not alpha >= 0:
        raise ValueError('alpha must be a non-negative number. Given {0!r}'.format(alpha))
    if not isinstance(tol, (int, float, np.integer, np.floating)) or isinstance(tol, (bool, np.bool_)) or not tol >= 0:
        raise ValueError('tol must be a non-negative number. Given {0!r}'.format(tol))
    if not _is_int(maxiter) or int(maxiter) < 1:
        raise ValueError('maxiter must be a positive integer. Given {0!r}'.format(maxiter))
    base = method[:-4] if isinstance(method, str) and method.endswith('_pos') else method
    if base not in _STRUCTURED + _DENSE:
        raise ValueError('Available methods are {0} and their _pos forms. Given {1!r}'.format(
            list(_STRUCTURED + _DENSE), method))
    _check_positive(base != method, _arrays.np_dtype(y))
    if Ch is not None and base not in _STRUCTURED:
        raise NotImplementedError('multichannel templates D [T, Ch, S] are coded with {0} and their _pos forms only. '
                                  'Given {1!r}'.format(list(_STRUCTURED), method))

    yd = _arrays.to_device(y)
    Dd = _arrays.to_device(D, yd.device.index).contiguous()
    y2 = yd.reshape((-1,) + sig).contiguous()
    B = y2.shape[0]
    if x is None:
        xd = torch.zeros((B, T, C), dtype=yd.dtype, device=yd.device)
    else:
        xd = _arrays.to_device(x, yd.device.index, copy=True).reshape(B, T, C).contiguous()
    _same_device(yd, Dd, xd)
    it = 0
    if B > 0 and Ch is None:
        it = _lasso(y2, Dd, xd, alpha, stride, padding, method, int(maxiter), tol)
    elif B > 0:
        out = ctypes.c_int(0)
        _call(y2, 'mc_lasso', y2, Dd, xd, B, T, Ch, S, N, stride, _pad_code(padding), float(alpha), float(tol),
              int(maxiter), lasso._METHOD_CODE[base], 1 if base != method else 0, ctypes.byref(out))
        it = out.value
    return it, _arrays.to_caller(xd.reshape(lead + (T, C)), kind)


def _pursuit_steps(n_nonzero_coefs, T, C):
    """The step limit of ``pursuit``: n_nonzero_coefs in [1, T C] (None: T C)."""
    if n_nonzero_coefs is None:
        return T * C
    if not _is_int(n_nonzero_coefs) or not 1 <= int(n_nonzero_coefs) <= T * C:
        raise ValueError('n_nonzero_coefs must be an integer in [1, T C = {0:d}]. Given {1!r}'.format(
            T * C, n_nonzero_coefs))
    return int(n_nonzero_coefs)


def _check_positive(positive, dt):
    if positive and np.dtype(dt).kind == 'c':
        raise ValueError('positive=True needs a real dtype.')


def _orthogonal_steps(n_nonzero_coefs, T, C, dt):
    """The step limit of ``orthogonal_pursuit``: n_nonzero_coefs in [1, min(T C, cap)] (None: the largest)."""
    from . import omp
    most = min(T * C, omp.sparsity_cap(dt))
    if n_nonzero_coefs is None:
        return most
    if not _is_int(n_nonzero_coefs) or not 1 <= int(n_nonzero_coefs) <= most:
        raise ValueError('n_nonzero_coefs must be an integer in [1, min(T C = {0:d}, {1:d})] (the cap is {2:d} for '
                         'real and {3:d} for complex dtypes). Given {4!r}'.format(
                             T * C, omp.sparsity_cap(dt), omp.CAP_REAL, omp.CAP_COMPLEX, n_nonzero_coefs))
    return int(n_nonzero_coefs)


def _geometry(T, S, N, stride, padding):
    """(stride, C) of templates [T, S] on signals of N samples, or ValueError."""
    if padding not in ('SAME', 'VALID'):
        raise ValueError("padding must be 'SAME' or 'VALID'. Given {0!r}".format(padding))
    if not _is_int(stride) or int(stride) < 1:
        raise ValueError('stride must be a positive integer. Given {0!r}'.format(stride))
    if T < 1 or S < 1 or S > N:
        raise ValueError('templates [{0:d}, {1:d}] need 1 <= T and 1 <= S <= N = {2:d}'.format(T, S, N))
    return int(stride), _coef_size(S, N, stride=int(stride), padding=padding)


def _pursuit_geometry(y, D, n_nonzero_coefs, tol, stride, padding):
    """The argument checks the greedy coders share, before any GPU call: (kind, stride, T, S, N, C, Ch), Ch None for
    templates [T, S] and the number of channels for templates [T, Ch, S] (y [..., Ch, N])."""
    kind = get_array_module(y, D)
    assertion.assert_dtypes(y=y, D=D)
    Ch = _channels(D)
    if len(y.shape) < (1 if Ch is None else 2):
        raise assertion.DimInvalidError('y must have at least %d dimension%s' % ((1, '') if Ch is None else (2, 's')))
    _check_y_channels(y, D, Ch)
    T, S = int(D.shape[0]), int(D.shape[-1])
    N = int(y.shape[-1])
    stride, C = _geometry(T, S, N, stride, padding)
    if n_nonzero_coefs is None and tol is None:
        raise ValueError('Either n_nonzero_coefs or tol must be given.')
    return kind, stride, T, S, N, C, Ch


def _channels(D):
    """None for templates [T, S], Ch >= 1 for multichannel templates [T, Ch, S]; anything else raises."""
    if len(D.shape) == 2:
        return None
    if len(D.shape) != 3:
        raise assertion.DimInvalidError('D must have 2 ([T, S]) or 3 ([T, Ch, S]) dimensions, has %d' % len(D.shape))
    if int(D.shape[1]) < 1:
        raise ValueError('multichannel templates [T, Ch, S] need Ch >= 1. Given D{0}'.format(tuple(D.shape)))
    return int(D.shape[1])


def _check_y_channels(y, D, Ch):
    """y [..., Ch, N] (at least 2-D) has the Ch channels of the templates D [T, Ch, S]; Ch None: nothing to check."""
    if Ch is not None and int(y.shape[-2]) != Ch:
        raise assertion.DimInvalidError('y{0} must be [..., Ch, N] with the Ch = {1:d} channels of the templates '
                                        'D{2}'.format(tuple(y.shape), Ch, tuple(D.shape)))


def _entry(name, T, Ch, S):
    """The library entry for templates [T, S] (Ch None) or [T, Ch, S] and the template dimensions it takes:
    (name, (T, S)) or ('mc_' + name, (T, Ch, S))."""
    return (name, (T, S)) if Ch is None else ('mc_' + name, (T, Ch, S))


def _learn_channels(y, D, lasso_method):
    """The channels of the templates ``solve`` is given (``_channels``), and for multichannel ones the checks on
    lasso_method and y [B, Ch, N] / [Ch, N].  No GPU call."""
    Ch = _channels(D)
    if Ch is None:
        return None
    if lasso_method not in _GREEDY:
        raise NotImplementedError('multichannel templates D [T, Ch, S] are learnt with lasso_method in {0} only. '
                                  'Given {1!r}'.format(sorted(_GREEDY), lasso_method))
    if len(y.shape) not in (2, 3):
        raise assertion.DimInvalidError('y must be [B, Ch, N] or [Ch, N] for templates D [T, Ch, S], has %d '
                                        'dimension(s)' % len(y.shape))
    _check_y_channels(y, D, Ch)
    return Ch


def _greedy_args(lasso_method, alpha, lasso_iter, lasso_tol, T, S, N, stride, padding, dt):
    """``solve`` with a greedy coder (lasso_method in _GREEDY) on signals (or windows) of N samples: alpha must be 0,
    lasso_iter is the coder's n_nonzero_coefs and lasso_tol its tol, each checked by the coder's own rule.  No GPU
    call.  Returns (n_steps, tol as the library takes it, max_events of the dictionary step)."""
    from . import omp
    if not (isinstance(alpha, (int, float, np.integer, np.floating)) and alpha == 0):
        raise ValueError('lasso_method={0!r} solves the sparsity-constrained problem, which has no L1 penalty: '
                         'alpha must be 0. Given {1!r}'.format(lasso_method, alpha))
    stride, C = _geometry(int(T), int(S), int(N), stride, padding)
    if lasso_iter is None and lasso_tol is None:
        raise ValueError('Either lasso_iter (the n_nonzero_coefs of {0!r}) or lasso_tol (its tol) must be '
                         'given.'.format(lasso_method))
    tol_c = omp.check_tol(lasso_tol)
    if lasso_method == 'omp':
        n_steps = _orthogonal_steps(lasso_iter, T, C, dt)
    else:
        n_steps = _pursuit_steps(lasso_iter, T, C)
        _check_positive(lasso_method == 'mp_pos', dt)
    return n_steps, tol_c, min(n_steps, C)


def _pursuit_call(name, kind, y, D, T, S, N, C, Ch, stride, padding, n_steps, tol_c, *flags):
    """The coder ``_entry`` names, dcp_tm_<name>_* on the signals of y flattened to [B, N] or, with Ch channels (not
    None), dcp_tm_mc_<name>_* on y flattened to [B, Ch, N]: (it, x [..., T, C])."""
    import torch
    yd = _arrays.to_device(y)
    Dd = _arrays.to_device(D, yd.device.index).contiguous()
    _same_device(yd, Dd)
    it = ctypes.c_int(0)
    entry, dims = _entry(name, T, Ch, S)
    sig = (N,) if Ch is None else (Ch, N)                             # the dimensions of one signal
    lead = tuple(yd.shape[:-len(sig)])
    y2 = yd.reshape((-1,) + sig).contiguous()
    B = y2.shape[0]
    if B > 0:
        xd = torch.empty((B, T, C), dtype=yd.dtype, device=yd.device)
        _call(y2, entry, y2, Dd, xd, B, *(dims + (N, stride, _pad_code(padding), n_steps, tol_c) + flags
                                          + (ctypes.byref(it),)))
    else:
        xd = torch.zeros((0, T, C), dtype=yd.dtype, device=yd.device)
    return it.value, _arrays.to_caller(xd.reshape(lead + (T, C)), kind)


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, (bool, np.bool_))


def _lasso(y, D, x, alpha, stride, padding, lasso_method, lasso_iter, lasso_tol):
    """solve_fastpath of lasso.py on the template operator; x [B, T, C] is updated in place."""
    base = lasso_method[:-4] if lasso_method.endswith('_pos') else lasso_method
    positive = lasso_method.endswith('_pos')
    B, N = y.shape
    T, S = D.shape
    if base in _STRUCTURED:
        it = ctypes.c_int(0)
        _call(y, 'lasso', y, D, x, B, T, S, N, stride,
              _pad_code(padding), float(alpha), float(lasso_tol), int(lasso_iter),
              lasso._METHOD_CODE[base], 1 if positive else 0, ctypes.byref(it))
        return it.value
    if base in _DENSE:
        A = _temp2mat(D, N, stride, padding).reshape(-1, N)
        it, xn = lasso.solve_fastpath(y, A, alpha, x.reshape(B, -1), lasso_tol, lasso_iter,
                                      lasso_method, None)
        x.copy_(xn.reshape(x.shape))
        return it
    raise NotImplementedError('Method ' + base + ' is not yet implemented.')


def _dstep(y, x, D, XXt, yX, stride, padding, acc_it):
    """Statistics of (y, x) into XXt / yX (written, or added / acc_it) and the update of D in place;
    returns max|D - D_new|."""
    B, N = y.shape
    T, S = D.shape
    out = ctypes.c_double(0.0)
    _call(y, 'dstep', y, x, D, XXt, yX,
          B, T, S, N, stride, _pad_code(padding), int(acc_it), ctypes.byref(out))
    return out.value


def _dstep_events(y, x, D, XXt, yX, stride, padding, acc_it, max_events):
    """``_dstep`` for a sparse x: the statistics are summed over lists of at most ``max_events`` non-zeros per
    (signal, template) row (a row with more is walked in full).  The same bits as ``_dstep``; y and x finite.
    With y [B, Ch, N] and D [T, Ch, S] (updated in place) yX is [T Ch S]; XXt stays [T S, T S]."""
    entry, dims = _entry('dstep_events', int(D.shape[0]), _channels(D), int(D.shape[-1]))
    out = ctypes.c_double(0.0)
    _call(y, entry, y, x, D, XXt, yX, y.shape[0], *(dims + (y.shape[-1], stride, _pad_code(padding), int(acc_it),
                                                            int(max_events), ctypes.byref(out))))
    return out.value


_mc_dstep_events = _dstep_events   # the name tests/test_gpu_tm_mc_learn.py calls the step on a 3-D D by


def _steps(N, D, alpha, stride, padding, lasso_method, lasso_iter, lasso_tol):
    """The two halves of an outer iteration on signals of N samples, (code(y, D, x), dstep(y, x, D, XXt, yX, acc_it)):
    the LASSO solver and the dense dictionary step, or for a greedy lasso_method its coder, which writes x entirely,
    and the dictionary step on event lists (the entries ``_entry`` names for D [T, S] or D [T, Ch, S])."""
    if lasso_method not in _GREEDY:
        def code(y, D, x):
            _lasso(y, D, x, alpha, stride, padding, lasso_method, lasso_iter, lasso_tol)

        def dstep(y, x, D, XXt, yX, acc_it):
            return _dstep(y, x, D, XXt, yX, stride, padding, acc_it)
        return code, dstep
    Ch = _channels(D)
    T, S = int(D.shape[0]), int(D.shape[-1])
    n_steps, tol_c, max_events = _greedy_args(lasso_method, alpha, lasso_iter, lasso_tol, T, S, N, stride, padding,
                                              _arrays.np_dtype(D))
    name, flags = _GREEDY[lasso_method]
    entry, dims = _entry(name, T, Ch, S)
    stride = int(stride)

    def code(y, D, x):
        it = ctypes.c_int(0)
        _call(y, entry, y, D, x, y.shape[0], *(dims + (N, stride, _pad_code(padding), n_steps, tol_c) + flags
                                               + (ctypes.byref(it),)))

    def dstep(y, x, D, XXt, yX, acc_it):
        return _dstep_events(y, x, D, XXt, yX, stride, padding, acc_it, max_events)
    return code, dstep


def _normalized_templates(D):
    """D [T, S] or [T, Ch, S] with every template scaled to unit norm (strictly) over all its entries."""
    if D.dim() == 2:
        return normalize.l2_strict(D, axis=-1)
    return normalize.l2_strict(D.reshape(D.shape[0], -1), axis=-1).reshape(D.shape)


def _device_args(y, D, x):
    assertion.assert_dtypes(y=y, D=D, x=x)
    kind = 'torch' if _arrays.is_torch(y) else 'numpy'
    yd = _arrays.to_device(y)
    dev = yd.device.index
    Dd = _arrays.to_device(D, dev).contiguous()
    xd = _arrays.to_device(x, dev, copy=True).contiguous()
    _same_device(yd, Dd, xd)
    return kind, yd.contiguous(), Dd, xd


def _draw_windows(rng, B, N, w, m, C, cw):
    """The rows and starts of one minibatch (minibatch_index((B, N - w), m, rng)).  A window's coefficients
    are x[b, :, start:start + cw] with the SAMPLE start: with stride > 1 (or a padding that makes C < N) such a
    slice can run past the C coefficients of the signal; the reference then fails inside np.stack with a
    ValueError, and so does this (checked before anything is gathered)."""
    rows, starts = minibatch_index((B, N - w), m, rng)
    if cw <= 0 or np.any(np.asarray(starts) + cw > C):
        raise ValueError('a window of %d samples takes %d coefficients from its start; the signal has only %d '
                         'coefficients (stride > 1 minibatch windows can run past them)' % (w, cw, C))
    return rows, starts


def solve_batch(y, D, alpha, x, stride, padding, tol, maxiter,
                lasso_method, lasso_iter, lasso_tol, xp):
    """
    Alternates, on the whole batch y [B, N] (y [B, Ch, N] for multichannel templates D [T, Ch, S], greedy coders):
      x <- the LASSO solution of y = x * D (lasso_iter iterations of lasso_method from the current x), or the code
           of the greedy coder ('omp', 'mp', 'mp_pos': at most lasso_iter events per signal, from zero);
      D <- l2(D + (yX - XXt D) / L), one gradient step on the templates.
    Stops when max|dD| < tol.  D is normalised (strictly) once at entry.  XXt is [T S, T S] whatever the number of
    channels (x is shared by them), yX has the size of D.
    """
    import torch
    code, dstep = _steps(y.shape[-1], D, alpha, stride, padding, lasso_method, lasso_iter, lasso_tol)
    kind, y, D, x = _device_args(y, D, x)
    D = _normalized_templates(D)
    T, S = D.shape[0], D.shape[-1]
    XXt = torch.empty((T * S, T * S), dtype=D.dtype, device=D.device)
    yX = torch.empty((D.numel(),), dtype=D.dtype, device=D.device)
    for it in range(1, maxiter):
        Dprev = D.clone()
        try:
            code(y, D, x)
            diff = dstep(y, x, D, XXt, yX, 0)
            if diff < tol:
                return it, _arrays.to_caller(D, kind), _arrays.to_caller(x, kind)
        except KeyboardInterrupt:
            return it, _arrays.to_caller(Dprev, kind), _arrays.to_caller(x, kind)
    return maxiter, _arrays.to_caller(D, kind), _arrays.to_caller(x, kind)


class Minibatcher(object):
    def __init__(self, array, size_of_minibatch, xp=None):
        """
        Windows of a [batch, n_sequence] or [batch, channels, n_sequence] array: ``self[index]`` for
        index = (rows, starts) stacks array[row, ..., start:start + size_of_minibatch];
        ``self[index] = values`` writes them back one after the other (the last window wins).
        """
        self.array = array
        self.size_of_minibatch = size_of_minibatch
        self.xp = xp

    def _stack(self, parts):
        if _arrays.is_torch(self.array):
            import torch
            return torch.stack(parts, 0)
        return np.stack(parts, axis=0)

    def __getitem__(self, index):
        w = self.size_of_minibatch
        if len(self.array.shape) == 2:
            return self._stack([self.array[i0, i1:i1 + w] for i0, i1 in zip(*index)])
        if len(self.array.shape) == 3:
            return self._stack([self.array[i0, :, i1:i1 + w] for i0, i1 in zip(*index)])

    def __setitem__(self, index, values):
        w = self.size_of_minibatch
        if len(self.array.shape) == 2:
            for (i0, i1), val in zip(index, values):
                self.array[i0, i1:i1 + w] = val
        if len(self.array.shape) == 3:
            for (i0, i1), val in zip(zip(*index), values):
                self.array[i0, :, i1:i1 + w] = val

    @property
    def shape(self):
        return self.array.shape

    @property
    def dtype(self):
        return self.array.dtype


def solve_minibatch(y, D, alpha, x, stride, padding, tol,
                    minibatch, size_of_minibatch, maxiter,
                    lasso_method, lasso_iter, lasso_tol, rng, xp):
    """
    As ``solve_batch`` on ``minibatch`` windows of ``size_of_minibatch`` samples per iteration
    (rows and starts drawn by minibatch_index((B, N - size_of_minibatch), minibatch, rng)); each
    window's coefficients are the slice x[b, :, start:start + _coef_size(S, size_of_minibatch)] and
    are written back in draw order (so with stride > 1 a window can run past the coefficients: ValueError,
    as in the reference, see _draw_windows).  The statistics are accumulated as XXt_sum += XXt / it,
    yX_sum += yX / it (it = 1, 2, ...).  Returns the full x.  A greedy coder codes every window from zero, with at
    most lasso_iter events per window.  Multichannel templates D [T, Ch, S]: the windows are yw [m, Ch, w].
    """
    import torch
    code, dstep = _steps(int(size_of_minibatch), D, alpha, stride, padding, lasso_method, lasso_iter, lasso_tol)
    kind, y, D, x = _device_args(y, D, x)
    D = _normalized_templates(D)
    B, N = y.shape[0], y.shape[-1]
    T, S = D.shape[0], D.shape[-1]
    C = x.shape[-1]
    w = int(size_of_minibatch)
    cw = _coef_size(S, w, stride=stride, padding=padding)
    m = int(minibatch)
    yX_sum = torch.zeros((D.numel(),), dtype=D.dtype, device=D.device)
    XXt_sum = torch.zeros((T * S, T * S), dtype=D.dtype, device=D.device)
    yw = torch.empty((m,) + tuple(y.shape[1:-1]) + (w,), dtype=y.dtype, device=y.device)
    xw = torch.empty((m, T, cw), dtype=y.dtype, device=y.device)
    gather, dims = _entry('gather_windows', T, _channels(D), S)
    for it in range(1, maxiter):
        Dprev = D.clone()
        try:
            rows, starts = _draw_windows(rng, B, N, w, m, C, cw)
            ib = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(y.device)
            inn = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int64)).to(y.device)
            _call(y, gather, y, x, ib, inn, m, B, *(dims + (N, w, stride, _pad_code(padding), yw, xw)))
            code(yw, D, xw)
            _call(y, 'scatter_windows', xw, x, ib, inn, m,
                  B, T, S, N, w, stride, _pad_code(padding))
            diff = dstep(yw, xw, D, XXt_sum, yX_sum, it)
            if diff < tol:
                return it, _arrays.to_caller(D, kind), _arrays.to_caller(x, kind)
        except KeyboardInterrupt:
            return it, _arrays.to_caller(Dprev, kind), _arrays.to_caller(x, kind)
    return maxiter, _arrays.to_caller(D, kind), _arrays.to_caller(x, kind)

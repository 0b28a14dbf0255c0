"""Non-negative matrix factorisation -- drop-in for ``decomp.nmf`` on MI355X.

Same entry point, argument meaning, return convention and error behaviour as the
reference's decomp/nmf.py:16-113: the full-batch multiplicative update
(``minibatch=None, method='mu'``) and the stochastic minibatch variants
(decomp_amd/nmf_minibatch.py).  Beyond the reference: ``method='hals'`` (l2, no mask,
full batch), exact block coordinate descent in libdecomp_hip.so (``dcp_nmf_hals_*``,
decomp_amd/csrc/nmf_hals.hpp) and ``method='em-hals'`` (the same with missing or weighted entries,
``dcp_nmf_emhals_*``).  The full-batch MU iteration itself
(decomp/nmf_methods/batch_mu.py:8-26 with the update rules of
decomp/nmf_methods/grads.py:77-160) runs in libdecomp_hip.so: see
include/decomp_hip.h ``dcp_nmf_mu_*`` and decomp_amd/csrc/nmf_impl.hpp.  Also beyond the reference: an L1/L2
penalty on the codes (``l1_penalty`` / ``l2_penalty``, ``dcp_set_nmf_penalty``) for both full-batch methods.
"""
import ctypes
import math
import numbers

import numpy as np

from . import _arrays, _hip
from ._arrays import get_array_module
from .utils import assertion

BATCH_METHODS = ['mu']
MINIBATCH_METHODS = [
    'asg-mu', 'gsg-mu', 'asag-mu', 'gsag-mu',  # Serizel et al.
    'svrmu', 'svrmu-acc',                      # Kasai et al.
    ]
_JITTER = 1.0e-15


def _likelihood_spec(likelihood):
    """grads.py:7-14: (code, beta).  code is the kernel code (an int) of a built-in likelihood, or the
    user-supplied ``Likelihood`` instance itself (grads.py:12-13), which then runs through the host loop
    ``_run_mu_user`` / ``nmf_minibatch._UserKernels``.  beta is the exponent that goes with DCP_LIK_BETA
    ('is' / 'itakura-saito' = 0, or a ``BetaDivergence``'s own), None for every other code."""
    from .nmf_methods import grads
    if isinstance(likelihood, str):
        if likelihood in ('l2', 'gaussian'):
            return _hip.LIK_L2, None
        if likelihood in ('kl', 'poisson'):
            return _hip.LIK_KL, None
        if likelihood in ('is', 'itakura-saito'):
            return _hip.LIK_BETA, 0.0
    elif isinstance(likelihood, grads.Likelihood):
        spec = grads.fused_spec(likelihood)
        return (likelihood, None) if spec is None else spec
    raise NotImplementedError('Likelihood {} is not implemented for nmf'.format(likelihood))


def _likelihood_code(likelihood):
    """The code of ``_likelihood_spec`` alone."""
    return _likelihood_spec(likelihood)[0]


def _fused_lik(lik, beta):
    """What the minibatch loops take as ``lik``: the code, or (DCP_LIK_BETA, beta)."""
    return (lik, beta) if isinstance(lik, int) and lik == _hip.LIK_BETA else lik


def _beta_of(likelihood):
    """beta of a beta-divergence likelihood ('is' / 'itakura-saito', any ``BetaDivergence``), else None."""
    from .nmf_methods import grads
    if isinstance(likelihood, str):
        return 0.0 if likelihood in ('is', 'itakura-saito') else None
    if isinstance(likelihood, grads.BetaDivergence):
        return likelihood.beta
    return None


def _check_beta_data(likelihood, y, mask):
    """Data a beta divergence is defined on: beta < 2 needs y >= 0 (as 'kl', nmf.py:67-68), beta <= 0 also
    y > 0 wherever mask != 0 (a missing entry is zero by the reference's convention, nmf.py:48).  NumPy arrays
    are checked on the host, torch tensors on their device.  Raises AssertionError."""
    beta = _beta_of(likelihood)
    if beta is None or beta >= 2.0:
        return
    assertion.assert_nonnegative_host_or_device(y)
    if beta <= 0.0:
        assertion.assert_positive_where(y, mask)


def _check_penalty(l1_penalty, l2_penalty):
    """(l1, l2) as floats.  ValueError for a penalty that is not a finite real number >= 0."""
    out = []
    for name, v in (('l1_penalty', l1_penalty), ('l2_penalty', l2_penalty)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Real):
            raise ValueError('%s must be a real number, not %r' % (name, v))
        v = float(v)
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError('%s must be finite and >= 0, not %r' % (name, v))
        out.append(v)
    return tuple(out)


def _check_penalty_scope(penalty, minibatch, method, likelihood):
    """What the penalty on the codes covers: the full-batch MU loop with a fused likelihood and HALS.  Raises
    NotImplementedError for a non-zero penalty with a minibatch method or with a user ``Likelihood`` whose update
    rule runs on the host (``_run_mu_user``).  Zero penalties pass everywhere."""
    if penalty == (0.0, 0.0):
        return
    if minibatch is not None:
        raise NotImplementedError('l1_penalty / l2_penalty are not implemented for the minibatch NMF methods')
    if method == 'mu' and not isinstance(_likelihood_spec(likelihood)[0], int):
        raise NotImplementedError('l1_penalty / l2_penalty are not implemented for a likelihood with its own '
                                  'update rule')


def _set_penalty(h, penalty):
    """Hand (l1, l2) to the handle right before a call of the MU / HALS loops or split steps
    (``dcp_set_nmf_penalty``); (0, 0) included, so that no earlier call's penalty is read."""
    l1, l2 = penalty
    _hip.check(h, _hip.load().dcp_set_nmf_penalty(h, float(l1), float(l2)), 'dcp_set_nmf_penalty')


class _OnesLike(object):
    """Stand-in for the default x = ones((N, K)) during validation, so that the default
    is materialised directly in device memory."""
    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), dtype


def solve(y, D, x=None, tol=1.0e-3, minibatch=None, maxiter=1000, method='mu',
          likelihood='l2', mask=None, random_seed=None, l1_penalty=0.0, l2_penalty=0.0, **kwargs):
    """
    Non-negative matrix factorisation  argmin_{x, D} |y - xD|^2,  x >= 0, D >= 0,
    |D_j| = 1, by multiplicative updates (method='mu'), or, for the l2 likelihood without a
    mask, by HALS (method='hals': exact block coordinate descent on the columns of x and the
    atoms of D, then the atoms rescaled to unit norm with x rescaled so that xD is unchanged),
    or, for the l2 likelihood with missing or weighted entries, by method='em-hals'.

    method='em-hals' minimises  1/2 sum mask o (y - xD)^2  (+ the penalty below) for weights mask in [0, 1]
    (anything else, NaN included: ValueError).  Each iteration fills the unobserved part of y in from the
    current model,  y' = mask o y + (1 - mask) o (xD),  and runs one HALS iteration on y' (EM for weighted
    low-rank factorisation, Srebro & Jaakkola 2003, with HALS as the M step).  1/2 |y' - xD|^2 majorises the
    masked objective and touches it at the current iterate, so no iteration can increase the objective; the
    smaller the observed fraction, the slower the convergence (the imputed part pulls every step towards the
    previous iterate).  Defaults, return convention and penalties as for 'hals'; mask=None runs plain HALS.
    Full batch and l2 only (NotImplementedError otherwise).

    l1_penalty, l2_penalty (lambda1, lambda2 >= 0, default 0): a penalty on the codes.  The objective
    becomes  loss(y, xD) + lambda1 sum(x) + lambda2/2 |x|^2,  loss = 1/2 |M o (y - xD)|^2 for 'l2' (M the
    mask, or 1), sum M o d(y | xD) for 'kl' and the beta divergences; no 1/n_samples scaling and no penalty
    on D, whose rows stay unit norm.  So for a fixed D and lambda2 = 0 the x problem is exactly
    ``lasso.solve(y, D, alpha=lambda1 / n_channels, method='cd_pos')`` (the lasso scales alpha by
    n_channels).  MU divides by  grad_neg + lambda1 + lambda2 x  in its x update; HALS takes the exact
    coordinate minimiser of the penalised objective in its x sweep.  Both 0 runs exactly the unpenalised
    solver.  Non-zero penalties are not implemented for the minibatch methods or a likelihood with its own
    update rule (NotImplementedError).

    y: [n_samples, n_channels], x: [n_samples, n_features], D: [n_features, n_channels],
    mask (optional): [n_samples, n_channels], 0 marks a missing entry; float32 or
    float64, all arrays of the same dtype.  NumPy arrays (copied to the GPU, results
    returned as NumPy) or torch CUDA tensors (results returned as torch tensors).
    Out of core (nmf.py:93-103): with a minibatch method, a torch CUDA ``D`` and NumPy
    ``y`` / ``x`` / ``mask``, the NumPy arrays stay in pinned host memory and are streamed
    through the GPU minibatch by minibatch (utils.data.AsyncMinibatchData); ``x`` then
    comes back as a NumPy array.

    Returns (it, D, x) exactly as the reference: ``it`` is the iteration at which
    max|D - D_new| < tol was met, or ``maxiter`` when it never was.
    """
    penalty = _check_penalty(l1_penalty, l2_penalty)
    if method == 'em-hals':
        _check_emhals_scope(likelihood, minibatch, kwargs)
    _check_penalty_scope(penalty, minibatch, method, likelihood)
    kind = get_array_module(D)
    x_given = x
    if x is None:                                                     # nmf.py:53-54
        x = _OnesLike((y.shape[0], D.shape[0]), _arrays.np_dtype(y))

    assertion.assert_dtypes(y=y, D=D, x=x)                            # nmf.py:56-63
    assertion.assert_dtypes(y=y, D=D, x=x, mask=mask, dtypes='f')
    assertion.assert_shapes('x', x, 'D', D, axes=1)
    assertion.assert_shapes('y', y, 'D', D, axes=[-1])
    assertion.assert_shapes('y', y, 'mask', mask)
    assertion.assert_ndim('y', y, 2)
    assertion.assert_ndim('D', D, 2)
    assertion.assert_ndim('x', x, 2)

    if minibatch is None or kind == 'numpy':
        get_array_module(D, x_given)
    # out of core (nmf.py:93-103): device D, host data, minibatch method
    streamed = (minibatch is not None and kind == 'torch' and
                any(a is not None and not _arrays.is_torch(a) for a in (y, x_given, mask)))

    # ---- from here on everything lives on the GPU ----
    import torch
    D_dev = _arrays.to_device(D, copy=True)           # normalised in place below
    dev = D_dev.device.index
    assertion.assert_nonnegative(D_dev)                               # nmf.py:64-65
    _check_beta_data(likelihood, y, mask)
    if streamed:
        return _solve_streamed(y, D_dev, x_given, tol, minibatch, maxiter, method, likelihood,
                               mask, random_seed, kwargs)
    if x_given is None:
        x_dev = torch.ones(x.shape, dtype=D_dev.dtype, device=D_dev.device)
    else:
        x_dev = _arrays.to_device(x_given, dev, copy=True)   # updated in place
    assertion.assert_nonnegative(x_dev)
    lik = None
    if isinstance(likelihood, str) and likelihood in ['kl']:          # nmf.py:67-68
        y_dev = _arrays.to_device(y, dev)
        assertion.assert_nonnegative(y_dev)
    else:
        y_dev = None

    _arrays.l2_normalize_(D_dev, strict=True)                         # nmf.py:70

    if minibatch is None:
        get_array_module(y, D, x_given)                               # nmf.py:75
        if method == 'mu':
            if kwargs:  # batch_mu.solve accepts no extra keyword (nmf.py:77, batch_mu.py:8)
                raise TypeError('solve() got an unexpected keyword argument %r'
                                % sorted(kwargs)[0])
            lik, beta = _likelihood_spec(likelihood)
            get_array_module(y, mask)
            if not isinstance(lik, int):
                it, D_dev, x_dev = _run_mu_user(y, mask, x_dev, D_dev, lik, tol, maxiter, kind)
                return it, _arrays.to_caller(D_dev, kind), _arrays.to_caller(x_dev, kind)
            if y_dev is None:
                y_dev = _arrays.to_device(y, dev)
            m_dev = _arrays.to_device(mask, dev)
            it = _run_mu(y_dev, m_dev, x_dev, D_dev, lik, tol, maxiter, beta=beta, penalty=penalty)
            return it, _arrays.to_caller(D_dev, kind), _arrays.to_caller(x_dev, kind)
        if method == 'hals':
            if kwargs:
                raise TypeError('solve() got an unexpected keyword argument %r'
                                % sorted(kwargs)[0])
            _check_hals_scope(likelihood, mask)
            if y_dev is None:
                y_dev = _arrays.to_device(y, dev)
            it = _run_hals(y_dev, x_dev, D_dev, tol, maxiter, penalty=penalty)
            return it, _arrays.to_caller(D_dev, kind), _arrays.to_caller(x_dev, kind)
        if method == 'em-hals':
            get_array_module(y, mask)
            if y_dev is None:
                y_dev = _arrays.to_device(y, dev)
            m_dev = _arrays.to_device(mask, dev)
            _check_weights(m_dev)
            it = _run_emhals(y_dev, m_dev, x_dev, D_dev, tol, maxiter, penalty=penalty)
            return it, _arrays.to_caller(D_dev, kind), _arrays.to_caller(x_dev, kind)
        raise NotImplementedError('Batch-NMF with {} algorithm is not yet '
                                  'implemented.'.format(method))
    # ---- stochastic variants: minibatch containers on the GPU (nmf.py:82-111) ----
    from .utils.data import MinibatchData, NoneIterator
    from . import nmf_minibatch
    if method not in MINIBATCH_METHODS:
        raise NotImplementedError('NMF with {} algorithm is not yet '
                                  'implemented.'.format(method))
    get_array_module(y, D, x_given, mask)
    lik = _fused_lik(*_likelihood_spec(likelihood))
    if y_dev is None:
        y_dev = _arrays.to_device(y, dev)
    ybat = MinibatchData(y_dev, minibatch)
    xbat = MinibatchData(x_dev, minibatch)
    mbat = NoneIterator() if mask is None else MinibatchData(_arrays.to_device(mask, dev), minibatch)
    rng = np.random.RandomState(random_seed)
    if method in ['asg-mu', 'gsg-mu', 'asag-mu', 'gsag-mu']:
        it, Dout, xout = nmf_minibatch.solve_serizel(ybat, D_dev, xbat, tol, minibatch, maxiter,
                                                     method, lik, mbat, rng, kind=kind, **kwargs)
    else:
        it, Dout, xout = nmf_minibatch.solve_kasai(ybat, D_dev, xbat, tol, minibatch, maxiter,
                                                   method, lik, mbat, rng, kind=kind, **kwargs)
    return it, _arrays.to_caller(Dout, kind), _arrays.to_caller(xout, kind)


def _solve_streamed(y, D_dev, x_given, tol, minibatch, maxiter, method, likelihood, mask,
                    random_seed, kwargs):
    """nmf.py:93-111: every array that is a NumPy array stays on the host and is streamed
    (x with write-back); device arrays use the in-core container.  Returns (it, D, x) with
    x a NumPy array when it was streamed."""
    import torch
    from .utils.data import MinibatchData, AsyncMinibatchData, NoneIterator
    from . import nmf_minibatch
    if method not in MINIBATCH_METHODS:
        raise NotImplementedError('NMF with {} algorithm is not yet '
                                  'implemented.'.format(method))
    dev = D_dev.device.index

    def dataset(a, needs_update):
        if a is None:
            return NoneIterator()
        if _arrays.is_torch(a):
            t = _arrays.to_device(a, dev, copy=needs_update)
            if needs_update:
                assertion.assert_nonnegative(t)                       # nmf.py:65
            return MinibatchData(t, minibatch)
        if needs_update or (isinstance(likelihood, str) and likelihood in ['kl']):
            assertion.assert_nonnegative_host_or_device(a)            # nmf.py:65,67-68
        return AsyncMinibatchData(a, minibatch, needs_update=needs_update, device=dev)

    if x_given is None:                                               # nmf.py:53-54: ones in D's module
        x_given = torch.ones((y.shape[0], D_dev.shape[0]), dtype=D_dev.dtype, device=D_dev.device)
    if _arrays.is_torch(y) and isinstance(likelihood, str) and likelihood in ['kl']:
        assertion.assert_nonnegative(_arrays.to_device(y, dev))
    _arrays.l2_normalize_(D_dev, strict=True)                         # nmf.py:70
    lik = _fused_lik(*_likelihood_spec(likelihood))
    xbat = dataset(x_given, True)
    ybat = dataset(y, False)
    mbat = dataset(mask, False)
    rng = np.random.RandomState(random_seed)
    if method in ['asg-mu', 'gsg-mu', 'asag-mu', 'gsag-mu']:
        it, Dout, xout = nmf_minibatch.solve_serizel(ybat, D_dev, xbat, tol, minibatch, maxiter,
                                                     method, lik, mbat, rng, **kwargs)
    else:
        it, Dout, xout = nmf_minibatch.solve_kasai(ybat, D_dev, xbat, tol, minibatch, maxiter,
                                                   method, lik, mbat, rng, **kwargs)
    return it, Dout, xout


def _loop_call(method, sharded, y, mask, x, D, lik, beta, penalty, tol, maxiter, resid_trace=None):
    """One full-batch solver loop inside the library, ``dcp_nmf_{mu,hals,emhals}[_sharded]_*``, on device arrays; x
    and D are updated in place.  Returns it.  The hals entries take neither mask nor likelihood (``lik`` None), the
    emhals entries a mask (or None) but no likelihood, the
    sharded ones no residual trace.  ``beta`` goes with lik == DCP_LIK_BETA; ``penalty`` is (l1, l2) on the codes,
    set on the handle for this call alone."""
    from .nmf_methods.grads import set_beta
    lib, h = _arrays.lib_handle(D)
    name = 'dcp_nmf_%s_%s%s' % (method, 'sharded_' if sharded else '', _arrays.suffix(D))
    ctype = ctypes.c_float if name.endswith('f32') else ctypes.c_double
    it = ctypes.c_int(0)
    last = ctype(0)
    mu = method == 'mu'
    masked = mu or method == 'emhals'
    args = [h, _arrays.ptr(y)] + ([_arrays.ptr(mask)] if masked else []) + [_arrays.ptr(x), _arrays.ptr(D)]
    args += list(y.shape) + [D.shape[0]] + ([lik] if mu else [])
    args += [ctype(tol), int(maxiter), ctypes.byref(it), ctypes.byref(last)]
    trace = None
    if not sharded:
        if resid_trace is not None:
            trace = (ctype * max(int(maxiter), 1))()
        args.append(trace)
    set_beta(h, lik, beta)
    _set_penalty(h, penalty)
    try:
        rc = getattr(lib, name)(*args)
    finally:
        if penalty != (0.0, 0.0):
            _set_penalty(h, (0.0, 0.0))
    _hip.check(h, rc, name)
    if trace is not None:
        n_done = it.value if it.value < maxiter else maxiter - 1
        resid_trace.extend(float(trace[i]) for i in range(max(n_done, 0)))
    return it.value


def _run_mu(y, mask, x, D, lik, tol, maxiter, resid_trace=None, beta=None, penalty=(0.0, 0.0)):
    """batch_mu.solve on device arrays; x and D are updated in place.  Returns it.  ``beta`` goes with
    lik == DCP_LIK_BETA; ``penalty`` is (l1, l2) on the codes."""
    return _loop_call('mu', False, y, mask, x, D, lik, beta, penalty, tol, maxiter, resid_trace)


def _check_hals_scope(likelihood, mask):
    """What method='hals' covers: the squared loss without a mask.  Raises NotImplementedError otherwise."""
    if mask is not None:
        raise NotImplementedError('NMF with the hals algorithm does not support a mask '
                                  '(use method=\'mu\')')
    if not (isinstance(likelihood, str) and likelihood in ('l2', 'gaussian')):
        raise NotImplementedError('NMF with the hals algorithm supports only the l2 likelihood, '
                                  'not {} (use method=\'mu\')'.format(likelihood))


def _run_hals(y, x, D, tol, maxiter, resid_trace=None, penalty=(0.0, 0.0)):
    """HALS (exact block coordinate descent) on device arrays, D l2_strict normalised; x and D are updated
    in place.  Same stop rule and return convention as ``_run_mu``; ``penalty`` is (l1, l2) on the codes.
    Returns it."""
    return _loop_call('hals', False, y, None, x, D, None, None, penalty, tol, maxiter, resid_trace)


def _check_emhals_scope(likelihood, minibatch, kwargs):
    """What method='em-hals' covers: the squared loss, full batch, no extra keyword.  Runs before any GPU call."""
    if kwargs:
        raise TypeError('solve() got an unexpected keyword argument %r' % sorted(kwargs)[0])
    if minibatch is not None:
        raise NotImplementedError('NMF with the em-hals algorithm is a full-batch method (minibatch=None)')
    if not (isinstance(likelihood, str) and likelihood in ('l2', 'gaussian')):
        raise NotImplementedError('NMF with the em-hals algorithm supports only the l2 likelihood, '
                                  'not {} (use method=\'mu\')'.format(likelihood))


def _check_weights(mask):
    """The weights of em-hals must lie in [0, 1] (one pass on the device, once per solve; a NaN fails both
    comparisons).  None passes."""
    if mask is not None and not bool(((mask >= 0) & (mask <= 1)).all()):
        raise ValueError('mask must lie in [0, 1] for the em-hals algorithm')


def _run_emhals(y, mask, x, D, tol, maxiter, resid_trace=None, penalty=(0.0, 0.0)):
    """em-hals on device arrays (``dcp_nmf_emhals_*``): every iteration imputes the entries the weights ``mask``
    in [0, 1] leave out from the current x D, then runs one HALS iteration on the result.  ``mask`` None runs
    plain HALS.  Conventions of ``_run_hals``; ``resid_trace`` collects |(y - x D) o mask|_F.  Returns it."""
    return _loop_call('emhals', False, y, mask, x, D, None, None, penalty, tol, maxiter, resid_trace)


def _run_mu_user(y, mask, x_dev, D_dev, lik, tol, maxiter, kind):
    """batch_mu.py:8-26 with a user-supplied Likelihood (grads.py:12-13).  The plugin's
    ``update_x`` / ``update_d`` see arrays of the caller's kind (NumPy or torch CUDA); the
    inherited update rule, ``l2_strict`` and the stop test run on the GPU
    (``dcp_mu_quotient_*``, ``dcp_l2_normalize_diff_*``).  Returns (it, D, x) as device tensors."""
    import torch
    dev = D_dev.device.index
    sfx = _arrays.suffix(D_dev)
    K, F = D_dev.shape
    md = ctypes.c_double(0.0)

    def user(t):
        return _arrays.to_caller(t, kind)

    y_u = y if kind == 'numpy' else _arrays.to_device(y, dev)
    m_u = mask if (mask is None or kind == 'numpy') else _arrays.to_device(mask, dev)
    x, D = x_dev, D_dev
    D_new = torch.empty_like(D)
    for it in range(1, maxiter):                                       # batch_mu.py:16
        x = _arrays.to_device(lik.update_x(y_u, user(x), user(D), m_u), dev)
        U = _arrays.to_device(lik.update_d(y_u, user(x), user(D), m_u), dev)
        if U.shape != D.shape or U.dtype != D.dtype:
            raise ValueError('update_d must return an array like D: %s %s' % (tuple(U.shape), U.dtype))
        lib, h = _arrays.lib_handle(D)
        fn = getattr(lib, 'dcp_l2_normalize_diff_' + sfx)
        _hip.check(h, fn(h, _arrays.ptr(U), _arrays.ptr(D), _arrays.ptr(D_new), K, F, 1,
                         ctypes.byref(md)), 'dcp_l2_normalize_diff')
        if md.value < tol:                                             # batch_mu.py:22
            return it, D_new, x
        D, D_new = D_new, D
    return maxiter, D, x

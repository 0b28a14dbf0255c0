"""GPU: the six stochastic NMF methods end to end against oracle.nmf_minibatch (float64 NumPy on float64 copies of
the same inputs), at a shape of several tiles whose epochs leave a ragged tail: N = 2100, F = 1030, K = 70, 256-row
minibatches, i.e. 8 minibatches per epoch and 52 rows left out of each.

Inputs are float32-representable, so the float32 and float64 runs start from the same values and one oracle run
serves both.  Metric: max-abs error over max-abs value, for D and for x.
  float64: 1e-9.
  float32: every D update and every x update is a multiplicative step whose parts are fp32 products of positive
  terms; each step is within delta = 6 P + 4 u of its float64 value, relative, with P = 2 sqrt(d) u for the deepest
  reduction d = max(F, K, minibatch) (the per-update bound of test_gpu_nmf_grads.py), and the errors of successive
  steps add up.  A run of n D updates, each after an x update, stays within 2 n delta: 2 epochs of 8 updates give
  8.1e-4 here."""
import numpy as np
import pytest

from oracle import nmf_minibatch as omb

pytestmark = pytest.mark.gpu

METHODS = ['asg-mu', 'gsg-mu', 'asag-mu', 'gsag-mu', 'svrmu', 'svrmu-acc']
N, F, K, MB = 2100, 1030, 70, 256
U32 = 2.0 ** -24


def _f32_bound(n_updates, depth):
    delta = 6 * 2.0 * np.sqrt(depth) * U32 + 4 * U32
    return 2 * n_updates * delta


def _err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, float(np.max(np.abs(b)))))


def _data(n, f, k, masked, seed):
    """Strictly positive y (as the beta checks require where the mask is non-zero), D0 and a 0/1 mask."""
    rng = np.random.RandomState(seed)
    Dt = rng.uniform(0.1, 1.0, (k, f))
    xt = rng.uniform(0.1, 1.0, (n, k))
    y = (xt.dot(Dt) * rng.uniform(0.7, 1.3, (n, f))).astype(np.float32).astype(np.float64)
    D0 = (Dt * rng.uniform(0.5, 1.5, (k, f))).astype(np.float32).astype(np.float64)
    mask = (rng.uniform(size=(n, f)) >= 0.3).astype(np.float64) if masked else None
    return y, D0, mask


def _oracle(y, D0, mask, lik, method, maxiter=3, tol=0.0, minibatch=MB, trace=None, **kw):
    return omb.solve(y.copy(), D0.copy(), tol=tol, minibatch=minibatch, maxiter=maxiter, method=method,
                     likelihood=lik, mask=None if mask is None else mask.copy(), random_seed=0, trace=trace, **kw)


def _gpu(y, D0, mask, lik, method, dt, maxiter=3, tol=0.0, minibatch=MB, **kw):
    import decomp_amd
    return decomp_amd.nmf.solve(y.astype(dt), D0.astype(dt), x=None, tol=tol, minibatch=minibatch,
                                maxiter=maxiter, method=method, likelihood=lik,
                                mask=None if mask is None else mask.astype(dt), random_seed=0, **kw)


def _d_updates(method, n, mb, epochs):
    per_epoch = 1 if method == 'gsag-mu' else n // mb
    return per_epoch * epochs


def _check(got, ref, dt, method, what, n=N, mb=MB, epochs=2, depth=max(F, K, MB)):
    it, D, x = got
    it_r, D_r, x_r = ref
    assert it == it_r, (what, it, it_r)
    assert D.dtype == np.dtype(dt) and x.dtype == np.dtype(dt)
    tol = 1e-9 if dt == np.float64 else _f32_bound(_d_updates(method, n, mb, epochs), depth)
    assert tol < 1e-3
    eD, ex = _err(D, D_r), _err(x, x_r)
    assert eD <= tol and ex <= tol, (what, eD, ex, tol)


_ORACLE = {}


def _cached_oracle(key, *args, **kw):
    if key not in _ORACLE:
        _ORACLE[key] = _oracle(*args, **kw)
    return _ORACLE[key]


@pytest.mark.parametrize('dt', [np.float64, np.float32], ids=['float64', 'float32'])
@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('lik', ['l2', 'kl'])
@pytest.mark.parametrize('method', METHODS)
def test_main_grid(method, lik, masked, dt):
    y, D0, mask = _data(N, F, K, masked, seed=1)
    ref = _cached_oracle(('main', method, lik, masked), y, D0, mask, lik, method)
    _check(_gpu(y, D0, mask, lik, method, dt), ref, dt, method, (method, lik, masked))


@pytest.mark.parametrize('dt', [np.float64, np.float32], ids=['float64', 'float32'])
@pytest.mark.parametrize('lik', ['is', 'beta0.5'])
@pytest.mark.parametrize('method', METHODS)
def test_beta_divergence(method, lik, dt):
    """'is' (beta = 0) and BetaDivergence(0.5), the 'is' runs with a mask."""
    from decomp_amd.nmf_methods.grads import BetaDivergence
    masked = lik == 'is'
    y, D0, mask = _data(N, F, K, masked, seed=2)
    spec, obj = ('is', 'is') if lik == 'is' else (0.5, BetaDivergence(0.5))
    ref = _cached_oracle(('beta', method, lik), y, D0, mask, spec, method)
    _check(_gpu(y, D0, mask, obj, method, dt), ref, dt, method, (method, lik))


def test_svrmu_acc_inner_count():
    """kasai.py:24-28 with F, K = D.shape as written: 2 x updates per minibatch at N = 240, F = 2000, K = 8 (and 10
    with beta = 2.0), against 1 at the fixtures' shape."""
    assert omb.svrmu_acc_iters(8, 2000, 240) == 2
    assert omb.svrmu_acc_iters(8, 2000, 240, beta=2.0) == 10
    assert omb.svrmu_acc_iters(3, 20, 1001) == 1
    y, D0, mask = _data(240, 2000, 8, True, seed=3)
    for dt in (np.float64, np.float32):
        for kw in ({}, {'beta': 2.0}):
            ref = _cached_oracle(('acc', str(kw)), y, D0, mask, 'l2', 'svrmu-acc', minibatch=40, **kw)
            got = _gpu(y, D0, mask, 'l2', 'svrmu-acc', dt, minibatch=40, **kw)
            _check(got, ref, dt, 'svrmu-acc', kw, n=240, mb=40, depth=2000)


@pytest.mark.parametrize('dt', [np.float64, np.float32], ids=['float64', 'float32'])
@pytest.mark.parametrize('method,kw', [('svrmu', {'alpha': 0.5}), ('svrmu-acc', {'beta': 2.0}),
                                       ('asag-mu', {'forget_rate': 0.2}), ('gsag-mu', {'forget_rate': 0.2})],
                         ids=['svrmu-alpha0.5', 'svrmu-acc-beta2', 'asag-forget0.2', 'gsag-forget0.2'])
def test_non_default_keywords(method, kw, dt):
    y, D0, mask = _data(N, F, K, False, seed=4)
    ref = _cached_oracle(('kw', method, str(kw)), y, D0, mask, 'l2', method, **kw)
    default = _cached_oracle(('kw', method, '{}'), y, D0, mask, 'l2', method)
    assert _err(ref[1], default[1]) > 1e-6        # the keyword changes the result
    _check(_gpu(y, D0, mask, 'l2', method, dt, **kw), ref, dt, method, (method, kw))


def test_out_of_core_matches_oracle():
    """Device D, host y / mask: the minibatches are streamed (utils.data.AsyncMinibatchData)."""
    import torch
    import decomp_amd
    y, D0, mask = _data(N, F, K, True, seed=1)
    for method in METHODS:
        ref = _cached_oracle(('main', method, 'l2', True), y, D0, mask, 'l2', method)
        it, D, x = decomp_amd.nmf.solve(y, torch.from_numpy(D0).cuda(), tol=0.0, minibatch=MB, maxiter=3,
                                        method=method, likelihood='l2', mask=mask, random_seed=0)
        x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
        _check((it, D.cpu().numpy(), x), ref, np.float64, method, ('streamed', method))


@pytest.mark.parametrize('case', [(8292, 2048, 256, 4096, True), (2100, 1024, 128, 1024, False)],
                         ids=['x6_4096x2048x256', 'fp32_1024x1024x128'])
def test_float32_l2_both_product_modes(case):
    """Float32 l2 without a mask in both product modes (dcp_set_f32_product_mode).  4096-row minibatches with
    F = 2048, K = 256 put the x update and the statistics product on the split-bf16 core (test_gpu_nmf_grads.py
    'bf16x6'), so the two modes' results differ; 1024-row minibatches with F = 1024, K = 128 have too few tiles
    for it and give bitwise equal results.  Both modes within the float32 bound."""
    from test_gpu_nmf_grads import _Mode
    n, f, k, mb, on_core = case
    y, D0, _ = _data(n, f, k, False, seed=5)
    ref = _cached_oracle(('modes', n), y, D0, None, 'l2', 'asg-mu', minibatch=mb)
    outs = []
    for mode in (0, 1):
        with _Mode(mode):
            got = _gpu(y, D0, None, 'l2', 'asg-mu', np.float32, minibatch=mb)
        _check(got, ref, np.float32, 'asg-mu', ('mode', mode), n=n, mb=mb, depth=max(f, k, mb))
        outs.append(got)
    same = np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    assert same == (not on_core)


@pytest.mark.parametrize('method', ['asg-mu', 'svrmu'])
def test_stop_fires_mid_epoch(method):
    """tol between two consecutive max|dD| values of the oracle's trace, at an update in the middle of the second
    epoch: the same it as the oracle, D from BEFORE the converged step (serizel.py:58-59, kasai.py:79-80), and the
    rows that no minibatch reached before the stop keep x = 1."""
    y, D0, mask = _data(N, F, K, False, seed=6)
    trace = []
    _oracle(y, D0, mask, 'l2', method, maxiter=4, trace=trace)
    n_mb = N // MB
    assert len(trace) == 3 * n_mb
    # the first update after epoch 1, neither first nor last of its epoch, that sets a new running minimum (by a
    # margin far above float64 rounding)
    i = [j for j in range(n_mb, 3 * n_mb) if 0 < j % n_mb < n_mb - 1 and trace[j] < min(trace[:j]) * (1 - 1e-4)][0]
    tol = 0.5 * (trace[i] + min(trace[:i]))
    ref = _oracle(y, D0, mask, 'l2', method, maxiter=4, tol=tol)
    assert ref[0] == i // n_mb + 1
    it, D, x = _gpu(y, D0, mask, 'l2', method, np.float64, maxiter=4, tol=tol)
    assert it == ref[0]
    assert _err(D, ref[1]) <= 1e-9 and _err(x, ref[2]) <= 1e-9
    # the returned D is the one before the converged step, which would move it by trace[i] >> 1e-9
    assert trace[i] > 1e-6
    unvisited = np.all(ref[2] == 1.0, axis=1)
    assert unvisited.any()
    assert np.all(x[unvisited] == 1.0) and not np.any(np.all(x[~unvisited] == 1.0, axis=1))

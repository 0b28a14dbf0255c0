"""CPU: the L1/L2 penalty on the NMF codes (nmf.solve / nmf_solve_sharded l1_penalty, l2_penalty) -- argument
checks made before any GPU call, and the float64 restatement of the penalised updates (penalty_ref.py) pinned to
oracle/nmf.py (itself pinned to the reference's golden vectors) at zero penalty."""
import numpy as np
import pytest

import penalty_ref


def _problem(dtype=np.float32):
    rng = np.random.RandomState(0)
    return np.abs(rng.randn(40, 12)).astype(dtype), np.abs(rng.randn(3, 12)).astype(dtype)


@pytest.fixture
def no_gpu(monkeypatch):
    from decomp_amd import _arrays, _hip

    def boom(*a, **k):
        raise AssertionError('a GPU call was made before the argument check')
    monkeypatch.setattr(_arrays, 'to_device', boom)
    monkeypatch.setattr(_hip, 'load', boom)


BAD = [-1.0, -1e-300, float('nan'), float('inf'), -float('inf'), '0.1', None, 1j, [0.1], True]


def _solvers():
    from decomp_amd import nmf, sharded
    return [('solve_mu', lambda y, D, **k: nmf.solve(y, D, **k)),
            ('solve_hals', lambda y, D, **k: nmf.solve(y, D, method='hals', **k)),
            ('sharded_mu', lambda y, D, **k: sharded.nmf_solve_sharded(y, D, **k)),
            ('sharded_hals', lambda y, D, **k: sharded.nmf_solve_sharded(y, D, method='hals', **k))]


@pytest.mark.parametrize('bad', BAD, ids=repr)
@pytest.mark.parametrize('which', ['l1_penalty', 'l2_penalty'])
def test_bad_penalty_is_a_value_error_before_any_gpu_call(no_gpu, which, bad):
    y, D = _problem()
    for name, fn in _solvers():
        with pytest.raises(ValueError):
            fn(y, D, **{which: bad})


def test_penalty_out_of_scope_before_any_gpu_call(no_gpu):
    from decomp_amd import nmf
    from decomp_amd.nmf_methods import grads
    y, D = _problem()
    for method in nmf.MINIBATCH_METHODS:
        for pen in ({'l1_penalty': 0.1}, {'l2_penalty': 0.1}, {'l1_penalty': 0.1, 'l2_penalty': 0.2}):
            with pytest.raises(NotImplementedError):
                nmf.solve(y, D, minibatch=8, method=method, **pen)

    class OwnUpdateX(grads.Gaussian):
        def update_x(self, y, x, d, mask=None):
            return x

    with pytest.raises(NotImplementedError):
        nmf.solve(y, D, likelihood=OwnUpdateX(), l1_penalty=0.5)
    with pytest.raises(NotImplementedError):
        nmf.solve(y, D, likelihood=OwnUpdateX(), l2_penalty=0.5)


def test_zero_and_valid_penalties_pass_the_check(no_gpu):
    """Zero penalties everywhere (minibatch methods and user likelihoods included) and valid non-zero ones on the
    full-batch solvers reach the device copy."""
    from decomp_amd import nmf
    from decomp_amd.nmf_methods import grads
    y, D = _problem()

    class OwnUpdateX(grads.Gaussian):
        def update_x(self, y, x, d, mask=None):
            return x

    ok = [dict(l1_penalty=0.0, l2_penalty=0.0), dict(l1_penalty=0, l2_penalty=np.float32(0))]
    for pen in ok:
        with pytest.raises(AssertionError, match='GPU call'):
            nmf.solve(y, D, minibatch=8, method='asg-mu', **pen)
        with pytest.raises(AssertionError, match='GPU call'):
            nmf.solve(y, D, likelihood=OwnUpdateX(), **pen)
    for pen in ok + [dict(l1_penalty=0.3), dict(l2_penalty=np.float64(2.0)), dict(l1_penalty=1, l2_penalty=1e-3)]:
        for name, fn in _solvers():
            with pytest.raises(AssertionError, match='GPU call'):
                fn(y, D, **pen)


def test_keywords_follow_random_seed():
    """Appended after random_seed: the reference's positional order is kept."""
    import inspect
    from decomp_amd import nmf
    names = list(inspect.signature(nmf.solve).parameters)
    i = names.index('random_seed')
    assert names[i + 1:i + 3] == ['l1_penalty', 'l2_penalty']
    assert inspect.signature(nmf.solve).parameters['l1_penalty'].default == 0.0
    assert inspect.signature(nmf.solve).parameters['l2_penalty'].default == 0.0


# ---- the restatement ---------------------------------------------------------------------------------------
def _golden_cases(golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, 'nmf_golden.npz'), allow_pickle=False)
    return g, [str(c) for c in g['cases']]


def test_restatement_at_zero_equals_oracle_iterates(golden_dir):
    """At l1 = l2 = 0 the penalised MU step is the oracle's step on every golden case (both likelihoods, mask or
    not), and the oracle's iterates are the reference's golden trace."""
    from oracle import common
    from oracle import nmf as onmf
    g, cases = _golden_cases(golden_dir)
    for name in cases:
        base, mtag = name.rsplit('_', 1)
        y = g[base + '/y'].astype(np.float64)
        D0 = g[base + '/D0'].astype(np.float64)
        mask = g[base + '/mask'].astype(np.float64) if mtag == 'mask' else None
        lik = 'kl' if '_kl' in base else 'l2'
        n = len(g[name + '/trace_maxdiff'])
        x, D = np.ones((y.shape[0], D0.shape[0])), common.l2_strict(D0)
        for i, (xp, Dp) in enumerate(penalty_ref.mu_iterates(y, D0, mask=mask, likelihood=lik, n=n)):
            x, D, _ = onmf.mu_step(y, x, D, mask, lik)
            assert np.array_equal(xp, x) and np.array_equal(Dp, D), (name, i)
        if g[base + '/y'].dtype == np.float64:
            scale = max(1.0, float(np.max(np.abs(g[name + '/trace_x']))))
            assert np.max(np.abs(x - g[name + '/trace_x'])) <= 1e-9 * scale, name


def test_restatement_at_zero_equals_plain_hals():
    """At l1 = l2 = 0 the penalised HALS step is the plain sweep (the x sweep on Y D^T and D D^T)."""
    rng = np.random.RandomState(2)
    y, D = np.abs(rng.randn(30, 20)), np.abs(rng.randn(4, 20)) + 0.1
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    x = np.abs(rng.randn(30, 4))
    xs = penalty_ref.sweep(x, y.dot(D.T), D.dot(D.T))
    assert np.array_equal(penalty_ref.hals_x_sweep(y, x, D), xs)


def test_restatement_penalised_mu_formula():
    """The penalised MU x update is the quotient with l1 + l2 x added to the negative part, and shrinks x."""
    from oracle import nmf as onmf
    rng = np.random.RandomState(3)
    y, D = np.abs(rng.randn(25, 16)), np.abs(rng.randn(5, 16)) + 0.1
    x = np.abs(rng.randn(25, 5)) + 0.1
    for lik in ('l2', 'kl', 'is'):
        pos, neg = onmf._parts_x(y, x, D, None, lik)
        got = penalty_ref.mu_update_x(y, x, D, None, lik, 0.3, 0.7)
        assert np.allclose(got, x * np.maximum(pos, 0) / np.maximum(neg + 0.3 + 0.7 * x, 1e-15), rtol=1e-14)
        assert np.all(got <= penalty_ref.mu_update_x(y, x, D, None, lik) + 1e-15)


def test_restatement_hals_x_sweep_is_penalised_coordinate_minimiser():
    """After the penalised sweep no single coordinate change lowers the penalised l2 objective (each coordinate
    was minimised exactly in its turn, and the last pass leaves a KKT point after repetition)."""
    rng = np.random.RandomState(4)
    y, D = np.abs(rng.randn(20, 15)), np.abs(rng.randn(4, 15)) + 0.1
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    l1, l2 = 0.4, 0.3
    x = np.abs(rng.randn(20, 4))
    for _ in range(300):
        x = penalty_ref.hals_x_sweep(y, x, D, l1, l2)
    G, C = D.dot(D.T), y.dot(D.T)
    grad = x.dot(G) - C + l1 + l2 * x
    assert np.all(np.abs(grad[x > 0]) < 1e-10)
    assert np.all(grad[x == 0] > -1e-10)

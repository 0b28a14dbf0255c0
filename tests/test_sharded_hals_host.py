"""CPU: nmf_solve_sharded(method=...) rejects what row-sharded HALS does not cover -- a mask, a likelihood other
than l2, an unknown method -- with NotImplementedError before any GPU call."""
import numpy as np
import pytest


def _problem():
    rng = np.random.RandomState(0)
    return np.abs(rng.randn(40, 12)).astype(np.float32), np.abs(rng.randn(3, 12)).astype(np.float32)


@pytest.fixture
def no_gpu(monkeypatch):
    from decomp_amd import _arrays, _hip

    def boom(*a, **k):
        raise AssertionError('a GPU call was made before the argument check')
    monkeypatch.setattr(_arrays, 'to_device', boom)
    monkeypatch.setattr(_hip, 'load', boom)


def test_hals_scope_errors_before_any_gpu_call(no_gpu):
    from decomp_amd import sharded
    y, D = _problem()
    with pytest.raises(NotImplementedError):
        sharded.nmf_solve_sharded(y, D, mask_local=np.ones_like(y), method='hals')
    with pytest.raises(NotImplementedError):
        sharded.nmf_solve_sharded(y, D, likelihood='kl', method='hals')
    with pytest.raises(NotImplementedError):
        sharded.nmf_solve_sharded(y, D, method='nope')


def test_valid_hals_call_reaches_the_gpu(no_gpu):
    """The l2 likelihood without a mask passes the check: the next step is the device copy."""
    from decomp_amd import sharded
    y, D = _problem()
    for lik in ('l2', 'gaussian'):
        with pytest.raises(AssertionError, match='GPU call'):
            sharded.nmf_solve_sharded(y, D, likelihood=lik, method='hals')

"""CPU: the beta-divergence (Itakura-Saito) likelihood's host surface -- names, dispatch codes, argument
checks and the C ABI pieces that need no GPU."""
import math

import numpy as np
import pytest

from decomp_amd import _hip, nmf
from decomp_amd.nmf_methods import grads
from decomp_amd.utils import assertion


@pytest.mark.parametrize('name', ['is', 'itakura-saito'])
def test_is_names_give_beta_zero(name):
    lik = grads.get_likelihood(name)
    assert isinstance(lik, grads.BetaDivergence) and lik.beta == 0.0
    assert nmf._likelihood_spec(name) == (_hip.LIK_BETA, 0.0)
    assert nmf._likelihood_code(name) == _hip.LIK_BETA == 2


def test_existing_names_keep_their_meaning():
    assert isinstance(grads.get_likelihood('l2'), grads.Gaussian)
    assert isinstance(grads.get_likelihood('kl'), grads.Poisson)
    assert nmf._likelihood_code('l2') == _hip.LIK_L2 and nmf._likelihood_code('kl') == _hip.LIK_KL
    with pytest.raises(NotImplementedError):
        grads.get_likelihood('nope')
    with pytest.raises(NotImplementedError):
        nmf._likelihood_code('nope')


def test_fused_code_routes_beta():
    assert grads.fused_code(grads.BetaDivergence(1.0)) == _hip.LIK_KL
    assert grads.fused_code(grads.BetaDivergence(2.0)) == _hip.LIK_L2
    assert grads.fused_code(grads.BetaDivergence(0.5)) == _hip.LIK_BETA
    assert grads.fused_spec(grads.BetaDivergence(0.5)) == (_hip.LIK_BETA, 0.5)
    assert nmf._likelihood_spec(grads.BetaDivergence(3)) == (_hip.LIK_BETA, 3.0)

    class OnlyLogp(grads.BetaDivergence):
        def logp(self, y, x, d, mask):
            return 0.0

    class OwnGradX(grads.BetaDivergence):
        def grad_x(self, y, x, d, mask):
            return x, x

    class OwnUpdateD(grads.BetaDivergence):
        def update_d(self, y, x, d, mask):
            return d

    assert grads.fused_code(OnlyLogp(0.0)) == _hip.LIK_BETA
    assert grads.fused_code(OwnGradX(0.0)) is None
    assert grads.fused_code(OwnUpdateD(2.0)) is None
    inst = OwnGradX(0.5)
    assert nmf._likelihood_code(inst) is inst


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), -float('inf')])
def test_non_finite_beta_raises(bad):
    with pytest.raises(ValueError):
        grads.BetaDivergence(bad)


def test_abi_beta_pieces():
    lib = _hip.load()
    assert 'dcp_set_nmf_beta' in _hip.SIGNATURES
    assert lib.dcp_set_nmf_beta(None, 0.0) == -1
    assert lib.dcp_set_nmf_beta(None, float('nan')) == -1
    assert lib.dcp_nmf_mu_stats_width(4096, 256, 2, 0) == 8192
    assert lib.dcp_nmf_mu_stats_width(4096, 256, 2, 1) == 8192
    for s in ('f32', 'f64'):
        assert getattr(lib, 'dcp_nmf_beta_divergence_' + s) is not None
        assert 'dcp_nmf_beta_divergence_' + s in _hip.SIGNATURES


def test_assert_positive_matches_reference():
    assertion.assert_positive(None)
    assertion.assert_positive(np.array([[1.0, 2.0], [0.5, 1e-30]]))
    for bad in (np.array([1.0, 0.0]), np.array([1.0, -1.0]), np.array([1.0, math.nan]),
                np.array([1 + 1j, 2 + 0j])):
        with pytest.raises(AssertionError):
            assertion.assert_positive(bad)


def test_assert_positive_where_mask():
    y = np.array([[1.0, 0.0], [2.0, 3.0]])
    m = np.array([[1.0, 0.0], [1.0, 1.0]])
    assertion.assert_positive_where(y, m)
    with pytest.raises(AssertionError):
        assertion.assert_positive_where(y, None)
    with pytest.raises(AssertionError):
        assertion.assert_positive_where(y, np.ones_like(y))


def test_beta_data_checks_on_host_arrays():
    y = np.array([[1.0, 0.0], [2.0, 3.0]])
    m = np.array([[1.0, 0.0], [1.0, 1.0]])
    nmf._check_beta_data('is', y, m)                          # the zero is masked out
    with pytest.raises(AssertionError):
        nmf._check_beta_data('is', y, None)
    nmf._check_beta_data(grads.BetaDivergence(0.5), y, None)  # 0 < beta < 2: y >= 0 suffices
    with pytest.raises(AssertionError):
        nmf._check_beta_data(grads.BetaDivergence(1.5), -y, None)
    nmf._check_beta_data(grads.BetaDivergence(2.0), -y, None)  # the square loss takes any y
    nmf._check_beta_data('l2', -y, None)

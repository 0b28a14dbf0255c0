"""GPU: the fused beta-divergence (Itakura-Saito) NMF likelihood -- golden parity with the real reference,
the fused kernels against the host plugin loop and a float64 NumPy restatement, routing of beta 1 / 2 to the
'kl' / 'l2' kernels, the sharded and out-of-core paths, and the input checks."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nmf_beta_golden.npz')
SHAPES = [(64, 48, 4), (101, 20, 3)]
BETAS = [0.0, 0.5, 1.5, 3.0]
TOL = {'float32': 2e-4, 'float64': 1e-9}


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, float(np.max(np.abs(b)))))


def _np(a):
    import torch
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


# ---- float64 NumPy restatement of the math of the issue --------------------------------------------------
def parts_np(y, x, d, mask, beta):
    y, x, d = (np.asarray(a, np.float64) for a in (y, x, d))
    V = x.dot(d) + 1e-15
    M = np.ones_like(V) if mask is None else np.asarray(mask, np.float64)
    return y * M * V ** (beta - 2.0), M * V ** (beta - 1.0)


def grad_x_np(y, x, d, mask, beta):
    r1, r2 = parts_np(y, x, d, mask, beta)
    d = np.asarray(d, np.float64)
    return r1.dot(d.T), r2.dot(d.T)


def grad_d_np(y, x, d, mask, beta):
    r1, r2 = parts_np(y, x, d, mask, beta)
    x = np.asarray(x, np.float64)
    return x.T.dot(r1), x.T.dot(r2)


def divergence_np(y, x, d, mask, beta):
    y = np.asarray(y, np.float64)
    v = np.asarray(x, np.float64).dot(np.asarray(d, np.float64)) + 1e-15
    M = np.ones_like(v) if mask is None else np.asarray(mask, np.float64)
    keep = M != 0
    y, v, M = y[keep], v[keep], M[keep]
    if beta == 0.0:
        e = y / v - np.log(y / v) - 1.0
    elif beta == 1.0:
        e = np.where(y > 0, y * np.log(np.where(y > 0, y, 1.0) / v), 0.0) - y + v
    elif beta == 2.0:
        e = 0.5 * (y - v) ** 2
    else:
        e = (y ** beta + (beta - 1.0) * v ** beta - beta * y * v ** (beta - 1.0)) / (beta * (beta - 1.0))
    return float(np.sum(M * e))


def mu_np(y, D0, mask, beta, iters):
    """batch_mu.solve with the beta rule in float64 (x = ones, D l2_strict normalised, tol = 0)."""
    D = np.asarray(D0, np.float64)
    D = D / np.sqrt(np.sum(D * D, axis=1, keepdims=True))
    x = np.ones((y.shape[0], D.shape[0]))
    for _ in range(iters):
        p, n = grad_x_np(y, x, D, mask, beta)
        x = x * np.maximum(p, 0) / np.maximum(n, 1e-15)
        p, n = grad_d_np(y, x, D, mask, beta)
        U = D * np.maximum(p, 0) / np.maximum(n, 1e-15)
        D = U / np.sqrt(np.sum(U * U, axis=1, keepdims=True))
    return D, x


def beta_data(seed, N, F, K, dtype, masked):
    rng = np.random.RandomState(seed)
    Dt = rng.uniform(0.1, 1.0, size=(K, F))
    xt = rng.uniform(0.1, 1.0, size=(N, K))
    y = xt.dot(Dt) * rng.uniform(0.7, 1.3, size=(N, F))
    D0 = Dt * rng.uniform(0.5, 1.5, size=(K, F))
    x0 = xt * rng.uniform(0.5, 1.5, size=(N, K))
    mask = None
    if masked:
        mask = (rng.uniform(size=(N, F)) >= 0.3).astype(dtype)
        y = y * mask
    return y.astype(dtype), D0.astype(dtype), x0.astype(dtype), mask


# ---- golden parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['float32', 'float64'])
@pytest.mark.parametrize('si', [0, 1])
def test_golden_batch_mu(si, dt):
    from decomp_amd import nmf
    from decomp_amd.nmf_methods.grads import BetaDivergence
    g = np.load(GOLDEN)
    y, ym, D0, mask = (g['in/%d/%s/%s' % (si, dt, n)] for n in ('y', 'ym', 'D0', 'mask'))
    for beta in BETAS:
        for masked in (0, 1):
            yy, mm = (ym, mask) if masked else (y, None)
            lik = 'is' if beta == 0.0 and masked else BetaDivergence(beta)
            it, D, x = nmf.solve(yy, D0, tol=0.0, maxiter=25, likelihood=lik, mask=mm)
            key = 'mu/%d/%s/%s/%d/' % (si, dt, beta, masked)
            assert it == 25
            assert D.dtype == np.dtype(dt) and x.dtype == np.dtype(dt)
            assert _rel(D, g[key + 'D']) < TOL[dt], (key, _rel(D, g[key + 'D']))
            assert _rel(x, g[key + 'x']) < TOL[dt], (key, _rel(x, g[key + 'x']))


@pytest.mark.parametrize('dt', ['float32', 'float64'])
def test_golden_early_stop(dt):
    from decomp_amd import nmf
    g = np.load(GOLDEN)
    y, D0 = g['in/0/%s/y' % dt], g['in/0/%s/D0' % dt]
    it, D, x = nmf.solve(y, D0, tol=float(g['stop/%s/tol' % dt]), maxiter=400, likelihood='itakura-saito')
    assert it == int(g['stop/%s/it' % dt])
    assert _rel(D, g['stop/%s/D' % dt]) < TOL[dt] and _rel(x, g['stop/%s/x' % dt]) < TOL[dt]


@pytest.mark.parametrize('dt', ['float32', 'float64'])
@pytest.mark.parametrize('method', ['asg-mu', 'svrmu'])
def test_golden_minibatch(method, dt):
    from decomp_amd import nmf
    g = np.load(GOLDEN)
    y, D0 = g['in/0/%s/y' % dt], g['in/0/%s/D0' % dt]
    it, D, x = nmf.solve(y, D0, tol=0.0, minibatch=16, maxiter=6, method=method, likelihood='is', random_seed=3)
    key = 'mb/%s/%s/' % (method, dt)
    assert it == int(g[key + 'it'])
    assert _rel(D, g[key + 'D']) < TOL[dt] and _rel(x, g[key + 'x']) < TOL[dt]


# ---- the fused path against the host plugin loop ---------------------------------------------------------------
@pytest.mark.parametrize('dt', ['float32', 'float64'])
@pytest.mark.parametrize('beta', [0.0, 0.5])
@pytest.mark.parametrize('masked', [False, True])
def test_fused_matches_host_plugin_loop(beta, masked, dt):
    from decomp_amd import nmf
    from decomp_amd.nmf_methods import grads

    class NumpyBeta(grads.Likelihood):   # overrides the loop methods: runs through nmf._run_mu_user
        def grad_x(self, y, x, d, mask):
            r1, r2 = parts_np(y, x, d, mask, beta)
            return r1.dot(d.T).astype(x.dtype), r2.dot(d.T).astype(x.dtype)

        def grad_d(self, y, x, d, mask):
            r1, r2 = parts_np(y, x, d, mask, beta)
            return x.T.dot(r1).astype(d.dtype), x.T.dot(r2).astype(d.dtype)

    assert grads.fused_code(NumpyBeta()) is None
    y, D0, _, mask = beta_data(5, 101, 20, 3, dt, masked)
    it_h, D_h, x_h = nmf.solve(y, D0, tol=0.0, maxiter=20, likelihood=NumpyBeta(), mask=mask)
    it_f, D_f, x_f = nmf.solve(y, D0, tol=0.0, maxiter=20, likelihood=grads.BetaDivergence(beta), mask=mask)
    assert it_h == it_f == 20
    assert _rel(D_f, D_h) < TOL[dt] and _rel(x_f, x_h) < TOL[dt]


# ---- routing: beta 1 / 2 run the 'kl' / 'l2' kernels ------------------------------------------------------------
@pytest.mark.parametrize('dt', ['float32', 'float64'])
@pytest.mark.parametrize('masked', [False, True])
def test_routing_bit_identical(masked, dt):
    from decomp_amd import nmf
    from decomp_amd.nmf_methods.grads import BetaDivergence
    y, D0, _, mask = beta_data(7, 96, 64, 5, dt, masked)
    for beta, name in ((1.0, 'kl'), (2.0, 'l2')):
        a = nmf.solve(y, D0, tol=0.0, maxiter=12, likelihood=BetaDivergence(beta), mask=mask)
        b = nmf.solve(y, D0, tol=0.0, maxiter=12, likelihood=name, mask=mask)
        assert a[0] == b[0]
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (beta, name)


# ---- grad_x, grad_d, divergence against the float64 restatement ------------------------------------------------
GRAD_SHAPES = [(101, 20, 3), (256, 128, 8), (1000, 4090, 250)]


@pytest.mark.parametrize('shape', GRAD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('dt', ['float32', 'float64'])
@pytest.mark.parametrize('masked', [False, True])
def test_grads_and_divergence(shape, dt, masked):
    import torch
    from decomp_amd.nmf_methods.grads import BetaDivergence
    N, F, K = shape
    y, D0, x0, mask = beta_data(11, N, F, K, dt, masked)
    D = D0 / np.sqrt(np.sum(D0.astype(np.float64) ** 2, axis=1, keepdims=True)).astype(dt)
    tol = 1e-4 if dt == 'float32' else 1e-9
    for beta in (0.0, 0.5, 1.0, 1.5, 2.0, 3.0):
        lik = BetaDivergence(beta)
        px, nx = lik.grad_x(y, x0, D, mask)
        assert isinstance(px, np.ndarray) and px.shape == (N, K) and nx.shape == (N, K) and px.dtype == y.dtype
        ex, fx = grad_x_np(y, x0, D, mask, beta)
        assert _rel(px, ex) < tol and _rel(nx, fx) < tol, (beta, _rel(px, ex), _rel(nx, fx))
        pd, nd = lik.grad_d(y, x0, D, mask)
        assert pd.shape == (K, F) and nd.shape == (K, F)
        ed, fd = grad_d_np(y, x0, D, mask, beta)
        assert _rel(pd, ed) < tol and _rel(nd, fd) < tol, (beta, _rel(pd, ed), _rel(nd, fd))
        dv = lik.divergence(y, x0, D, mask)
        ref = divergence_np(y, x0, D, mask, beta)
        assert isinstance(dv, np.generic) and dv.dtype == y.dtype
        assert abs(float(dv) - ref) <= tol * abs(ref), (beta, float(dv), ref)
        assert float(lik.logp(y, x0, D, mask)) == -float(dv)
    # torch in -> torch out
    yt, xt, Dt = (torch.from_numpy(a).cuda() for a in (y, x0, D))
    mt = None if mask is None else torch.from_numpy(mask).cuda()
    p, n = BetaDivergence(0.0).grad_x(yt, xt, Dt, mt)
    assert isinstance(p, torch.Tensor) and p.is_cuda
    assert isinstance(BetaDivergence(0.5).divergence(yt, xt, Dt, mt), torch.Tensor)


# ---- properties ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [1.25, 1.5, 1.75])
def test_x_updates_do_not_increase_divergence(beta):
    import torch
    from decomp_amd import _arrays, _hip
    from decomp_amd.nmf_methods.grads import BetaDivergence, set_beta
    y, D0, x0, _ = beta_data(13, 200, 96, 6, 'float64', False)
    D = D0 / np.sqrt(np.sum(D0 ** 2, axis=1, keepdims=True))
    x0 = np.random.RandomState(1).uniform(0.05, 2.0, size=x0.shape)
    yd, Dd, xd = (torch.from_numpy(a).cuda() for a in (y, D, x0))
    gp, gn = torch.empty_like(Dd), torch.empty_like(Dd)
    lik = BetaDivergence(beta)
    lib, h = _arrays.lib_handle(Dd)
    prev = float(lik.divergence(yd, xd, Dd, None))
    for _ in range(15):
        set_beta(h, _hip.LIK_BETA, beta)
        _hip.check(h, lib.dcp_nmf_grads_f64(h, _arrays.ptr(yd), None, _arrays.ptr(xd), _arrays.ptr(Dd), 200, 96, 6,
                                           _hip.LIK_BETA, 1, _arrays.ptr(gp), _arrays.ptr(gn)), 'dcp_nmf_grads')
        cur = float(lik.divergence(yd, xd, Dd, None))
        assert cur <= prev * (1 + 1e-12), (prev, cur)
        prev = cur


def test_is_batch_iterations_decrease_divergence():
    from decomp_amd import nmf
    from decomp_amd.nmf_methods.grads import BetaDivergence
    y, D0, _, _ = beta_data(17, 128, 64, 4, 'float64', False)
    lik = BetaDivergence(0.0)
    Dn = D0 / np.sqrt(np.sum(D0 ** 2, axis=1, keepdims=True))
    start = float(lik.divergence(y, np.ones((128, 4)), Dn, None))
    it, D, x = nmf.solve(y, D0, tol=0.0, maxiter=51, likelihood='is')
    end = float(lik.divergence(y, x, D, None))
    assert np.isfinite(end) and end < start, (start, end)


# ---- the benchmark shape ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('beta', [0.0, 0.5])
@pytest.mark.parametrize('masked', [False, True])
def test_large_shape_three_iterations(beta, masked):
    """16384 x 4096, k = 256, float32, 3 iterations against float64.  1e-4 relative (max-abs) on x and D: the
    positive data keep V away from zero, so V^-2 (IS) amplifies the fp32 product's relative error only by 2x."""
    import torch
    from decomp_amd import nmf
    from decomp_amd.nmf_methods.grads import BetaDivergence
    N, F, K = 16384, 4096, 256
    y, D0, _, mask = beta_data(19, N, F, K, 'float32', masked)
    yt, Dt = torch.from_numpy(y).cuda(), torch.from_numpy(D0).cuda()
    mt = None if mask is None else torch.from_numpy(mask).cuda()
    it, D, x = nmf.solve(yt, Dt, tol=0.0, maxiter=4, likelihood=BetaDivergence(beta), mask=mt)
    D, x = _np(D), _np(x)
    assert it == 4 and np.all(np.isfinite(D)) and np.all(np.isfinite(x))
    De, xe = mu_np(y, D0, mask, beta, 3)
    assert _rel(D, De) < 1e-4 and _rel(x, xe) < 1e-4, (_rel(D, De), _rel(x, xe))


# ---- sharded (one rank) and out of core --------------------------------------------------------------------------
@pytest.mark.parametrize('masked', [False, True])
def test_sharded_one_rank_bit_identical(masked):
    import torch
    from decomp_amd import nmf, sharded
    y, D0, _, mask = beta_data(23, 300, 80, 5, 'float32', masked)
    yt, Dt = torch.from_numpy(y).cuda(), torch.from_numpy(D0).cuda()
    mt = None if mask is None else torch.from_numpy(mask).cuda()
    a = sharded.nmf_solve_sharded(yt, Dt, tol=1e-4, maxiter=30, likelihood='is', mask_local=mt)
    b = nmf.solve(yt, Dt, tol=1e-4, maxiter=30, likelihood='is', mask=mt)
    assert a[0] == b[0]
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_out_of_core_matches_in_core():
    import torch
    from decomp_amd import nmf
    y, D0, x0, _ = beta_data(29, 200, 64, 4, 'float64', False)
    Dt = torch.from_numpy(D0).cuda()
    it_s, D_s, x_s = nmf.solve(y, Dt, x=x0.copy(), tol=0.0, minibatch=50, maxiter=4, method='asg-mu',
                               likelihood='is', random_seed=1)
    assert isinstance(x_s, np.ndarray)
    it_c, D_c, x_c = nmf.solve(torch.from_numpy(y).cuda(), Dt, x=torch.from_numpy(x0).cuda(), tol=0.0,
                               minibatch=50, maxiter=4, method='asg-mu', likelihood='is', random_seed=1)
    assert it_s == it_c
    np.testing.assert_allclose(_np(D_s), _np(D_c), rtol=1e-12, atol=0)
    np.testing.assert_allclose(x_s, _np(x_c), rtol=1e-12, atol=0)


# ---- input checks ----------------------------------------------------------------------------------------------
def test_zero_data_under_is():
    from decomp_amd import nmf
    from decomp_amd.nmf_methods.grads import BetaDivergence
    y, D0, _, _ = beta_data(31, 40, 16, 3, 'float64', False)
    y[3, 5] = 0.0
    with pytest.raises(AssertionError):
        nmf.solve(y, D0, tol=0.0, maxiter=3, likelihood='is')
    with pytest.raises(AssertionError):
        nmf.solve(y, D0, tol=0.0, maxiter=3, likelihood=BetaDivergence(-0.5))
    mask = np.ones_like(y)
    mask[3, 5] = 0.0
    it, D, x = nmf.solve(y, D0, tol=0.0, maxiter=3, likelihood='is', mask=mask)
    assert it == 3 and np.all(np.isfinite(D)) and np.all(np.isfinite(x))
    nmf.solve(y, D0, tol=0.0, maxiter=3, likelihood=BetaDivergence(0.5))     # 0 < beta < 2: zeros allowed
    y[0, 0] = -1.0
    with pytest.raises(AssertionError):
        nmf.solve(y, D0, tol=0.0, maxiter=3, likelihood=BetaDivergence(1.5))


@pytest.mark.parametrize('masked', [False, True])
def test_few_rows_split_x_update(masked):
    """Rows not a multiple of 256 with few row tiles: the x update splits its F reduction (slab path, not the
    stacked launch).  3 float32 iterations against float64."""
    from decomp_amd import nmf
    from decomp_amd.nmf_methods.grads import BetaDivergence
    y, D0, _, mask = beta_data(37, 1000, 2048, 64, 'float32', masked)
    it, D, x = nmf.solve(y, D0, tol=0.0, maxiter=4, likelihood=BetaDivergence(0.0), mask=mask)
    De, xe = mu_np(y, D0, mask, 0.0, 3)
    assert it == 4 and _rel(D, De) < 1e-4 and _rel(x, xe) < 1e-4, (_rel(D, De), _rel(x, xe))

"""GPU: the L1/L2 penalty on the NMF codes (nmf.solve / nmf_solve_sharded l1_penalty, l2_penalty,
dcp_set_nmf_penalty) -- zero is bit for bit the unpenalised solver, a penalised call does not leak into the next,
MU and HALS follow the float64 restatement (penalty_ref.py) on every x-update path, the HALS x sweep reaches the
elastic-net NNLS optimum (and the lasso's at l2 = 0), MU x steps descend, and the sharded loops agree.

Paths of the float32 x update (nmf_stats, nmf_impl.hpp) reached here: (2048, 512, 128) F < 1024, unsplit: the
quotient fused into the Y D^T epilogue (EpiMuNum, on the bf16x6 core in product mode 0, the fp32 MFMA core in
mode 1); (2048, 1024, 256) F split: l2 without a mask EpiMuDenSlabs (X_out != X) or mu_quotient_slabs_kernel
(X_out == X, dcp_nmf_mu_stats_*), masked l2 and 'is' the stacked product and mu_quotient_stacked_kernel, kl
mu_quotient_slabs_kernel; (1000, 300, 30) the bounds-checked tiles.  float64: unsplit on the fp64 MFMA core, split
(2048, 1024, 256) with mu_quotient_slabs_kernel."""
import functools

import numpy as np
import pytest

import penalty_ref
from test_gpu_nmf_bf16x6 import _Mode
from test_gpu_nmf_hals_sharded import _finish, _free_port, _spawn

pytestmark = pytest.mark.gpu

SHAPES = {'fused': (2048, 512, 128), 'split': (2048, 1024, 256), 'odd': (1000, 300, 30)}
PRECS = ['f32m0', 'f32m1', 'f64']
LIKS = ['l2', 'kl', 'is']


@functools.lru_cache(maxsize=None)
def _problem(shape, masked):
    N, F, K = SHAPES[shape]
    rng = np.random.RandomState(N + F + K + int(masked))
    xt = np.maximum(rng.randn(N, K), 0)
    Dt = np.maximum(rng.randn(K, F), 0)
    y = (xt.dot(Dt) + 0.1 * np.abs(rng.randn(N, F)) + 0.01).astype(np.float32)
    d0 = np.maximum(Dt + 0.3 * rng.randn(K, F), 0.1).astype(np.float32)
    m = (rng.rand(N, F) >= 0.2).astype(np.float32) if masked else None
    return y, d0, m


def _cast(prec, *arrays):
    dt = np.float64 if prec == 'f64' else np.float32
    return tuple(None if a is None else a.astype(dt) for a in arrays)


class _Prec:
    """The product mode of the float32 cases for the duration of a block (float64: nothing to set)."""

    def __init__(self, prec):
        self.mode = {'f32m0': 0, 'f32m1': 1}.get(prec)
        self.ctx = None

    def __enter__(self):
        if self.mode is not None:
            self.ctx = _Mode(self.mode)
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)


@functools.lru_cache(maxsize=None)
def _scale(shape, masked, lik):
    """c of the (c, 0) / (0, c) / (c, c) penalties: a tenth of the mean negative x-gradient part at x = 1."""
    from oracle import common
    from oracle import nmf as onmf
    y, d0, m = _problem(shape, masked)
    y, d, m = (None if a is None else a.astype(np.float64) for a in (y, common.l2_strict(d0.astype(np.float64)), m))
    _, neg = onmf._parts_x(y, np.ones((y.shape[0], d.shape[0])), d, m, lik)
    return 0.1 * float(np.mean(neg))


def _pens(c):
    return [(c, 0.0), (0.0, c), (c, c)]


def _solve(prec, shape, lik, masked, n, method='mu', **pen):
    import decomp_amd
    y, d0, m = _cast(prec, *_problem(shape, masked))
    with _Prec(prec):
        it, D, x = decomp_amd.nmf.solve(y, d0, tol=0.0, maxiter=n + 1, likelihood=lik, mask=m, method=method, **pen)
    assert it == n + 1
    return D, x


def _lib_h(t):
    from decomp_amd import _arrays
    return _arrays.lib_handle(t)


def _mu_stats(prec, Y, M, X, X_out, D, lik):
    """dcp_nmf_mu_stats_* -> stats (X_out written)."""
    import torch
    from decomp_amd import _arrays, _hip, nmf
    N, F = Y.shape
    K = D.shape[0]
    code = nmf._likelihood_code(lik)
    W = _hip.load().dcp_nmf_mu_stats_width(F, K, code, 0 if M is None else 1)
    stats = torch.empty((K, W), dtype=Y.dtype, device='cuda')
    lib, h = _lib_h(D)
    if code == _hip.LIK_BETA:
        _hip.check(h, lib.dcp_set_nmf_beta(h, 0.0), 'dcp_set_nmf_beta')
    sfx = 'f64' if prec == 'f64' else 'f32'
    with _Prec(prec):
        _hip.check(h, getattr(lib, 'dcp_nmf_mu_stats_' + sfx)(h, _arrays.ptr(Y), _arrays.ptr(M), _arrays.ptr(X),
                                                              _arrays.ptr(X_out), _arrays.ptr(D), N, F, K, code,
                                                              _arrays.ptr(stats)), 'dcp_nmf_mu_stats')
    torch.cuda.synchronize()
    return stats


def _set_penalty(D, l1, l2):
    from decomp_amd import nmf
    nmf._set_penalty(_lib_h(D)[1], (l1, l2))


@pytest.fixture(autouse=True)
def _reset_penalty():
    """Every test leaves the device-0 handle without a penalty, whatever it did."""
    yield
    import torch
    from decomp_amd import nmf
    nmf._set_penalty(_lib_h(torch.empty(1, device='cuda'))[1], (0.0, 0.0))


# ---- 1. zero is bit for bit the unpenalised solver ------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_zero_penalty_is_bit_identical(prec, shape):
    for lik in LIKS:
        for masked in (False, True):
            D1, x1 = _solve(prec, shape, lik, masked, 3)
            D2, x2 = _solve(prec, shape, lik, masked, 3, l1_penalty=0.0, l2_penalty=0.0)
            assert np.array_equal(D1, D2) and np.array_equal(x1, x2), (lik, masked)
    D1, x1 = _solve(prec, shape, 'l2', False, 3, method='hals')
    D2, x2 = _solve(prec, shape, 'l2', False, 3, method='hals', l1_penalty=0, l2_penalty=0)
    assert np.array_equal(D1, D2) and np.array_equal(x1, x2)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('inplace', [False, True])
def test_zero_penalty_stats_entry_is_bit_identical(prec, inplace):
    """dcp_nmf_mu_stats_* on the split shape (split_gram with X_out != X, the slab quotient in place): the handle
    at (0, 0) after a penalised setting gives the never-penalised result."""
    import torch
    from decomp_amd import _arrays
    y, d0, m = _cast(prec, *_problem('split', False))
    Y, D = torch.from_numpy(y).cuda(), torch.from_numpy(d0).cuda()
    _arrays.l2_normalize_(D, strict=True)
    x0, = _cast(prec, np.random.RandomState(5).rand(Y.shape[0], D.shape[0]) + 0.1)
    X0 = torch.from_numpy(x0).cuda()
    outs = []
    for pen in [None, (0.5, 0.5), (0.0, 0.0)]:
        if pen is not None:
            _set_penalty(D, *pen)
        X = X0.clone()
        Xo = X if inplace else torch.empty_like(X)
        st = _mu_stats(prec, Y, None, X, Xo, D, 'l2')
        outs.append((Xo.cpu().numpy(), st.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[2][0]) and np.array_equal(outs[0][1], outs[2][1])
    assert not np.array_equal(outs[0][0], outs[1][0])


# ---- 2. no leak -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
def test_penalised_call_does_not_leak(prec):
    for method, lik in (('mu', 'l2'), ('mu', 'kl'), ('hals', 'l2')):
        D1, x1 = _solve(prec, 'split', lik, False, 2, method=method)
        Dp, xp = _solve(prec, 'split', lik, False, 2, method=method, l1_penalty=1.0, l2_penalty=1.0)
        assert not np.array_equal(xp, x1)
        D2, x2 = _solve(prec, 'split', lik, False, 2, method=method)
        assert np.array_equal(D1, D2) and np.array_equal(x1, x2), (method, lik)


def test_fresh_handle_default_matches_after_penalised_solve():
    """A default solve after a penalised one on this device equals a default solve in a fresh process."""
    _solve('f32m0', 'fused', 'l2', True, 2, l1_penalty=0.7, l2_penalty=0.2)
    D2, x2 = _solve('f32m0', 'fused', 'l2', True, 2)
    p, q = _spawn(_fresh_worker, ())
    D1, x1 = _finish(p, q)
    assert np.array_equal(D1, D2) and np.array_equal(x1, x2)


def _fresh_worker(q):
    import os
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.cuda.set_device(0)
    q.put(_solve('f32m0', 'fused', 'l2', True, 2))


# ---- 3. parity with the restatement ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_mu(shape, masked, lik, l1, l2):
    y, d0, m = _problem(shape, masked)
    return penalty_ref.mu_iterates(y, d0, mask=m, likelihood=lik, l1=l1, l2=l2, n=5)


@functools.lru_cache(maxsize=None)
def _ref_hals(shape, l1, l2):
    y, d0, _ = _problem(shape, False)
    return penalty_ref.hals_iterates(y, d0, l1=l1, l2=l2, n=5)


def _tols(prec, n):
    if prec == 'f64':
        return 1e-10 if n == 1 else 1e-9
    return 2e-4 if n == 1 else 1e-3     # fp32 and bf16x6 (test_gpu_tile_tiers.py: 2e-4 over three steps)


def _check(prec, n, D, x, ref, what):
    xr, dr = ref[n - 1]
    dx = float(np.max(np.abs(x - xr)) / max(1.0, float(np.max(np.abs(xr)))))
    dd = float(np.max(np.abs(D - dr)))
    tol = _tols(prec, n)
    assert dx <= tol and dd <= tol, (what, n, dx, dd)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('lik', LIKS)
@pytest.mark.parametrize('masked', [False, True])
def test_mu_parity_with_restatement(prec, shape, lik, masked):
    c = _scale(shape, masked, lik)
    for l1, l2 in _pens(c):
        ref = _ref_mu(shape, masked, lik, l1, l2)
        for n in (1, 5):
            D, x = _solve(prec, shape, lik, masked, n, l1_penalty=l1, l2_penalty=l2)
            _check(prec, n, D, x, ref, (l1, l2))


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_hals_parity_with_restatement(prec, shape):
    c = _scale(shape, False, 'l2')
    for l1, l2 in _pens(c):
        ref = _ref_hals(shape, l1, l2)
        for n in (1, 5):
            D, x = _solve(prec, shape, 'l2', False, n, method='hals', l1_penalty=l1, l2_penalty=l2)
            _check(prec, n, D, x, ref, (l1, l2))


@pytest.mark.parametrize('prec', PRECS)
def test_mu_stats_entry_parity(prec):
    """dcp_nmf_mu_stats_* with the penalty on the handle (split_gram and the in-place slab quotient)."""
    import torch
    from decomp_amd import _arrays
    from oracle import common
    y, d0, _ = _problem('split', False)
    Dn = common.l2_strict(d0.astype(np.float64))
    x0 = np.random.RandomState(8).rand(y.shape[0], d0.shape[0]) + 0.1
    y, dn, x0 = _cast(prec, y, Dn, x0)
    c = _scale('split', False, 'l2')
    for l1, l2 in _pens(c):
        ref = penalty_ref.mu_update_x(y, x0, dn, None, 'l2', l1, l2)
        for inplace in (False, True):
            Y, D, X = (torch.from_numpy(a).cuda() for a in (y, dn, x0))
            Xo = X if inplace else torch.empty_like(X)
            _set_penalty(D, l1, l2)
            _mu_stats(prec, Y, None, X, Xo, D, 'l2')
            got = Xo.cpu().numpy()
            assert np.max(np.abs(got - ref)) / np.max(np.abs(ref)) <= _tols(prec, 1), (l1, l2, inplace)


# ---- 4. not only the restatement ------------------------------------------------------------------------
def _hals_stats(Y, X, X_out, D):
    import torch
    from decomp_amd import _arrays, _hip
    N, F = Y.shape
    K = D.shape[0]
    stats = torch.empty((K, F + K), dtype=Y.dtype, device='cuda')
    lib, h = _lib_h(D)
    _hip.check(h, lib.dcp_nmf_hals_stats_f64(h, _arrays.ptr(Y), _arrays.ptr(X), _arrays.ptr(X_out), _arrays.ptr(D),
                                             N, F, K, _arrays.ptr(stats)), 'dcp_nmf_hals_stats')
    return stats


def _fixed_d_problem(N=600, F=200, K=20, seed=21):
    rng = np.random.RandomState(seed)
    xt = np.maximum(rng.randn(N, K), 0) * (rng.rand(N, K) < 0.4)
    Dt = np.maximum(rng.randn(K, F), 0) + 0.02
    Dt /= np.linalg.norm(Dt, axis=1, keepdims=True)
    y = xt.dot(Dt) + 0.05 * np.abs(rng.randn(N, F))
    return y, Dt


def _hals_x_fixed_d(y, D, l1, l2, sweeps):
    import torch
    Y, Dd = torch.from_numpy(y).cuda(), torch.from_numpy(D).cuda()
    X = torch.ones((y.shape[0], D.shape[0]), dtype=torch.float64, device='cuda')
    Xo = torch.empty_like(X)
    _set_penalty(Dd, l1, l2)
    for _ in range(sweeps):
        _hals_stats(Y, X, Xo, Dd)
        X, Xo = Xo, X
    torch.cuda.synchronize()
    return X.cpu().numpy()


@pytest.mark.parametrize('l1,l2', [(0.5, 0.0), (0.0, 0.5), (0.5, 0.5), (2.0, 0.1)])
def test_hals_x_sweeps_reach_elastic_net_kkt(l1, l2):
    y, D = _fixed_d_problem()
    x = _hals_x_fixed_d(y, D, l1, l2, 1000)
    G, C = D.dot(D.T), y.dot(D.T)
    g = x.dot(G) - C + l1 + l2 * x
    tol = 1e-8 * float(np.max(np.abs(C)))
    assert np.all(np.abs(g[x > 0]) <= tol), float(np.max(np.abs(g[x > 0])))
    assert np.all(g[x == 0] >= -tol)
    assert (x == 0).any() or l1 == 0.0


def test_hals_x_at_l2_zero_matches_lasso_cd_pos():
    import decomp_amd
    y, D = _fixed_d_problem()
    F = y.shape[1]
    l1 = 0.5
    x = _hals_x_fixed_d(y, D, l1, 0.0, 1000)
    _, xl = decomp_amd.lasso.solve(y, D, alpha=l1 / F, method='cd_pos', tol=1e-10, maxiter=5000)
    xl = np.asarray(xl)
    assert np.max(np.abs(x - xl)) <= 1e-6 * max(1.0, float(np.max(np.abs(xl))))


@pytest.mark.parametrize('lik', ['l2', 'kl'])
def test_mu_x_steps_never_increase_penalised_objective(lik):
    import torch
    y, D = _fixed_d_problem(seed=22)
    l1, l2 = 0.3, 0.2
    Y, Dd = torch.from_numpy(y).cuda(), torch.from_numpy(D).cuda()
    X = torch.ones((y.shape[0], D.shape[0]), dtype=torch.float64, device='cuda')
    Xo = torch.empty_like(X)
    prev = penalty_ref.objective(y, X.cpu().numpy(), D, None, lik, l1, l2)
    for step in range(20):
        _set_penalty(Dd, l1, l2)
        _mu_stats('f64', Y, None, X, Xo, Dd, lik)
        X, Xo = Xo, X
        cur = penalty_ref.objective(y, X.cpu().numpy(), D, None, lik, l1, l2)
        assert cur <= prev * (1 + 1e-12) + 1e-12, (step, prev, cur)
        prev = cur


@pytest.mark.parametrize('prec', PRECS)
def test_hals_large_l1_gives_zero_codes(prec):
    from oracle import common
    y, d0, _ = _problem('fused', False)
    Dn = common.l2_strict(d0.astype(np.float64))
    big = float(np.max(y.astype(np.float64).dot(Dn.T))) * 1.01
    D, x = _solve(prec, 'fused', 'l2', False, 3, method='hals', l1_penalty=big)
    assert np.all(x == 0)
    assert np.all(np.isfinite(D))


def test_hals_sparsity_grows_with_l1():
    import decomp_amd
    rng = np.random.RandomState(31)
    N, F, K = 1024, 256, 32
    xt = np.maximum(rng.randn(N, K), 0) * (rng.rand(N, K) < 0.25)
    Dt = np.maximum(rng.randn(K, F), 0)
    y = (xt.dot(Dt) + 0.05 * np.abs(rng.randn(N, F))).astype(np.float32)
    d0 = np.maximum(Dt + 0.3 * rng.randn(K, F), 0.1).astype(np.float32)
    c = float(np.mean(y.astype(np.float64).dot((d0 / np.linalg.norm(d0, axis=1, keepdims=True)).T)))
    fr = []
    for l1 in (0.05 * c, 0.3 * c, 1.0 * c):
        _, _, x = decomp_amd.nmf.solve(y, d0.copy(), tol=0.0, maxiter=31, method='hals', l1_penalty=l1)
        fr.append(float(np.mean(x == 0)))
    assert fr[0] < fr[1] < fr[2], fr


# ---- 5. sharded ---------------------------------------------------------------------------------------------
PEN = dict(l1_penalty=0.8, l2_penalty=0.3)


def _sharded_problem():
    y, d0, _ = _problem('fused', False)
    return y[:768], d0


def _world1_worker(q, method, dt):
    import os
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.cuda.set_device(0)
    from decomp_amd import _arrays, _hip, sharded
    y, d0 = _sharded_problem()
    tdt = torch.float32 if dt == 'f32' else torch.float64
    Y = torch.from_numpy(y).cuda().to(tdt)
    D = torch.from_numpy(d0).cuda().to(tdt)
    _arrays.l2_normalize_(D, strict=True)
    x = torch.ones((Y.shape[0], D.shape[0]), dtype=tdt, device='cuda')
    assert sharded.attach_communicator(D), 'RCCL communicator could not be created'
    pen = (PEN['l1_penalty'], PEN['l2_penalty'])
    if method == 'hals':
        it = sharded.hals_solve_in_library(Y, x, D, 0.0, 6, penalty=pen)
    else:
        it = sharded.mu_solve_in_library(Y, None, x, D, _hip.LIK_L2, 0.0, 6, penalty=pen)
    torch.cuda.synchronize()
    sharded.detach_communicator(D)
    q.put((it, D.cpu().numpy(), x.cpu().numpy()))


@pytest.mark.parametrize('method', ['mu', 'hals'])
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_sharded_world1_bit_identical(method, dt):
    """In-library loop on a 1-rank RCCL communicator and the Python loop (no communicator) with a penalty equal
    the one-GPU solve bit for bit."""
    import torch
    import decomp_amd
    from decomp_amd import sharded
    y, d0 = _sharded_problem()
    npdt = np.float32 if dt == 'f32' else np.float64
    y, d0 = y.astype(npdt), d0.astype(npdt)
    it1, D1, x1 = decomp_amd.nmf.solve(y, d0.copy(), tol=0.0, maxiter=6, method=method, **PEN)
    its, Ds, xs = sharded.nmf_solve_sharded(torch.from_numpy(y).cuda(), torch.from_numpy(d0).cuda(), tol=0.0,
                                            maxiter=6, method=method, **PEN)
    assert its == it1
    assert np.array_equal(Ds.cpu().numpy(), D1) and np.array_equal(xs.cpu().numpy(), x1)
    p, q = _spawn(_world1_worker, (method, dt))
    it, D, x = _finish(p, q)
    assert it == it1
    assert np.array_equal(D, D1) and np.array_equal(x, x1)


def _rank_run(rank, world, port, counts, method):
    from datetime import timedelta
    import torch
    import torch.distributed as dist
    from decomp_amd import sharded
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=world,
                            timeout=timedelta(seconds=180))
    try:
        y, d0 = _sharded_problem()
        r0 = sum(counts[:rank])
        it, D, x = sharded.nmf_solve_sharded(torch.from_numpy(y[r0:r0 + counts[rank]]).cuda(),
                                             torch.from_numpy(d0).cuda(), tol=0.0, maxiter=6, method=method, **PEN)
        kind = sharded.communicator_kind(D)
        out = (it, D.cpu().numpy(), x.cpu().numpy(), kind)
        if kind is not None:
            sharded.detach_communicator(D)
        return out
    finally:
        dist.destroy_process_group()


def _gloo_worker(q, rank, world, port, counts, method):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    torch.cuda.set_device(0)
    q.put((rank,) + _rank_run(rank, world, port, counts, method))


@pytest.mark.parametrize('method', ['mu', 'hals'])
def test_two_gloo_ranks_match_one_process(method):
    import decomp_amd
    y, d0 = _sharded_problem()
    it1, D1, x1 = decomp_amd.nmf.solve(y, d0.copy(), tol=0.0, maxiter=6, method=method, **PEN)
    counts = [384, 384]
    port = _free_port()
    p, q = _spawn(_gloo_worker, (1, 2, port, counts, method))
    try:
        res = [(0,) + _rank_run(0, 2, port, counts, method)]
    finally:
        kid = _finish(p, q)
    res = sorted(res + [kid], key=lambda t: t[0])
    for r in res:
        assert r[1] == it1
        assert np.array_equal(r[2], res[0][2])
    x_all = np.concatenate([r[3] for r in res], axis=0)
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    assert rel(res[0][2], D1) < 1e-4 and rel(x_all, x1) < 1e-3

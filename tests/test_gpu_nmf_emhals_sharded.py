"""GPU: row-sharded em-hals (nmf_solve_sharded(method='em-hals')): the in-library loop dcp_nmf_emhals_sharded_*
over a 1-rank RCCL communicator and over gloo (the external exchange), the Python loop through mu_loop
(HipEmHalsStepBackend) and the split step dcp_nmf_impute_* / dcp_nmf_hals_stats_* / dcp_nmf_hals_update_* against
nmf.solve(method='em-hals').  Child processes start with the spawn context; no test has more than 2 processes
with the GPU open (in the gloo test this process is rank 0)."""
import ctypes
import socket
from datetime import timedelta

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL, MAXITER = 2e-3, 200     # the masked problem below stops at iteration 22 (max|dD| 2.0e-3 -> 1.7e-3, float64)


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, float(np.max(np.abs(b)))))


def _sharded_problem():
    """The problem of tests/test_gpu_nmf_hals_sharded.py with 30 % of the entries missing."""
    rng = np.random.RandomState(7)
    N, F, K = 768, 1536, 24
    xt = np.maximum(rng.randn(N, K), 0).astype(np.float32)
    Dt = np.maximum(rng.randn(K, F), 0).astype(np.float32)
    y = (xt @ Dt + 0.1 * np.abs(rng.randn(N, F))).astype(np.float32)
    D0 = np.maximum(Dt + 0.3 * rng.randn(K, F), 0.1).astype(np.float32)
    w = (rng.uniform(size=(N, F)) >= 0.3).astype(np.float32)
    return y, D0, w


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _spawn(target, args):
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=target, args=(q,) + tuple(args))
    p.start()
    return p, q


def _finish(p, q, timeout=300):
    try:
        res = q.get(timeout=timeout)
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    assert p.exitcode == 0
    return res


@pytest.fixture(scope='module')
def single():
    """nmf.solve(method='em-hals') on the whole problem, per dtype and (tol, maxiter): computed once."""
    import decomp_amd
    cache = {}

    def get(dt, tol=TOL, maxiter=MAXITER):
        key = (dt, tol, maxiter)
        if key not in cache:
            y, D0, w = _sharded_problem()
            npdt = np.float32 if dt == 'f32' else np.float64
            cache[key] = decomp_amd.nmf.solve(y.astype(npdt), D0.astype(npdt), tol=tol, maxiter=maxiter,
                                              method='em-hals', mask=w.astype(npdt))
        return cache[key]
    return get


# ---- 1. world 1, RCCL, in-library loop --------------------------------------------------------------------
def _in_library_world1_worker(q, dt):
    import os
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.cuda.set_device(0)
    from decomp_amd import _arrays, sharded
    y, D0, w = _sharded_problem()
    tdt = torch.float32 if dt == 'f32' else torch.float64
    Y = torch.from_numpy(y).cuda().to(tdt)
    W = torch.from_numpy(w).cuda().to(tdt)
    D = torch.from_numpy(D0).cuda().to(tdt)
    _arrays.l2_normalize_(D, strict=True)
    x = torch.ones((Y.shape[0], D.shape[0]), dtype=tdt, device='cuda')
    assert sharded.attach_communicator(D), 'RCCL communicator could not be created on the GPU box'
    assert sharded.communicator_kind(D) == 'rccl'
    it = sharded.emhals_solve_in_library(Y, W, x, D, TOL, MAXITER)
    torch.cuda.synchronize()
    sharded.detach_communicator(D)
    q.put((it, D.cpu().numpy(), x.cpu().numpy()))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_in_library_world1_rccl_bit_exact(dt, single):
    """dcp_nmf_emhals_sharded_* with the all-reduce on a 1-rank RCCL communicator (the identity) reproduces
    nmf.solve(method='em-hals') bit for bit, stop iteration included."""
    it1, D1, x1 = single(dt)
    assert 2 < it1 < MAXITER - 1
    p, q = _spawn(_in_library_world1_worker, (dt,))
    it, D, x = _finish(p, q)
    assert it == it1
    assert np.array_equal(D, D1) and np.array_equal(x, x1)


# ---- 2. world 1 without a communicator: the Python loop -----------------------------------------------------
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('tol,maxiter', [(TOL, MAXITER), (0.0, 6)])
def test_python_loop_world1_bit_exact(dt, tol, maxiter, single):
    """HipEmHalsStepBackend through mu_loop (impute -> stats -> update, speculative next iteration with rollback)
    equals nmf.solve(method='em-hals') bit for bit: converged at an inner iteration, and maxiter reached."""
    import torch
    from decomp_amd import sharded
    y, D0, w = _sharded_problem()
    npdt = np.float32 if dt == 'f32' else np.float64
    it1, D1, x1 = single(dt, tol, maxiter)
    if tol > 0:
        assert 2 < it1 < maxiter - 1
    else:
        assert it1 == maxiter
    Yd = torch.from_numpy(y.astype(npdt)).cuda()
    assert sharded.communicator_kind(Yd) is None
    its, Ds, xs = sharded.nmf_solve_sharded(Yd, torch.from_numpy(D0.astype(npdt)).cuda(), tol=tol, maxiter=maxiter,
                                            method='em-hals', mask_local=torch.from_numpy(w.astype(npdt)).cuda())
    assert its == it1
    assert np.array_equal(Ds.cpu().numpy(), D1) and np.array_equal(xs.cpu().numpy(), x1)


def test_python_loop_without_mask_is_sharded_hals():
    import torch
    from decomp_amd import sharded
    y, D0, _ = _sharded_problem()
    Yd, Dd = torch.from_numpy(y).cuda(), torch.from_numpy(D0).cuda()
    a = sharded.nmf_solve_sharded(Yd, Dd, tol=0.0, maxiter=4, method='hals')
    b = sharded.nmf_solve_sharded(Yd, Dd, tol=0.0, maxiter=4, method='em-hals')
    assert a[0] == b[0] == 4
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ---- 3. the split step is one loop iteration ------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('pen', [(0.0, 0.0), (0.1, 0.5)])
def test_split_step_is_one_loop_iteration(dt, pen):
    """dcp_nmf_impute_*, dcp_nmf_hals_stats_* on its output, dcp_nmf_hals_update_*: bit-equal to one iteration of
    dcp_nmf_emhals_* (maxiter = 2), penalty on the codes included."""
    import torch
    from decomp_amd import _arrays, _hip, nmf
    rng = np.random.RandomState(3)
    N, F, K = 300, 200, 20
    tdt = torch.float32 if dt == 'f32' else torch.float64
    y = np.maximum(rng.randn(N, K), 0).dot(np.maximum(rng.randn(K, F), 0)) + 0.05 * np.abs(rng.randn(N, F))
    D = np.abs(rng.randn(K, F)) + 0.05
    x = np.abs(rng.randn(N, K)) + 0.1
    w = (rng.uniform(size=(N, F)) >= 0.3).astype(np.float64)
    Yd, Dd, Xd, Wd = (torch.from_numpy(a).cuda().to(tdt) for a in (y, D, x, w))
    _arrays.l2_normalize_(Dd, strict=True)
    lib, h = _arrays.lib_handle(Dd)
    # the loop
    Dl, Xl = Dd.clone(), Xd.clone()
    assert nmf._run_emhals(Yd, Wd, Xl, Dl, 0.0, 2, penalty=pen) == 2
    # the split step
    Yi = torch.full_like(Yd, float('nan'))
    Xo = torch.full_like(Xd, float('nan'))
    stats = torch.full((K, F + K), float('nan'), dtype=tdt, device='cuda')
    Dn = torch.full_like(Dd, float('nan'))
    md = torch.zeros((2,), dtype=tdt, device='cuda')
    nmf._set_penalty(h, pen)
    try:
        _hip.check(h, getattr(lib, 'dcp_nmf_impute_' + dt)(h, _arrays.ptr(Yd), _arrays.ptr(Wd), _arrays.ptr(Xd),
                                                           _arrays.ptr(Dd), N, F, K, _arrays.ptr(Yi)),
                   'dcp_nmf_impute')
        _hip.check(h, getattr(lib, 'dcp_nmf_hals_stats_' + dt)(h, _arrays.ptr(Yi), _arrays.ptr(Xd), _arrays.ptr(Xo),
                                                               _arrays.ptr(Dd), N, F, K, _arrays.ptr(stats)),
                   'dcp_nmf_hals_stats')
        _hip.check(h, getattr(lib, 'dcp_nmf_hals_update_' + dt)(h, _arrays.ptr(stats), _arrays.ptr(Dd),
                                                                _arrays.ptr(Dn), _arrays.ptr(Xo), N, F, K,
                                                                _arrays.ptr(md[0:1]), _arrays.ptr(md[1:2])),
                   'dcp_nmf_hals_update')
    finally:
        nmf._set_penalty(h, (0.0, 0.0))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Dn).all()) and not torch.equal(Dn, Dd)
    assert torch.equal(Dn, Dl) and torch.equal(Xo, Xl)


# ---- 4. two ranks sharing the one GPU over gloo, uneven shards --------------------------------------------------
def _rank_run(rank, world, port, counts):
    import torch
    import torch.distributed as dist
    from decomp_amd import sharded
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=world,
                            timeout=timedelta(seconds=180))
    try:
        y, D0, w = _sharded_problem()
        r0 = sum(counts[:rank])
        rows = slice(r0, r0 + counts[rank])
        it, D, x = sharded.nmf_solve_sharded(torch.from_numpy(y[rows]).cuda(), torch.from_numpy(D0).cuda(), tol=TOL,
                                             maxiter=MAXITER, method='em-hals',
                                             mask_local=torch.from_numpy(w[rows]).cuda())
        kind = sharded.communicator_kind(D)
        out = (it, D.cpu().numpy(), x.cpu().numpy(), kind)
        if kind is not None:
            sharded.detach_communicator(D)
        return out
    finally:
        dist.destroy_process_group()


def _gloo_worker(q, rank, world, port, counts):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    torch.cuda.set_device(0)
    q.put((rank,) + _rank_run(rank, world, port, counts))


def test_two_ranks_uneven_shards_gloo(single):
    """Two ranks with 300 and 468 rows, the statistics all-reduced over gloo inside dcp_nmf_emhals_sharded_f32:
    both ranks take the same decision at the same iteration and hold the same D; the result is the single-process
    one up to the order of the row sums (the tolerances of the unmasked sharded HALS test)."""
    counts = [300, 468]
    y, D0, w = _sharded_problem()
    assert sum(counts) == len(y)
    it1, D1, x1 = single('f32')
    port = _free_port()
    kid = _spawn(_gloo_worker, (1, 2, port, counts))
    try:
        res = [(0,) + _rank_run(0, 2, port, counts)]
    finally:
        res_k = _finish(*kid)
    res = sorted(res + [res_k], key=lambda t: t[0])
    for r in res:
        assert r[4] == 'external', r[4]
        assert r[1] == res[0][1]
        assert np.array_equal(r[2], res[0][2])
        assert r[3].shape == (counts[r[0]], D0.shape[0])
    it = res[0][1]
    assert abs(it - it1) <= 1
    if it == it1:
        x_all = np.concatenate([r[3] for r in res], axis=0)
        assert _rel(res[0][2], D1) < 1e-4 and _rel(x_all, x1) < 1e-3


# ---- 5. error path -----------------------------------------------------------------------------------------
def test_sharded_entry_without_communicator_is_an_error():
    import torch
    from decomp_amd import _arrays, _hip
    D = torch.rand(4, 32, device='cuda')
    Y = torch.rand(16, 32, device='cuda')
    W = torch.ones(16, 32, device='cuda')
    x = torch.ones(16, 4, device='cuda')
    lib, h = _arrays.lib_handle(D)
    it = ctypes.c_int(0)
    rc = lib.dcp_nmf_emhals_sharded_f32(h, _arrays.ptr(Y), _arrays.ptr(W), _arrays.ptr(x), _arrays.ptr(D), 16, 32, 4,
                                        ctypes.c_float(0.0), 3, ctypes.byref(it), None)
    assert rc == _hip.ERR_COMM
    assert torch.equal(x, torch.ones_like(x))

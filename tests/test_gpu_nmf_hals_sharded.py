"""GPU: row-sharded HALS (nmf_solve_sharded(method='hals')): the in-library loop dcp_nmf_hals_sharded_* over a
1-rank RCCL communicator and over gloo (the external exchange), the Python loop through mu_loop and the split step
dcp_nmf_hals_stats_* / dcp_nmf_hals_update_* against a float64 NumPy HALS step.  Child processes start with the
spawn context; no test has more than 3 processes with the GPU open (in the gloo tests this process is rank 0)."""
import ctypes
import socket
from datetime import timedelta

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL, MAXITER = 2e-3, 200     # the planted problem below stops at iteration 17 (max|dD| 2.1e-3 -> 1.7e-3)


# ---- float64 NumPy restatement (as tests/test_gpu_nmf_hals.py) --------------------------------------------
def sweep_np(V, C, G):
    """for k = 0 .. K-1 in order, with the current V: where G[k,k] > 0,
    V[:,k] = max(0, V[:,k] - (V G[:,k] - C[:,k]) / G[k,k]); V [R, K], C [R, K], G [K, K]."""
    V = np.array(V, np.float64)
    C = np.asarray(C, np.float64)
    G = np.asarray(G, np.float64)
    for k in range(G.shape[0]):
        if G[k, k] > 0:
            V[:, k] = np.maximum(0.0, V[:, k] - (V.dot(G[:, k]) - C[:, k]) / G[k, k])
    return V


def hals_step_parts_np(y, x, D):
    """One HALS iteration in the split form -> (x swept, stats, D_new, x rescaled, max|D - D_new|)."""
    y, x, D = (np.asarray(a, np.float64) for a in (y, x, D))
    F = y.shape[1]
    xs = sweep_np(x, y.dot(D.T), D.dot(D.T))
    stats = np.concatenate([xs.T.dot(y), xs.T.dot(xs)], axis=1)
    Dt = sweep_np(D.T, stats[:, :F].T, stats[:, F:])
    n = np.sqrt(np.sum(Dt * Dt, axis=0))
    pos = n > 0
    D_new = Dt.T.copy()
    D_new[pos] /= n[pos][:, None]
    xr = xs.copy()
    xr[:, pos] *= n[pos]
    return xs, stats, D_new, xr, float(np.max(np.abs(D - D_new)))


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, float(np.max(np.abs(b)))))


def _sharded_problem():
    rng = np.random.RandomState(7)
    N, F, K = 768, 1536, 24
    xt = np.maximum(rng.randn(N, K), 0).astype(np.float32)
    Dt = np.maximum(rng.randn(K, F), 0).astype(np.float32)
    y = (xt @ Dt + 0.1 * np.abs(rng.randn(N, F))).astype(np.float32)
    D0 = np.maximum(Dt + 0.3 * rng.randn(K, F), 0.1).astype(np.float32)
    return y, D0


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


# ---- 1. world 1, RCCL, in-library loop --------------------------------------------------------------------
def _in_library_world1_worker(q, dt):
    import os
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.cuda.set_device(0)
    from decomp_amd import _arrays, sharded
    y, D0 = _sharded_problem()
    tdt = torch.float32 if dt == 'f32' else torch.float64
    Y = torch.from_numpy(y).cuda().to(tdt)
    D = torch.from_numpy(D0).cuda().to(tdt)
    _arrays.l2_normalize_(D, strict=True)
    x = torch.ones((Y.shape[0], D.shape[0]), dtype=tdt, device='cuda')
    assert sharded.attach_communicator(D), 'RCCL communicator could not be created on the GPU box'
    assert sharded.communicator_kind(D) == 'rccl'
    it = sharded.hals_solve_in_library(Y, x, D, TOL, MAXITER)
    torch.cuda.synchronize()
    sharded.detach_communicator(D)
    q.put((it, D.cpu().numpy(), x.cpu().numpy()))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_in_library_world1_rccl_bit_exact(dt):
    """dcp_nmf_hals_sharded_* with the all-reduce on a 1-rank RCCL communicator (the identity) reproduces
    nmf.solve(method='hals') bit for bit, stop iteration included."""
    import decomp_amd
    y, D0 = _sharded_problem()
    npdt = np.float32 if dt == 'f32' else np.float64
    it1, D1, x1 = decomp_amd.nmf.solve(y.astype(npdt), D0.astype(npdt), tol=TOL, maxiter=MAXITER, method='hals')
    assert 2 < it1 < MAXITER - 1
    p, q = _spawn(_in_library_world1_worker, (dt,))
    it, D, x = _finish(p, q)
    assert it == it1
    assert np.array_equal(D, D1) and np.array_equal(x, x1)


# ---- 2. world 1 without a communicator: the Python loop -----------------------------------------------------
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('tol,maxiter', [(TOL, MAXITER), (0.0, 6)])
def test_python_loop_world1_bit_exact(dt, tol, maxiter):
    """HipHalsStepBackend through mu_loop (stats -> update, speculative next iteration with rollback) equals
    nmf.solve(method='hals') bit for bit: converged at an inner iteration, and maxiter reached."""
    import torch
    import decomp_amd
    from decomp_amd import sharded
    y, D0 = _sharded_problem()
    npdt = np.float32 if dt == 'f32' else np.float64
    y, D0 = y.astype(npdt), D0.astype(npdt)
    it1, D1, x1 = decomp_amd.nmf.solve(y, D0.copy(), tol=tol, maxiter=maxiter, method='hals')
    if tol > 0:
        assert 2 < it1 < maxiter - 1
    else:
        assert it1 == maxiter
    Yd = torch.from_numpy(y).cuda()
    assert sharded.communicator_kind(Yd) is None
    its, Ds, xs = sharded.nmf_solve_sharded(Yd, torch.from_numpy(D0).cuda(), tol=tol, maxiter=maxiter,
                                            method='hals')
    assert its == it1
    assert np.array_equal(Ds.cpu().numpy(), D1) and np.array_equal(xs.cpu().numpy(), x1)


# ---- 3, 4. several ranks sharing the one GPU over gloo: the in-library loop, external exchange ---------------
def _rank_run(rank, world, port, counts):
    """Initialise gloo, run nmf_solve_sharded(method='hals') on this rank's rows.  Returns (it, D, x, kind)."""
    import torch
    import torch.distributed as dist
    from decomp_amd import sharded
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=world,
                            timeout=timedelta(seconds=180))
    try:
        y, D0 = _sharded_problem()
        r0 = sum(counts[:rank])
        it, D, x = sharded.nmf_solve_sharded(torch.from_numpy(y[r0:r0 + counts[rank]]).cuda(),
                                             torch.from_numpy(D0).cuda(), tol=TOL, maxiter=MAXITER, method='hals')
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


def _check_gloo(counts):
    import decomp_amd
    y, D0 = _sharded_problem()
    assert sum(counts) == len(y)
    it1, D1, x1 = decomp_amd.nmf.solve(y, D0.copy(), tol=TOL, maxiter=MAXITER, method='hals')
    world = len(counts)
    port = _free_port()
    kids = [_spawn(_gloo_worker, (r, world, port, counts)) for r in range(1, world)]
    try:
        res = [(0,) + _rank_run(0, world, port, counts)]
    finally:
        res_k = [_finish(p, q) for p, q in kids]
    res = sorted(res + res_k, key=lambda t: t[0])
    for r in res:
        assert r[4] == 'external', r[4]           # the in-library loop with the exchange as a callback
        assert r[1] == res[0][1]                  # same stop iteration on every rank
        assert np.array_equal(r[2], res[0][2])    # replicated D identical on every rank
        assert r[3].shape == (counts[r[0]], D0.shape[0])
    it = res[0][1]
    assert abs(it - it1) <= 1
    if it == it1:
        x_all = np.concatenate([r[3] for r in res], axis=0)
        assert _rel(res[0][2], D1) < 1e-4 and _rel(x_all, x1) < 1e-3


def test_two_ranks_on_one_gpu_gloo():
    """Two ranks, the statistics all-reduced over gloo inside dcp_nmf_hals_sharded_f32: every rank takes the same
    decision at the same iteration and holds the same D; the result is the single-process one up to the order
    of the row sums."""
    _check_gloo([384, 384])


def test_uneven_shards_three_ranks_gloo():
    """Three ranks with 100, 300 and 368 rows."""
    _check_gloo([100, 300, 368])


# ---- 5. the split step against NumPy ------------------------------------------------------------------------
@pytest.mark.parametrize('dt,alias,pingpong', [('f64', False, True), ('f64', True, False), ('f32', False, True),
                                               ('f32', True, False)])
def test_split_step_matches_numpy(dt, alias, pingpong):
    """dcp_nmf_hals_stats_* then dcp_nmf_hals_update_*: X_out, stats, D_new, the rescaled X and max|D - D_new|
    against a float64 NumPy HALS step; X_out aliasing X; maxdiff_next cleared (ping-pong) or not given."""
    import torch
    from decomp_amd import _arrays, _hip
    rng = np.random.RandomState(3)
    N, F, K = 300, 200, 20
    x0 = np.maximum(rng.randn(N, K), 0)
    y = x0.dot(np.maximum(rng.randn(K, F), 0)) + 0.05 * np.abs(rng.randn(N, F))
    D = np.abs(rng.randn(K, F)) + 0.05
    D /= np.sqrt(np.sum(D * D, axis=1, keepdims=True))
    x = np.abs(rng.randn(N, K)) + 0.1
    tdt = torch.float32 if dt == 'f32' else torch.float64
    npdt = np.float32 if dt == 'f32' else np.float64
    y, D, x = y.astype(npdt), D.astype(npdt), x.astype(npdt)
    Yd, Dd, Xd = (torch.from_numpy(a).cuda() for a in (y, D, x))
    Xo = Xd if alias else torch.full_like(Xd, float('nan'))
    stats = torch.full((K, F + K), float('nan'), dtype=tdt, device='cuda')
    Dn = torch.full_like(Dd, float('nan'))
    md = torch.tensor([0.0, 5.0] if pingpong else [7.0, 5.0], dtype=tdt, device='cuda')
    lib, h = _arrays.lib_handle(Dd)
    _hip.check(h, getattr(lib, 'dcp_nmf_hals_stats_' + dt)(h, _arrays.ptr(Yd), _arrays.ptr(Xd), _arrays.ptr(Xo),
                                                           _arrays.ptr(Dd), N, F, K, _arrays.ptr(stats)),
               'dcp_nmf_hals_stats')
    torch.cuda.synchronize()
    xs_gpu, stats_gpu = Xo.cpu().numpy().copy(), stats.cpu().numpy()
    _hip.check(h, getattr(lib, 'dcp_nmf_hals_update_' + dt)(h, _arrays.ptr(stats), _arrays.ptr(Dd), _arrays.ptr(Dn),
                                                            _arrays.ptr(Xo), N, F, K, _arrays.ptr(md[0:1]),
                                                            _arrays.ptr(md[1:2]) if pingpong else None),
               'dcp_nmf_hals_update')
    torch.cuda.synchronize()
    xs, st, D_new, xr, diff = hals_step_parts_np(y, x, D)
    tol = 1e-10 if dt == 'f64' else 2e-4
    assert _rel(xs_gpu, xs) < tol
    assert _rel(stats_gpu, st) < tol
    assert _rel(Dn.cpu().numpy(), D_new) < tol
    assert _rel(Xo.cpu().numpy(), xr) < tol
    m = md.cpu().numpy()
    assert abs(float(m[0]) - diff) < tol * max(diff, 1.0)
    assert float(m[1]) == (0.0 if pingpong else 5.0)
    assert alias or np.array_equal(Xd.cpu().numpy(), x)     # X untouched when X_out is another array


# ---- 6. error path -----------------------------------------------------------------------------------------
def test_sharded_entry_without_communicator_is_an_error():
    import torch
    from decomp_amd import _arrays, _hip
    D = torch.rand(4, 32, device='cuda')
    Y = torch.rand(16, 32, device='cuda')
    x = torch.ones(16, 4, device='cuda')
    lib, h = _arrays.lib_handle(D)
    it = ctypes.c_int(0)
    rc = lib.dcp_nmf_hals_sharded_f32(h, _arrays.ptr(Y), _arrays.ptr(x), _arrays.ptr(D), 16, 32, 4,
                                      ctypes.c_float(0.0), 3, ctypes.byref(it), None)
    assert rc == _hip.ERR_COMM
    assert torch.equal(x, torch.ones_like(x))


# ---- 7. one larger shard ------------------------------------------------------------------------------------
def _large_shard_worker(q):
    import os
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.cuda.set_device(0)
    from decomp_amd import _arrays, _hip, sharded
    g = torch.Generator(device='cuda')
    g.manual_seed(11)
    N, F, K = 8192, 4096, 256
    Y = torch.rand((N, F), generator=g, device='cuda')
    D0 = torch.rand((K, F), generator=g, device='cuda') + 0.05
    _arrays.l2_normalize_(D0, strict=True)
    lib, h = _arrays.lib_handle(D0)
    D1, x1 = D0.clone(), torch.ones((N, K), device='cuda')
    it1 = ctypes.c_int(0)
    _hip.check(h, lib.dcp_nmf_hals_f32(h, _arrays.ptr(Y), _arrays.ptr(x1), _arrays.ptr(D1), N, F, K,
                                       ctypes.c_float(0.0), 4, ctypes.byref(it1), None, None), 'dcp_nmf_hals_f32')
    D2, x2 = D0.clone(), torch.ones((N, K), device='cuda')
    assert sharded.attach_communicator(D2), 'RCCL communicator could not be created on the GPU box'
    it2 = sharded.hals_solve_in_library(Y, x2, D2, 0.0, 4)
    torch.cuda.synchronize()
    sharded.detach_communicator(D2)
    q.put((it1.value, it2, bool(torch.equal(D1, D2)), bool(torch.equal(x1, x2)),
           bool(torch.isfinite(D2).all()), bool(torch.equal(D1, D0))))


def test_large_shard_in_library_equals_single_gpu():
    """8192 x 4096, k = 256 (one rank's rows of the 65536-row headline shape on 8 GPUs), float32, 3 iterations:
    the in-library world-1 loop equals dcp_nmf_hals_f32 bit for bit."""
    p, q = _spawn(_large_shard_worker, ())
    it1, it2, same_d, same_x, finite, unchanged = _finish(p, q)
    assert it1 == it2 == 4
    assert finite and not unchanged
    assert same_d and same_x

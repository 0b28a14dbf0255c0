#!/usr/bin/env python3
"""Benchmark of the headline metric (BASELINE.json): NMF multiplicative-update
iterations/s at Y = 65536 x 4096, k = 256, float32, on N GPUs of one node.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A step is ONE MU iteration (x update, D update, l2_strict, max|dD| stop test) of the
whole job; rows of Y / x are sharded over the ranks (strong scaling: the problem size is
fixed) and the [K, F+K] statistics are all-reduced once per step (RCCL).  Inputs are
synthetic (SURVEY 8d recipe) and resident in HBM before the timed region.

Rank 0 prints one JSON line.  `roofline` is the dominant kernel (the fused
Y.D^T + quotient GEMM) timed with HIP events on the solver's own stream inside the timed
steps.  A plain run stops there: set-up, warm-up, timed steps, --dump-outputs, the line.
--full adds what takes work of its own after the timed steps: the per-kernel breakdown pass
(`kernel_ms_avg`, `roofline_stats_gemm`, `phase_ms`), `cpu_baseline` -- the NumPy oracle (the
reference's formulation) timed at the FULL shape on this host's cores -- with `parity`, the
per-iteration residual of the HIP path against that same oracle run on the timed run's own Y
(N = 1, rank 0 only), and `secondary`, the side measurements of the other BASELINE configs.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_ROWS, N_FEAT, N_ATOMS = 65536, 4096, 256
PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: dense fp32 MFMA peak
PEAK_HBM_GBS = 8000.0


def synth(n_rows, rank_seed, device):
    """SURVEY 8(d), C2, with np.random.RandomState on the HOST (the generator the CPU and GPU runs share):
    Dt = max(randn(K, F), 0), xt = max(randn(N, K), 0), Y = xt.Dt + 0.1 |randn| (>= 0),
    D0 = max(Dt + 0.3 randn, 0.1), float32.  Dt / D0 come from RandomState(1234) on every rank, a rank's rows
    from RandomState(99 + rank).  Data synthesis only: the product xt.Dt is formed by the host BLAS, the arrays
    are copied to HBM before anything is timed."""
    import numpy as np
    import torch
    rs = np.random.RandomState(1234)
    Dt = np.maximum(rs.randn(N_ATOMS, N_FEAT), 0).astype(np.float32)
    D0 = np.maximum(Dt + 0.3 * rs.randn(N_ATOMS, N_FEAT), 0.1).astype(np.float32)
    rs = np.random.RandomState(99 + rank_seed)
    xt = np.maximum(rs.randn(n_rows, N_ATOMS), 0).astype(np.float32)
    Y = xt @ Dt
    del xt
    block = 8192                                # noise in row blocks: bounded host temporaries
    for r0 in range(0, n_rows, block):
        r1 = min(n_rows, r0 + block)
        Y[r0:r1] += (0.1 * np.abs(rs.randn(r1 - r0, N_FEAT))).astype(np.float32)
    return torch.from_numpy(Y).to(device), torch.from_numpy(D0).to(device)


DUMP_X_ROWS = 16384         # --dump-outputs: rows of x written (a fixed, seeded sample when x has more)


def dump_outputs(out_dir, D, x, seed=0):
    """--dump-outputs: what a caller of the timed path receives after its last timed step, as float32 .npy files
    for an output-by-output comparison of two builds.  D.npy is the whole dictionary [K, F]; x.npy holds the codes
    [rows, K] whole when rows <= DUMP_X_ROWS, else the rows listed in x_rows.npy (float64 indices: a sample drawn
    from RandomState(seed), in ascending order, the same for every run with the same arguments).  At the headline
    shape: 4 MiB + 16 MiB + 128 KiB.  Returns {name: shape}."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    rows = x.shape[0]
    arrays = {'D': D.detach().float().cpu().numpy()}
    if rows <= DUMP_X_ROWS:
        arrays['x'] = x.detach().float().cpu().numpy()
    else:
        idx = np.sort(np.random.RandomState(seed).choice(rows, DUMP_X_ROWS, replace=False))
        arrays['x'] = x[torch.from_numpy(idx).to(x.device)].float().cpu().numpy()
        arrays['x_rows'] = idx.astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + '.npy'), np.ascontiguousarray(a))
    return {name: list(a.shape) for name, a in arrays.items()}


def pmc_traffic(kernel_key):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC
    summary (profiles/*_pmc_summary.json: (c*FETCH_SIZE + WRITE_SIZE)*1024, separate --pmc
    passes; c = the gfx950 FETCH_SIZE correction of MI355X_MICROARCH.md, 2.0 for wide
    coalesced reads and 1.10 as calibrated for the K-contiguous panel loader's 64-byte row
    segments, profiles/r01_fetch_calibration.txt).  PMC counters cannot be read inside this
    process, so the number is the one measured by tools/profile_round.sh on this same
    command at N = 1; None when no summary is committed."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, 'profiles', '*_pmc_summary.json')))
    if not files:
        return None, 'no committed PMC summary'
    try:
        d = json.load(open(files[-1]))
        for k, v in d.items():
            if kernel_key in k and 'hbm_bytes_corrected' in v:
                return v['hbm_bytes_corrected'], ('from %s (N=1 run; FETCH_SIZE x %.2f as calibrated for this loader, '
                                                  'profiles/r01_fetch_calibration.txt; with the guide\'s x2 for wide '
                                                  'reads: %.4g B)' % (os.path.basename(files[-1]),
                                                                     v.get('fetch_correction_factor', 2.0),
                                                                     v.get('hbm_bytes_guide_x2', float('nan'))))
    except Exception as e:  # pragma: no cover
        return None, 'unreadable PMC summary: %s' % e
    return None, 'kernel not in PMC summary'


def host_cpu_info():
    """(model name, physical cores inside this process's affinity mask, logical cpus in the mask)."""
    try:
        affinity = sorted(os.sched_getaffinity(0))
    except AttributeError:
        affinity = list(range(os.cpu_count() or 1))
    model, cores = 'unknown', set()
    try:
        cur = {}
        for line in open('/proc/cpuinfo'):
            if ':' in line:
                k, v = [t.strip() for t in line.split(':', 1)]
                cur[k] = v
                if k == 'model name':
                    model = v
            elif cur:
                if int(cur.get('processor', -1)) in affinity:
                    cores.add((cur.get('physical id', '0'), cur.get('core id', cur.get('processor'))))
                cur = {}
        if cur and int(cur.get('processor', -1)) in affinity:
            cores.add((cur.get('physical id', '0'), cur.get('core id', cur.get('processor'))))
    except Exception:
        pass
    return model, (len(cores) or len(affinity)), len(affinity)


def cgroup_cpu_quota():
    """CPUs this container may use per scheduling period (cgroup v2 cpu.max / v1 cfs quota), or None when unlimited.
    Threads beyond it do not add throughput: the kernel throttles the whole group for the rest of the period
    (the GPU boxes of this pool: 16 CPUs on a 256-thread host)."""
    try:
        q, per = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
        if q != 'max':
            return float(q) / float(per)
    except Exception:
        pass
    try:
        q = float(open('/sys/fs/cgroup/cpu/cpu.cfs_quota_us').read())
        per = float(open('/sys/fs/cgroup/cpu/cpu.cfs_period_us').read())
        if q > 0:
            return q / per
    except Exception:
        pass
    return None


def host_residual(y, x, d, block=8192):
    """||y - x d||_F with float64 accumulation, evaluated on the host in row blocks (the same
    function scores the GPU's and the oracle's iterates, so a difference can only come from x, D)."""
    import numpy as np
    acc = 0.0
    for r0 in range(0, y.shape[0], block):
        r = y[r0:r0 + block] - x[r0:r0 + block].dot(d)
        acc += float(np.sum(np.square(r, dtype=np.float64)))
    return acc ** 0.5


def parity_and_cpu_baseline(torch, lib, h, Y, D0, timed_iters=3):
    """SURVEY 8(d) "parity gates run with every benchmark" + the CPU baseline, both at the FULL
    configs[1] shape on the very Y the GPU was timed on:
      * the NumPy oracle (oracle.nmf.mu_step: the reference's 6-GEMM formulation, grads.py:108-125,
        batch_mu.py:16-24) and the HIP path each run 1 + timed_iters MU iterations from the same
        (Y, D0, x = ones); after every iteration ||Y - x D||_F of both is evaluated on the host by
        the same function and must agree to 1e-5 relative (north_star);
      * cpu_baseline = the oracle's measured seconds per iteration over the last `timed_iters`
        iterations (the first one warms up BLAS threads and page faults), BLAS threads = physical
        cores of this process's affinity mask."""
    import numpy as np
    from decomp_amd import _arrays, _hip
    from oracle import nmf as onmf, common
    model, phys, logical = host_cpu_info()
    quota = cgroup_cpu_quota()
    want = phys if quota is None else max(1, min(phys, int(quota)))     # no more BLAS threads than CPUs we may use
    threads, blas, limiter = want, 'unknown', None
    try:
        from threadpoolctl import threadpool_info, threadpool_limits
        pools = [p for p in threadpool_info() if p.get('user_api') == 'blas']
        if pools:
            blas = '%s %s' % (pools[0].get('internal_api'), pools[0].get('version'))
        limiter = threadpool_limits(limits=want, user_api='blas')
        pools = [p for p in threadpool_info() if p.get('user_api') == 'blas']
        if pools:   # what the BLAS really runs with (a build-time thread cap may sit below `phys`)
            threads = int(max(p.get('num_threads', 1) for p in pools))
    except Exception:
        pass
    n_rows = Y.shape[0]
    y = Y.cpu().numpy()
    d0 = D0.cpu().numpy()
    n_it = 1 + timed_iters
    # ---- HIP path, one iteration per call (dcp_nmf_mu with maxiter = 2) ----
    xg = torch.ones((n_rows, N_ATOMS), dtype=torch.float32, device=Y.device)
    Dg = D0.clone()
    _arrays.l2_normalize_(Dg, strict=True)                      # nmf.py:70
    it = ctypes.c_int(0)
    gpu_iter = []
    for _ in range(n_it):
        _hip.check(h, lib.dcp_nmf_mu_f32(h, _arrays.ptr(Y), None, _arrays.ptr(xg), _arrays.ptr(Dg), n_rows,
                                         N_FEAT, N_ATOMS, _hip.LIK_L2, ctypes.c_float(0.0), 2,
                                         ctypes.byref(it), None, None), 'dcp_nmf_mu_f32 (parity)')
        gpu_iter.append((xg.cpu().numpy(), Dg.cpu().numpy()))
    del xg, Dg
    # ---- oracle ----
    x = np.ones((n_rows, N_ATOMS), np.float32)
    d = common.l2_strict(d0)
    res_cpu, res_gpu, times = [], [], []
    for i in range(n_it):
        t0 = time.perf_counter()
        x, d, _ = onmf.mu_step(y, x, d)
        times.append(time.perf_counter() - t0)
        res_cpu.append(host_residual(y, x, d))
        res_gpu.append(host_residual(y, *gpu_iter[i]))
    if limiter is not None:
        limiter.restore_original_limits()
    rel = [abs(a - b) / b for a, b in zip(res_gpu, res_cpu)]
    per_iter = sum(times[1:]) / max(1, len(times) - 1)
    tol = 1.0e-5
    parity = {'shape': '%dx%d k=%d fp32' % (n_rows, N_FEAT, N_ATOMS), 'iterations': n_it,
              'metric': '||Y - x D||_F after each MU iteration, HIP path vs NumPy oracle '
                        '(oracle.nmf.mu_step), both evaluated on the host',
              'rel_err': [float('%.3e' % r) for r in rel], 'rel_err_max': max(rel),
              'residual_oracle': res_cpu, 'residual_hip': res_gpu, 'tolerance': tol,
              'pass': bool(max(rel) <= tol)}
    base = {'value': 1.0 / per_iter, 'unit': 'iterations/s', 'cores': threads, 'kind': 'port',
            'blas': blas, 'cpu_model': model, 'physical_cores': phys, 'affinity_cpus': logical,
            'cgroup_cpu_quota': quota,
            's_per_iteration': per_iter,
            'sample': 'oracle.nmf.mu_step (NumPy/BLAS, reference 6-GEMM formulation) at the FULL '
                      '%dx%d k=%d fp32 shape on the GPU run\'s own Y: %d timed iterations after 1 '
                      'warm-up (%.1f s), %d BLAS threads (physical cores %d, container CPU quota %s)'
                      % (n_rows, N_FEAT, N_ATOMS, len(times) - 1, sum(times), threads, phys,
                         'none' if quota is None else '%g CPUs' % quota)}
    return parity, base


def dict_step_parity(torch, lib, h, step_name, Y, D, alpha=0.1, lasso_iter=10, lasso_tol=1e-5):
    """ONE dictionary-learning minibatch step (dictionary_learning.py:135-164) from the reference's
    starting state (x = 1, A = B = 0, count = 0) through dcp_dict_step_* and through the NumPy oracle
    (oracle.dictionary_learning.minibatch_step: lasso.solve_fastpath ista + A, B + sequential atom
    sweep) on the host copy of the very arrays the step is timed on: identical LASSO iteration count,
    x and D_new within 2e-4 of the largest entry (single precision)."""
    import numpy as np
    from decomp_amd import _arrays, _hip
    from oracle import dictionary_learning as odl
    MB, F = Y.shape
    K = D.shape[0]
    x = torch.ones((MB, K), device=Y.device, dtype=D.dtype)
    A = torch.zeros((K, K), device=Y.device, dtype=D.dtype)
    B = torch.zeros((K, F), device=Y.device, dtype=D.dtype)
    Dn = torch.empty_like(D)
    md, lit = ctypes.c_double(0), ctypes.c_int(0)
    _hip.check(h, getattr(lib, step_name)(h, _arrays.ptr(Y), _arrays.ptr(x), _arrays.ptr(D), _arrays.ptr(Dn),
                                          _arrays.ptr(A), _arrays.ptr(B), MB, F, K, (1.0 - MB) / 1.0, alpha,
                                          _hip.LASSO_ISTA, lasso_iter, lasso_tol, ctypes.byref(md),
                                          ctypes.byref(lit)), step_name + ' (parity)')
    gx, gD = x.cpu().numpy(), Dn.cpu().numpy()
    y, d = Y.cpu().numpy(), D.cpu().numpy()
    t0 = time.perf_counter()
    it2, ox, _, _, oD, odiff = odl.minibatch_step(y, np.ones((MB, K), y.dtype), d, np.zeros((K, K), y.dtype),
                                                  np.zeros((K, F), y.dtype), 0, MB, alpha, 'ista', lasso_iter,
                                                  lasso_tol)
    cpu_s = time.perf_counter() - t0
    ex = float(np.max(np.abs(gx - ox))) / float(np.max(np.abs(ox)))
    eD = float(np.max(np.abs(gD - oD))) / float(np.max(np.abs(oD)))
    tol = 2.0e-4
    return {'metric': 'one minibatch step from x=1, A=B=0: HIP vs NumPy oracle (oracle.dictionary_learning.'
                      'minibatch_step), max|diff| / max|oracle|',
            'lasso_it_hip': lit.value, 'lasso_it_oracle': int(it2), 'x_rel_err': ex, 'D_rel_err': eD,
            'maxdiff_hip': md.value, 'maxdiff_oracle': odiff, 'code_density': float((ox != 0).mean()),
            'tolerance': tol, 'oracle_s_per_step': cpu_s,
            'pass': bool(lit.value == it2 and ex <= tol and eD <= tol)}


def dict_step_cd_parity(torch, lib, h, Y, D, alpha=0.1, lasso_iter=10, lasso_tol=1e-5, n_rows=16):
    """The same gate for the reference's DEFAULT inner solver (lasso_method='cd').  The reference's sweep
    recomputes x.A for every coordinate (lasso.py:539-551: 1.8e14 flop for this minibatch), so the oracle runs
    stage-wise: its as-written coordinate descent on `n_rows` rows spread over the minibatch pins the codes
    (rows are independent given D; from x = 1 the stop test at sweep 0 cannot fire), and A, B + the sequential
    atom sweep of the oracle, fed with the HIP path's codes, pin the D side."""
    import numpy as np
    from decomp_amd import _arrays, _hip
    from oracle import dictionary_learning as odl, lasso as olasso
    MB, F = Y.shape
    K = D.shape[0]
    x = torch.ones((MB, K), device=Y.device, dtype=D.dtype)
    A = torch.zeros((K, K), device=Y.device, dtype=D.dtype)
    B = torch.zeros((K, F), device=Y.device, dtype=D.dtype)
    Dn = torch.empty_like(D)
    md, lit = ctypes.c_double(0), ctypes.c_int(0)
    _hip.check(h, lib.dcp_dict_step_f32(h, _arrays.ptr(Y), _arrays.ptr(x), _arrays.ptr(D), _arrays.ptr(Dn),
                                        _arrays.ptr(A), _arrays.ptr(B), MB, F, K, (1.0 - MB) / 1.0, alpha,
                                        _hip.LASSO_CD, lasso_iter, lasso_tol, ctypes.byref(md), ctypes.byref(lit)),
               'dcp_dict_step_f32 (cd parity)')
    gx, gD = x.cpu().numpy(), Dn.cpu().numpy()
    y, d = Y.cpu().numpy(), D.cpu().numpy()
    sel = np.arange(0, MB, max(1, MB // n_rows))
    t0 = time.perf_counter()
    it2, xs = olasso.solve_fastpath(y[sel], d, alpha, x=np.ones((len(sel), K), y.dtype), tol=lasso_tol,
                                    maxiter=lasso_iter, method='cd')
    cpu_s = time.perf_counter() - t0
    beta = (1.0 - MB) / 1.0
    oD = odl.atom_sweep(d, beta * np.zeros((K, K), y.dtype) + gx.T @ gx, beta * np.zeros((K, F), y.dtype) + gx.T @ y)
    ex = float(np.max(np.abs(gx[sel] - xs))) / float(np.max(np.abs(xs)))
    eD = float(np.max(np.abs(gD - oD))) / float(np.max(np.abs(oD)))
    tol = 2.0e-4
    return {'metric': 'one minibatch step, lasso_method=cd: codes of %d rows vs the oracle\'s as-written sweep; '
                      'D_new vs the oracle\'s A, B + atom sweep on the HIP codes; max|diff| / max|oracle|' % len(sel),
            'lasso_it_hip': lit.value, 'lasso_it_oracle': int(it2), 'x_rel_err': ex, 'D_rel_err': eD,
            'tolerance': tol, 'oracle_s': cpu_s, 'pass': bool(lit.value == it2 and ex <= tol and eD <= tol)}


def secondary_configs(torch, device, with_oracle=False):
    """The other BASELINE configs at their one-GPU shapes, measured live in a few seconds each (they
    are parity-test cases, not the headline; reported so that their numbers in DESIGN.md have a
    driver-side record).  Synthetic data of SURVEY 8d's recipes.  with_oracle: also check one dictionary
    step of configs[2] / configs[4] against the NumPy oracle at the timed shape (dict_step_parity)."""
    from decomp_amd import _arrays, _hip
    out = {}
    g = torch.Generator(device=device)
    g.manual_seed(2)

    def ms_of(fn, reps):
        # the side measurements run after ~20 s of host-only work (the CPU oracle): give the GPU
        # ~0.25 s of the same kernels to come back to its working clocks before timing
        t_end = time.perf_counter() + 0.25
        while True:
            fn()
            torch.cuda.synchronize()
            if time.perf_counter() >= t_end:
                break
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    # configs[2]: one dictionary-learning minibatch step, 8192 x 4096, k = 512, ista x 10, fp32
    MB, F, K = 8192, 4096, 512
    Dt = torch.randn((K, F), generator=g, device=device)
    xt = 30.0 * torch.randn((MB, K), generator=g, device=device) * \
        (torch.rand((MB, K), generator=g, device=device) < 0.05)
    Y = xt @ Dt + 0.1 * torch.randn((MB, F), generator=g, device=device)
    D = Dt + 0.2 * torch.randn((K, F), generator=g, device=device)
    _arrays.l2_normalize_(D, strict=True)
    x = torch.ones((MB, K), device=device)
    A = torch.zeros((K, K), device=device)
    B = torch.zeros((K, F), device=device)
    D_new = torch.empty_like(D)
    lib, h = _arrays.lib_handle(D)
    md, lit = ctypes.c_double(0), ctypes.c_int(0)
    dl_parity = dict_step_parity(torch, lib, h, 'dcp_dict_step_f32', Y, D) if with_oracle else None
    cd_parity = dict_step_cd_parity(torch, lib, h, Y, D) if with_oracle else None
    state = {'D': D, 'Dn': D_new, 'count': 0}

    def dl_step(method=_hip.LASSO_ISTA):
        theta = state['count'] * MB + 1.0
        _hip.check(h, lib.dcp_dict_step_f32(h, _arrays.ptr(Y), _arrays.ptr(x), _arrays.ptr(state['D']),
                                            _arrays.ptr(state['Dn']), _arrays.ptr(A), _arrays.ptr(B), MB, F, K,
                                            (theta - MB) / theta, 0.1, method, 10, 1e-5,
                                            ctypes.byref(md), ctypes.byref(lit)), 'dict_step')
        state['D'], state['Dn'] = state['Dn'], state['D']
        state['count'] += 1
    out['dictionary_step_ms'] = {'workload': 'configs[2] minibatch 8192x4096 k=512 ista x10 fp32',
                                 'value': round(ms_of(dl_step, 6), 4)}
    def dl_roofline(ms, MB_, F_, K_, iters, cplx):
        # LASSO (2 N F K + 2 K^2 F + iters 2 N K^2) + x^H x (2 N K^2) + x^H y (2 N K F) + sweep (2 K^2 F)
        fl = 2.0 * MB_ * F_ * K_ + 2.0 * K_ * K_ * F_ + iters * 2.0 * MB_ * K_ * K_ + 2.0 * MB_ * K_ * K_ + \
            2.0 * MB_ * K_ * F_ + 2.0 * K_ * K_ * F_
        if cplx:
            fl *= 4.0
        ach = fl / (ms * 1e-3) / 1e12
        return {'bound': 'mfma', 'scope': 'whole minibatch step (all kernels)', 'flops_per_step': fl,
                'achieved': ach, 'peak': PEAK_F32_MFMA_TFLOPS, 'unit': 'TFLOP/s', 'frac': ach / PEAK_F32_MFMA_TFLOPS}
    out['dictionary_step_ms']['roofline'] = dl_roofline(out['dictionary_step_ms']['value'], MB, F, K, 10, False)
    # The same step through dcp_dict_step_async_f32, the entry dictionary_learning.solve() drives: max|dD| lands in
    # pinned host memory and is read ONE STEP LATE, so the host never waits for the GPU between steps (the blocking
    # entry above returns max|dD| and so carries a host round trip per step: ~60 us of idle GPU in the kernel trace).
    md_pin = torch.zeros((2,), dtype=torch.float32).pin_memory()
    md_np = md_pin.numpy()

    def dl_step_async(method=_hip.LASSO_ISTA):
        c = state['count']
        theta = c * MB + 1.0
        md_np[c & 1] = -1.0
        _hip.check(h, lib.dcp_dict_step_async_f32(h, _arrays.ptr(Y), _arrays.ptr(x), _arrays.ptr(state['D']),
                                                  _arrays.ptr(state['Dn']), _arrays.ptr(A), _arrays.ptr(B), MB, F, K,
                                                  (theta - MB) / theta, 0.1, method, 10, 1e-5,
                                                  _arrays.ptr(md_pin[(c & 1):(c & 1) + 1]), ctypes.byref(lit)),
                   'dict_step_async')
        if state.get('primed'):
            while md_np[(c & 1) ^ 1] == -1.0:     # the previous step's max|dD| (a stop test would read it here)
                pass
        state['primed'] = True
        state['D'], state['Dn'] = state['Dn'], state['D']
        state['count'] += 1
    out['dictionary_step_ms']['async_entry_ms'] = round(ms_of(dl_step_async, 12), 4)
    out['dictionary_step_ms']['async_entry_roofline_frac'] = round(
        dl_roofline(out['dictionary_step_ms']['async_entry_ms'], MB, F, K, 10, False)['frac'], 4)
    if dl_parity is not None:
        out['dictionary_step_ms']['parity'] = dl_parity
    # the same step with the reference's DEFAULT inner solver (dictionary_learning.py:14, lasso_method='cd'),
    # codes carried over from the previous visit of the minibatch as in the reference's epochs
    out['dictionary_step_cd_ms'] = {'workload': "configs[2] minibatch 8192x4096 k=512 cd x10 fp32",
                                    'value': round(ms_of(lambda: dl_step(_hip.LASSO_CD), 6), 4)}
    out['dictionary_step_cd_ms']['async_entry_ms'] = round(ms_of(lambda: dl_step_async(_hip.LASSO_CD), 12), 4)
    if cd_parity is not None:
        out['dictionary_step_cd_ms']['parity'] = cd_parity
    del Y, x, A, B, D_new, xt

    # configs[2] END TO END through the public API: decomp_amd.dictionary_learning.solve on device
    # tensors, Y 65536 x 4096, k = 512, minibatch 8192, ista x 10, maxiter = 4 -> 3 epochs = 24 minibatch steps,
    # wall clock / 24 -- shuffle, per-step row gathers, stop test and the final copy-out included.
    import decomp_amd
    NT = 65536
    xt = 30.0 * torch.randn((NT, K), generator=g, device=device) * (torch.rand((NT, K), generator=g, device=device) < 0.05)
    Yfull = xt @ Dt
    del xt
    for r0 in range(0, NT, 8192):
        Yfull[r0:r0 + 8192] += 0.1 * torch.randn((8192, F), generator=g, device=device)
    kw = dict(tol=0.0, minibatch=MB, lasso_method='ista', lasso_iter=10, lasso_tol=1e-5, random_seed=0)
    decomp_amd.dictionary_learning.solve(Yfull, D, 0.1, maxiter=2, **kw)          # warm-up: one epoch
    torch.cuda.synchronize()

    def throttled_periods():
        try:
            for ln in open('/sys/fs/cgroup/cpu.stat'):
                if ln.startswith('nr_throttled'):
                    return int(ln.split()[1])
        except Exception:
            pass
        return None
    # as for every side measurement (ms_of): ~0.25 s of the same work first, so that the GPU is at its working
    # clocks -- the host-only data synthesis above let it fall back
    t_end = time.perf_counter() + 0.25
    while time.perf_counter() < t_end:
        decomp_amd.dictionary_learning.solve(Yfull, D, 0.1, maxiter=4, **kw)
        torch.cuda.synchronize()
    thr0 = throttled_periods()
    e2e_samples = []
    for _ in range(3):      # three identical calls: the median is reported, every sample is listed
        t0 = time.perf_counter()
        it_e2e, D_e2e, x_e2e = decomp_amd.dictionary_learning.solve(Yfull, D, 0.1, maxiter=4, **kw)
        torch.cuda.synchronize()
        e2e_samples.append(1e3 * (time.perf_counter() - t0) / (3 * (NT // MB)))
    e2e_ms = sorted(e2e_samples)[1]
    # the same call with maxiter = 13 (12 epochs = 96 steps): the per-call cost -- the first permutation of 65536 row
    # indices on the host, allocations, pipeline fill and drain, ~2 ms -- spread over a call of realistic length
    # (the reference's default is maxiter = 1000)
    t0 = time.perf_counter()
    it_long, D_long, x_long = decomp_amd.dictionary_learning.solve(Yfull, D, 0.1, maxiter=13, **kw)
    torch.cuda.synchronize()
    e2e_long_ms = 1e3 * (time.perf_counter() - t0) / (12 * (NT // MB))
    out['dictionary_learning_solve_ms_per_step'] = {
        'workload': 'configs[2] END TO END: decomp_amd.dictionary_learning.solve(Y 65536x4096 fp32 on the device, k=512, '
                    'minibatch=8192, lasso_method=ista, lasso_iter=10, maxiter=4): wall clock of the call / 24 steps, median of 3 calls',
        'value': round(e2e_ms, 4), 'samples_ms': [round(v, 4) for v in e2e_samples], 'it': int(it_e2e),
        'finite': bool(torch.isfinite(D_e2e).all().item()) and bool(torch.isfinite(x_e2e).all().item()),
        'code_density': float((x_e2e != 0).float().mean().item()),
        'vs_step_kernel_figure': round(e2e_ms / out['dictionary_step_ms']['value'], 4),
        'maxiter_13_96_steps': {'value': round(e2e_long_ms, 4), 'it': int(it_long),
                                'finite': bool(torch.isfinite(D_long).all().item()),
                                'vs_step_kernel_figure': round(e2e_long_ms / out['dictionary_step_ms']['value'], 4),
                                'vs_async_step': round(e2e_long_ms / out['dictionary_step_ms']['async_entry_ms'], 4)},
        'vs_async_step': round(e2e_ms / out['dictionary_step_ms']['async_entry_ms'], 4)}
    thr1 = throttled_periods()
    if thr0 is not None and thr1 is not None:
        # CFS periods in which this container was throttled while the end-to-end calls ran (0 on a quiet run; a
        # throttled launching thread shows up as tens of ms in one sample)
        out['dictionary_learning_solve_ms_per_step']['cgroup_throttled_periods'] = thr1 - thr0
    del D_long, x_long
    del Yfull, D_e2e, x_e2e, D, Dt

    # configs[3]: masked NMF MU, one GPU's shard 16384 x 4096, k = 256, 20 % missing, fp32
    N, F, K = 16384, 4096, 256
    Dt = torch.randn((K, F), generator=g, device=device).clamp_(min=0)
    xt = torch.randn((N, K), generator=g, device=device).clamp_(min=0)
    Y = xt @ Dt + 0.1 * torch.randn((N, F), generator=g, device=device).abs_()
    D = (Dt + 0.3 * torch.randn((K, F), generator=g, device=device)).clamp_(min=0.1)
    mask = (torch.rand((N, F), generator=g, device=device) >= 0.2).float()
    _arrays.l2_normalize_(D, strict=True)
    x = torch.ones((N, K), device=device)
    it = ctypes.c_int(0)

    def masked(n=5):
        _hip.check(h, lib.dcp_nmf_mu_f32(h, _arrays.ptr(Y), _arrays.ptr(mask), _arrays.ptr(x), _arrays.ptr(D),
                                         N, F, K, _hip.LIK_L2, ctypes.c_float(0.0), n + 1, ctypes.byref(it),
                                         None, None), 'nmf_mu masked')
    ms = ms_of(masked, 2) / 5
    out['masked_nmf_ms_per_iter'] = {'workload': 'configs[3] shard 16384x4096 k=256 20% mask fp32',
                                     'value': round(ms, 4),
                                     'tflops_on_12NKF': round(12.0 * N * K * F / ms / 1e9, 1)}
    # float64 (the reference's default dtype) on the fp64 MFMA core, same shard shape, no mask
    Yd, Dd = Y.double(), D.double()
    xd = torch.ones((N, K), device=device, dtype=torch.float64)

    def f64(n=5):
        _hip.check(h, lib.dcp_nmf_mu_f64(h, _arrays.ptr(Yd), None, _arrays.ptr(xd), _arrays.ptr(Dd), N, F, K,
                                         _hip.LIK_L2, ctypes.c_double(0.0), n + 1, ctypes.byref(it), None,
                                         None), 'nmf_mu f64')
    ms = ms_of(f64, 2) / 5
    W = 4.0 * N * K * F + 4.0 * N * K * K + 4.0 * K * K * F
    out['f64_nmf_ms_per_iter'] = {'workload': '16384x4096 k=256 float64', 'value': round(ms, 4),
                                  'tflops': round(W / ms / 1e9, 1), 'fp64_peak': 78.6}
    del Yd, Dd, xd, mask
    # one 8192-row shard of configs[1] (what each GPU of an 8-GPU run computes per step, no collective)
    Ns = 8192
    Ys, xs = Y[:Ns].contiguous(), torch.ones((Ns, K), device=device)
    Ds = D.clone()

    def shard(n=10):
        _hip.check(h, lib.dcp_nmf_mu_f32(h, _arrays.ptr(Ys), None, _arrays.ptr(xs), _arrays.ptr(Ds), Ns, F, K,
                                         _hip.LIK_L2, ctypes.c_float(0.0), n + 1, ctypes.byref(it), None, None),
                   'nmf_mu shard')
    ms_plain = ms_of(shard, 3) / 10
    # the loop a rank of an 8-GPU run executes: dcp_nmf_mu_sharded_f32 with the handle's RCCL communicator
    # (here a 1-rank communicator: the all-reduce call is issued every step, its wire time is not in it)
    from decomp_amd import sharded as _sh
    ms = None
    if _sh.attach_communicator(Ds):
        def shard_rank(n=10):
            _sh.mu_solve_in_library(Ys, None, xs, Ds, _hip.LIK_L2, 0.0, n + 1)
        ms = ms_of(shard_rank, 3) / 10
        _sh.detach_communicator(Ds)
    Ws = 4.0 * Ns * K * F + 4.0 * Ns * K * K + 4.0 * K * K * F
    shipped = ms if ms is not None else ms_plain
    out['shard_8192_rows_ms_per_iter'] = {
        'workload': 'one 8192-row shard of configs[1] on one GPU through dcp_nmf_mu_sharded_f32 (the loop a rank of '
                    'an 8-GPU run executes; 1-rank RCCL communicator, so the exchange is issued but costs no wire '
                    'time)' if ms is not None else 'one 8192-row shard of configs[1], dcp_nmf_mu_f32 (RCCL unavailable)',
        'value': round(shipped, 4), 'tflops': round(Ws / shipped / 1e9, 1),
        'without_exchange_call_ms': round(ms_plain, 4),
        'compute_side_speedup_at_8_gpus': None}
    del Y, Ys, xs, Ds, x
    # the usual NMF ranks are far below the headline's 256 atoms: same Y shape as configs[1] per 16384 rows, k = 32
    # (narrow 128x32 / 32x128 tiles; the step is bound by reading Y twice)
    N, F, K = 16384, 4096, 32
    Yk = torch.rand((N, F), generator=g, device=device)
    Dk = torch.rand((K, F), generator=g, device=device) + 0.1
    _arrays.l2_normalize_(Dk, strict=True)
    xk = torch.ones((N, K), device=device)

    def rank32(n=10):
        _hip.check(h, lib.dcp_nmf_mu_f32(h, _arrays.ptr(Yk), None, _arrays.ptr(xk), _arrays.ptr(Dk), N, F, K,
                                         _hip.LIK_L2, ctypes.c_float(0.0), n + 1, ctypes.byref(it), None, None),
                   'nmf_mu k=32')
    ms = ms_of(rank32, 3) / 10
    out['rank32_nmf_ms_per_iter'] = {'workload': '16384x4096 k=32 fp32 (narrow tiles)', 'value': round(ms, 4),
                                     'hbm_gbs_on_2_reads_of_Y': round(2.0 * N * F * 4 / ms / 1e6, 0)}
    del Yk, Dk, xk
    # configs[4]: one complex64 dictionary-learning minibatch step at one GPU's shape, 8192 x 8192, k = 512
    MB, F, K = 8192, 8192, 512

    def crandn(*sh):
        return torch.complex(torch.randn(sh, generator=g, device=device), torch.randn(sh, generator=g, device=device))
    Dt = crandn(K, F)
    xt = 30.0 * crandn(MB, K) * (torch.rand((MB, K), generator=g, device=device) < 0.05)
    Yc = xt @ Dt + 0.1 * crandn(MB, F)
    Dc = Dt + 0.2 * crandn(K, F)
    del xt, Dt
    _arrays.l2_normalize_(Dc, strict=True)
    xc = torch.ones((MB, K), device=device, dtype=torch.complex64)
    Ac = torch.zeros((K, K), device=device, dtype=torch.complex64)
    Bc = torch.zeros((K, F), device=device, dtype=torch.complex64)
    c_parity = dict_step_parity(torch, lib, h, 'dcp_dict_step_c64', Yc, Dc) if with_oracle else None
    cstate = {'D': Dc, 'Dn': torch.empty_like(Dc), 'count': 0}

    def dl_c64():
        theta = cstate['count'] * MB + 1.0
        _hip.check(h, lib.dcp_dict_step_c64(h, _arrays.ptr(Yc), _arrays.ptr(xc), _arrays.ptr(cstate['D']),
                                            _arrays.ptr(cstate['Dn']), _arrays.ptr(Ac), _arrays.ptr(Bc), MB, F, K,
                                            (theta - MB) / theta, 0.1, _hip.LASSO_ISTA, 10, 1e-5,
                                            ctypes.byref(md), ctypes.byref(lit)), 'dict_step c64')
        cstate['D'], cstate['Dn'] = cstate['Dn'], cstate['D']
        cstate['count'] += 1
    out['complex_dictionary_step_ms'] = {'workload': 'configs[4] minibatch 8192x8192 complex64 k=512 ista x10',
                                         'value': round(ms_of(dl_c64, 4), 4)}
    out['complex_dictionary_step_ms']['roofline'] = dl_roofline(out['complex_dictionary_step_ms']['value'], MB, F, K,
                                                               10, True)
    if c_parity is not None:
        out['complex_dictionary_step_ms']['parity'] = c_parity
    del Yc, Dc, xc, Ac, Bc
    # the reference's OWN benchmark shapes (speed_tests/tests/test_nmf.py:14-66, test_lasso.py:8-59), small enough
    # that launch latency decides: the drop-in on device arrays beside the NumPy oracle on this host's cores
    try:
        import importlib.util
        spec = importlib.util.spec_from_file_location('ref_speed_shapes', os.path.join(ROOT, 'tools', 'ref_speed_shapes.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        out['reference_speed_shapes'] = mod.run(with_cpu=with_oracle)
    except Exception as e:      # a side measurement never costs the headline line
        out['reference_speed_shapes'] = {'error': repr(e)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--full', action='store_true',
                    help='after the headline figure, also run the per-kernel breakdown pass, the full-shape '
                         'oracle parity gate with the CPU baseline and the side measurements of the other '
                         'BASELINE configs')
    ap.add_argument('--no-cpu-baseline', action='store_true',
                    help='with --full: skip the oracle parity gate and the CPU baseline')
    ap.add_argument('--no-secondary', action='store_true',
                    help='with --full: skip the few-second side measurements of the other BASELINE configs')
    ap.add_argument('--no-kernel-events', action='store_true',
                    help='(analysis only) do not bracket kernel groups with hipEvents in the timed steps')
    ap.add_argument('--force-sharded', action='store_true',
                    help='(analysis only) use the multi-GPU Python step loop even at N = 1')
    ap.add_argument('--rows', type=int, default=0,
                    help='(analysis only) rows of Y on this GPU instead of 65536/N: time one '
                         'shard of a larger run without the collective')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write the D and x they produced to DIR/<name>.npy (float32; '
                         'x as a fixed, seeded row sample at the full shape; rank 0 only)')
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be >= 1 and --warmup >= 0')

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # `python bench.py --gpus N` as ONE command: this parent has made no GPU call (torch is not even
        # imported yet); it starts the N ranks (one process per GPU) and exits with their return code.
        # Rank 0's JSON line goes to the inherited stdout.
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(('127.0.0.1', 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus),
               '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.run(cmd).returncode)

    import torch
    import torch.distributed as dist
    from decomp_amd import _arrays, _hip, sharded

    # torch's CPU thread pool defaults to one thread per host CPU (256 here) whatever the container's quota (16):
    # its workers spin after every parallel region and get the whole cgroup throttled -- the launching thread then
    # sits out the rest of the 100 ms period (profiles/r04_dictionary_learning_e2e.txt).  Cap it like the BLAS pool.
    quota0 = cgroup_cpu_quota()
    if quota0:
        torch.set_num_threads(max(1, min(torch.get_num_threads(), int(quota0))))

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    args.gpus = world
    # one rank per GPU; DCP_DIST_BACKEND=gloo lets several ranks share one GPU (rehearsal of the
    # launch path on a 1-GPU box -- never a measurement)
    backend = os.environ.get('DCP_DIST_BACKEND', 'nccl')
    dev_index = local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(dev_index)
    device = torch.device('cuda', dev_index)
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if backend == 'nccl':
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    rows = N_ROWS // world
    if args.rows:
        rows = args.rows
    Y, D0 = synth(rows, rank, device)
    x = torch.ones((rows, N_ATOMS), dtype=torch.float32, device=device)
    state = {'x': x}
    D = D0.clone()
    _arrays.l2_normalize_(D, strict=True)
    torch.cuda.synchronize()

    lib, h = _arrays.lib_handle(D)
    # Multi-GPU (and --force-sharded on one GPU): the loop a rank runs is dcp_nmf_mu_sharded_f32 -- the step
    # with the RCCL all-reduce of the statistics enqueued on the solver's own stream inside the library.  Only
    # when RCCL cannot serve the process group (DCP_DIST_BACKEND=gloo rehearsals: several ranks on one GPU)
    # does the Python loop over torch.distributed run instead; the JSON line says which (`config.loop`).
    sharded_run = world > 1 or args.force_sharded
    in_library = sharded_run and sharded.attach_communicator(D)
    kind = sharded.communicator_kind(D) if in_library else None
    loop_name = ('single-GPU dcp_nmf_mu_f32' if not sharded_run else
                 'in-library dcp_nmf_mu_sharded_f32 (ncclAllReduce on the solver stream)' if kind == 'rccl' else
                 'in-library dcp_nmf_mu_sharded_f32, exchange through a host callback over torch.distributed (%s): '
                 'a rehearsal, never a measurement' % backend if kind == 'external' else
                 'python sharded.mu_loop over torch.distributed (%s)' % backend)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    def run(n_steps):
        """n_steps MU iterations (tol = 0: the stop test is evaluated, never met)."""
        if not sharded_run:
            it = ctypes.c_int(0)
            rc = lib.dcp_nmf_mu_f32(h, _arrays.ptr(Y), None, _arrays.ptr(x), _arrays.ptr(D),
                                    rows, N_FEAT, N_ATOMS, _hip.LIK_L2, ctypes.c_float(0.0),
                                    n_steps + 1, ctypes.byref(it), None, None)
            _hip.check(h, rc, 'dcp_nmf_mu_f32')
            assert it.value == n_steps + 1
            return D
        if in_library:
            it = sharded.mu_solve_in_library(Y, None, state['x'], D, _hip.LIK_L2, 0.0, n_steps + 1)
            assert it == n_steps + 1
            return D
        backend = sharded.HipStepBackend(Y, None, state['x'], D, _hip.LIK_L2)
        it, Dout = sharded.mu_loop(backend, D, 0.0, n_steps + 1, world_size=world,
                                   new_like=torch.empty_like)
        assert it == n_steps + 1
        state['x'] = backend.x
        return Dout

    def read_profile():
        out = {}
        for lab in range(_hip.PROF_NLABELS):
            ms, cnt = ctypes.c_double(0), ctypes.c_int64(0)
            _hip.check(h, lib.dcp_profile_read(h, lab, ctypes.byref(ms), ctypes.byref(cnt)), 'profile_read')
            if cnt.value:
                out[lib.dcp_profile_label_name(lab).decode()] = {
                    'ms_total': ms.value, 'launches': cnt.value, 'ms_avg': ms.value / cnt.value}
        return out

    Dcur = run(args.warmup)
    if Dcur is not D:
        D.copy_(Dcur)
    # Timed region: K steps; only the DOMINANT kernel is bracketed by hipEvents inside it (a
    # bracket costs ~4 us of stream time; bracketing all eight kernel groups costs 2.5 % of a
    # step at N = 1 and 12 % on an 8192-row shard -- measured with --no-kernel-events).
    _hip.check(h, lib.dcp_profile_reset(h), 'profile_reset')
    _hip.check(h, lib.dcp_profile_select(h, 1 << _hip.PROF_XUPDATE), 'profile_select')
    _hip.check(h, lib.dcp_profile_enable(h, 0 if args.no_kernel_events else 1), 'profile_enable')
    barrier()
    t0 = time.perf_counter()
    Dcur = run(args.steps)
    barrier()
    elapsed = time.perf_counter() - t0
    _hip.check(h, lib.dcp_profile_enable(h, 0), 'profile_enable')

    t = torch.tensor([elapsed], dtype=torch.float64, device=device)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    prof = read_profile()
    # the outputs of the last timed step, before the breakdown pass below iterates D and x further
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, Dcur, state['x'])

    # --full only: after the timed region, a short untimed pass with every kernel group bracketed, for the
    # per-kernel breakdown (kernel_ms_avg); it does not enter `value`.
    breakdown, prof_stats = {}, None
    if args.full:
        if Dcur is not D:
            D.copy_(Dcur)
        _hip.check(h, lib.dcp_profile_reset(h), 'profile_reset')
        _hip.check(h, lib.dcp_profile_select(h, 0xffffffff), 'profile_select')
        _hip.check(h, lib.dcp_profile_enable(h, 1), 'profile_enable')
        Dcur = run(min(10, args.steps))
        barrier()
        _hip.check(h, lib.dcp_profile_enable(h, 0), 'profile_enable')
        breakdown = read_profile()
        prof_stats = breakdown.get('stats')

    # Multi-GPU (or --force-sharded): where one step's time goes on THIS rank -- local statistics (x update +
    # x^T [Y | x]), the exchange (ONE all-reduce of [K, F+K]; its time includes waiting for the slowest rank)
    # and the replicated D update; max over ranks reported.  In-library loop: the hipEvent brackets of the
    # breakdown pass above (the all-reduce has its own label); Python loop: torch events around its three calls.
    phase_ms = None
    if args.full and sharded_run:
        if in_library:
            def grp(*names):
                return sum(breakdown[n]['ms_avg'] for n in names if n in breakdown)
            acc = [grp('gram', 'x_neg', 'x_update', 'forward', 'stats', 'stats_sum'), grp('exchange'),
                   grp('d_update', 'd_norm')]
            how = 'hipEvent brackets inside dcp_nmf_mu_sharded_f32 over %d untimed steps' % min(10, args.steps)
        else:
            be = sharded.HipStepBackend(Y, None, state['x'], D, _hip.LIK_L2)
            Dn2 = torch.empty_like(D)
            Dc2 = D
            acc = [0.0, 0.0, 0.0]
            n_ph = 8
            for it in range(n_ph + 2):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                ev[0].record()
                st_ = be.local_stats(Dc2)
                ev[1].record()
                if world > 1:
                    dist.all_reduce(st_, op=dist.ReduceOp.SUM)
                ev[2].record()
                be.update(st_, Dc2, Dn2, it & 1)
                ev[3].record()
                torch.cuda.synchronize()
                if it >= 2:
                    for j in range(3):
                        acc[j] += ev[j].elapsed_time(ev[j + 1])
                Dc2, Dn2 = Dn2, Dc2
            state['x'] = be.x
            acc = [a_ / n_ph for a_ in acc]
            how = 'torch events around the three calls of the Python loop, synchronised after every step'
        t3 = torch.tensor(acc, dtype=torch.float64, device=device)
        if world > 1:
            dist.all_reduce(t3, op=dist.ReduceOp.MAX)
        K_, W_ = N_ATOMS, N_FEAT + N_ATOMS
        phase_ms = {'local_stats': round(float(t3[0]), 4), 'exchange_all_reduce': round(float(t3[1]), 4),
                    'replicated_update': round(float(t3[2]), 4),
                    'exchange_bytes_per_step': 4 * K_ * W_,
                    'note': 'per-phase GPU time of one step, max over ranks (%s; diagnostic, the timed region '
                            'runs without brackets). The all-reduce is fully exposed between the two compute '
                            'phases: each depends on the other (DESIGN.md section 5).' % how}

    finite = bool(torch.isfinite(Dcur).all().item()) and bool(torch.isfinite(state['x']).all().item())

    if rank == 0:
        ms_step = 1e3 * elapsed / args.steps
        W = 4.0 * N_ROWS * N_ATOMS * N_FEAT + 4.0 * N_ROWS * N_ATOMS ** 2 + 4.0 * N_ATOMS ** 2 * N_FEAT
        out = {
            'metric': 'nmf_mu_iterations_per_s', 'value': args.steps / elapsed,
            'unit': 'iterations/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': ms_step, 'higher_is_better': True, 'scaling': 'strong',
            'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            'config': {'workload': ('nmf_mu l2 no-mask Y=65536x4096 k=256 fp32 (BASELINE configs[1])'
                                    if not args.rows else 'ANALYSIS ONLY: one shard of %d rows' % rows),
                       'rows_per_gpu': rows, 'parallelism': 'rows sharded x%d, 1 all-reduce/step' % world,
                       'loop': loop_name},
            'algorithmic_tflops': W / (elapsed / args.steps) / 1e12,
            'mfma_roofline_frac_whole_step': W / (elapsed / args.steps) / 1e12 / (PEAK_F32_MFMA_TFLOPS * world),
            'finite': finite,
        }
        if args.full:
            out['kernel_ms_avg'] = {k: round(v['ms_avg'], 4) for k, v in breakdown.items()}
        if phase_ms is not None:
            out['phase_ms'] = phase_ms
        if dumped is not None:
            out['dumped_outputs'] = {'dir': args.dump_outputs, 'arrays': dumped}
        # dominant kernel: the fused Y.D^T GEMM + MU quotient (2.N.K.F flop per launch)
        dom = prof.get('x_update')
        if world == 1 and not args.rows:
            traffic, traffic_src = pmc_traffic('0, 0, false, EpiMuNum<float>')
        else:   # the committed PMC pass is the N = 1 run of the full shape; a shard's launch is another kernel
            traffic, traffic_src = None, 'not collected for this configuration (PMC pass exists for N=1 only)'
        if dom:
            flops = 2.0 * rows * N_ATOMS * N_FEAT
            ach = flops / (dom['ms_avg'] * 1e-3) / 1e12
            out['roofline'] = {'bound': 'mfma', 'kernel': 'gemm_mfma_kernel<NT, EpiMuNum> (Y.D^T + quotient)',
                               'achieved': ach, 'peak': PEAK_F32_MFMA_TFLOPS, 'unit': 'TFLOP/s',
                               'frac': ach / PEAK_F32_MFMA_TFLOPS, 'traffic': traffic,
                               'traffic_note': traffic_src,
                               'algorithmic_bytes': 4.0 * (rows * N_FEAT + N_ATOMS * N_FEAT + 3 * rows * N_ATOMS),
                               'launch_ms': dom['ms_avg'], 'launches': dom['launches']}
        st = prof_stats
        if st:
            flops = 2.0 * rows * N_ATOMS * (N_FEAT + N_ATOMS)
            ach = flops / (st['ms_avg'] * 1e-3) / 1e12
            out['roofline_stats_gemm'] = {'bound': 'mfma', 'kernel': 'gemm_mfma_kernel<TN, EpiSlab> (x^T.[Y|x])',
                                          'achieved': ach, 'peak': PEAK_F32_MFMA_TFLOPS,
                                          'unit': 'TFLOP/s', 'frac': ach / PEAK_F32_MFMA_TFLOPS,
                                          'launch_ms': st['ms_avg']}
        if args.full and world == 1 and not args.rows and not args.no_cpu_baseline:
            # full-shape oracle parity gate + measured CPU baseline (same Y as the timed run)
            out['parity'], out['cpu_baseline'] = parity_and_cpu_baseline(torch, lib, h, Y, D0)
        if args.full and world == 1 and not args.rows and not args.no_secondary:
            try:
                del Y
                torch.cuda.empty_cache()
                out['secondary'] = secondary_configs(torch, device, with_oracle=not args.no_cpu_baseline)
                sh = out['secondary'].get('shard_8192_rows_ms_per_iter')
                if sh:      # the full problem's step against one of its eight shards (before the all-reduce)
                    sh['compute_side_speedup_at_8_gpus'] = round(ms_step / sh['value'], 2)
            except Exception as e:      # never lose the headline line to a side measurement
                out['secondary'] = {'error': repr(e)}
        print(json.dumps(out))
        if 'parity' in out and not out['parity']['pass']:
            raise SystemExit('parity gate FAILED: %r' % (out['parity'],))
        for key in ('dictionary_step_ms', 'dictionary_step_cd_ms', 'complex_dictionary_step_ms'):
            par = (out.get('secondary') or {}).get(key, {})
            par = par.get('parity') if isinstance(par, dict) else None
            if par is not None and not par['pass']:
                raise SystemExit('%s parity gate FAILED: %r' % (key, par))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()

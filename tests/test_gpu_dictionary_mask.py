"""Masked dictionary learning (dictionary_learning.solve(mask=...) -> solve_cd_mask -> dcp_dict_mask_step_*) at sizes
where dict_mask_gram_kernel and dict_mask_atom_kernel (csrc/dict_impl.hpp) take their strided loops more than once:
every stage of one step against the float64 restatement of tests/dict_mask_ref.py, and whole solves against
oracle.dictionary_learning."""
import ctypes
import math

import numpy as np
import pytest

import dict_mask_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = ['float32', 'float64', 'complex64', 'complex128']
BETA = 0.75
LASSO_ITER, LASSO_TOL = 10, 1e-5

# (Nb, F, K): the smallest sizes that take each loop past its first trip
#   (50, 5, 3)      the golden fixtures' size: every loop runs once
#   (64, 256, 16)   K K = F = 256: the last size at which every loop runs once
#   (37, 257, 17)   the first second trip of the pair loop (289 pairs) and of the channel loops, ragged Nb
#   (96, 300, 40)   7 pair passes; also the masked 'fista' and 'cd' solvers inside the step
#   (200, 600, 70)  more than one 64-atom block, 3 channel strides, 20 pair passes
#   (4096, 64, 17)  float32 / complex64: x^H (y o m) is split 8 ways (see test_mask_step_direct)
SHAPES = [(50, 5, 3), (64, 256, 16), (37, 257, 17), (96, 300, 40), (200, 600, 70), (4096, 64, 17)]
FRACTIONAL = {(96, 300, 40), (200, 600, 70)}             # masks in (0, 1]; the others are binary
# alpha F: the LASSO's threshold is alpha sum_f m_nf per row.  At F = 5 the three atoms are strongly coherent and
# the zero column needs a higher threshold to stay zero.
ALPHA_F = {(50, 5, 3): 4.0}
# data seeds (shape, complex) at which the zero column stays zero with a 20 % margin in alpha (searched on the CPU
# oracle, float64, among seeds 0, 1, 2, ...); 0 unless listed
SEEDS = {((50, 5, 3), True): 20, ((4096, 64, 17), False): 1}


def _step_cases():
    out = []
    for shape in SHAPES:
        for dt in DTYPES:
            if shape == (4096, 64, 17) and dt in ('float64', 'complex128'):
                continue
            out.append(shape + (dt, 'ista'))
            if shape == (96, 300, 40):
                out.append(shape + (dt, 'fista'))
                out.append(shape + (dt, 'cd'))
    return out


def _err(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) / max(1.0, float(np.max(np.abs(b))))


def _problem(shape, dt):
    cplx = np.dtype(dt).kind == 'c'
    p = ref.Problem(dt, shape[0], shape[1], shape[2], shape in FRACTIONAL, seed=SEEDS.get((shape, cplx), 0))
    return p, ALPHA_F.get(shape, 2.0) / shape[1]


def _run_step(p, alpha, method):
    """dcp_dict_mask_step_* on the problem -> X, A3, B, D_new (NumPy, p.dt), max|dD| (float), lasso_it."""
    import torch
    from decomp_amd import _arrays, _hip

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Y, M, X, D, A3, B = t(p.y), t(p.m), t(p.x0), t(p.D), t(p.A3_old), t(p.B_old)
    D_new = torch.empty_like(D)
    md, lit = ctypes.c_double(-1.0), ctypes.c_int(-7)
    lib, h = _arrays.lib_handle(D)
    fn = getattr(lib, 'dcp_dict_mask_step_' + ref.SUFFIX[str(p.dt)])
    code = {'ista': _hip.LASSO_ISTA, 'fista': _hip.LASSO_FISTA, 'cd': _hip.LASSO_CD}[method]
    _hip.check(h, fn(h, _arrays.ptr(Y), _arrays.ptr(M), _arrays.ptr(X), _arrays.ptr(D), _arrays.ptr(D_new),
                     _arrays.ptr(A3), _arrays.ptr(B), p.Nb, p.F, p.K, BETA, alpha, code, LASSO_ITER, LASSO_TOL,
                     ctypes.byref(md), ctypes.byref(lit)), 'dcp_dict_mask_step')
    torch.cuda.synchronize()
    assert torch.equal(D, t(p.D)) and torch.equal(Y, t(p.y)) and torch.equal(M, t(p.m))     # inputs are only read
    return X.cpu().numpy(), A3.cpu().numpy(), B.cpu().numpy(), D_new.cpu().numpy(), md.value, lit.value


def check_step(p, alpha, method, X, A3, B, D_new, md, lit):
    """Every stage of the step against float64 computed from what that stage was handed.  Returns the largest
    ratio error / bound of the A3, B and D_new checks."""
    from oracle import lasso as olasso
    single = ref.is_single(p.dt)
    cplx = p.dt.kind == 'c'
    u = ref.unit_roundoff(p.dt)
    Nb, F, K, kz, fz = p.Nb, p.F, p.K, p.kz, p.fz
    tag = (Nb, F, K, str(p.dt), method)

    # --- X: the LASSO's codes, from the warm start
    ito, Xo = olasso.solve_fastpath(ref.up(p.y), ref.up(p.D), alpha, x=ref.up(p.x0), tol=LASSO_TOL,
                                    maxiter=LASSO_ITER, method=method, mask=ref.up(p.m))
    ex = _err(X, Xo)
    print('mask step', tag, 'x err %.3g' % ex, 'lasso_it', lit, ito, 'nonzero share %.3f' % (np.count_nonzero(X) / X.size))
    assert X.dtype == p.dt and ex < (3e-4 if single else 1e-9), (tag, ex)
    if not single:
        assert lit == ito, (tag, lit, ito)
    assert 0 <= lit < LASSO_ITER
    assert not Xo[:, kz].any() and not X[:, kz].any(), tag          # the zero column stays zero through the LASSO
    assert X[0].any() and np.count_nonzero(X) > X.size // 25, tag

    # --- A3, from the GPU's X
    A3_ref, B_ref = ref.stats(X, p.y, p.m, p.A3_old, p.B_old, BETA)
    bA, bB = ref.stats_bounds(X, p.y, p.m, p.A3_old, p.B_old, BETA)
    c_A = (Nb + 4) * (4 if cplx else 1)
    eA = np.abs(ref.up(A3) - A3_ref)
    live = bA > 0
    rA = float(np.max(eA[live] / (c_A * u * bA[live])))
    print('mask step', tag, 'A3 ratio %.3g' % rA)
    assert np.all(np.isfinite(eA)) and rA <= 1.0, (tag, rA)
    assert not A3[~live].any(), tag                                   # exact zeros where nothing is summed
    assert not live[kz].any() and not live[:, :, kz].any() and not live[:, fz].any() and live.sum() > live.size // 8

    # --- B, from the GPU's X
    eB = np.abs(ref.up(B) - B_ref)
    liveB = bB > 0
    rB = float(np.max(eB[liveB] / ((2e-5 if single else 1e-14) * bB[liveB])))
    print('mask step', tag, 'B ratio %.3g' % rB)
    assert np.all(np.isfinite(eB)) and rB <= 1.0, (tag, rB)
    assert not B[~liveB].any() and not liveB[kz].any() and not liveB[:, fz].any(), tag

    # --- D_new, from the GPU's A3 and B
    D_ref, uu, nrm, S = ref.atom_update(p.D, A3, B)
    c_D = (K + int(math.ceil(F / 256.0)) + 16) * (4 if cplx else 1)
    assert np.all(np.isfinite(ref.up(D_new))), tag
    tol_D = c_D * u * (S + np.abs(uu)) / nrm[:, None]
    rD = float(np.max(np.abs(ref.up(D_new) - D_ref) / tol_D))
    moved = float(np.max(np.abs(D_ref - ref.up(p.D))))
    print('mask step', tag, 'D_new ratio %.3g' % rD, 'largest tolerance %.3g' % float(np.max(tol_D)),
          'max|dD| %.3g' % moved, 'atoms with |u| > 1: %d' % int(np.sum(nrm > 1.0)))
    assert rD <= 1.0, (tag, rD)
    # the atom of the zero column: u_k = 0 / (F 1e-15) + D_k, and a unit row's norm is 1 to rounding
    assert np.all(np.abs(ref.up(D_new[kz]) - ref.up(p.D[kz])) <= c_D * u * np.abs(ref.up(p.D[kz]))), tag
    assert moved > 2.0 * float(np.max(tol_D)), tag           # the other atoms move by more than any tolerance

    # --- max|dD| of the arrays that came back
    if cplx:
        want = ref.maxdiff(p.D, D_new)
        assert abs(md - want) <= 4 * (2 * u) * want, (tag, md, want)
    else:
        assert md == float(np.max(np.abs(p.D - D_new))), (tag, md)
    return rA, rB, rD


@pytest.mark.parametrize('Nb,F,K,dt,method', _step_cases())
def test_mask_step_direct(Nb, F, K, dt, method):
    """One dcp_dict_mask_step_* call with non-zero old statistics and beta = 0.75 (dict_mask_ref.Problem: sparse warm
    start, strictly normalised D, a code column that is and stays zero, a channel masked in every row, binary or
    fractional mask), every stage against float64 computed from what the GPU handed to that stage:
      X      oracle.lasso.solve_fastpath from the same warm start: 3e-4 single, 1e-9 double (the bounds of
             test_gpu_lasso.py::test_random_shapes_against_oracle), lasso_it equal in double
      A3     |A3 - ref| <= c_A u bound_A elementwise, c_A = Nb + 4 (x 4 complex): the length of the kernel's
             sequential sum plus the scale-and-add; exact zeros where bound_A = 0
      B      |B - ref| <= 2e-5 (single) / 1e-14 (double) x bound_B elementwise: test_gpu_gemm.py's constants
      D_new  |D_new - ref| <= c_D u (S + |u|) / nrm elementwise, c_D = K + ceil(F / 256) + 16 (x 4 complex);
             finite; the zero column's atom comes back as D_k
      max|dD| equal to max|D - D_new| of the returned arrays (real), within 4 ulp (complex: a square root)
    The constants are worst-case operation counts, not tuned values.

    (4096, 64, 17), float32 and complex64: plan_splits<FORM_TN> (csrc/gemm.hpp) gives every split at least 32
    reduction blocks of 16 rows, so x^H (y o m) first splits at Nb = 1009 (64 blocks); at Nb = 4096 there are 256
    blocks and one or two output tiles, so the plan is min(1024 / tiles, 256 / 32, 64) = 8 splits of 512 rows, summed
    by reduce_slabs_kernel.  The other shapes (Nb <= 200, 13 blocks) run un-split.

    Largest ratios error / bound observed on an MI355X, over all shapes and solvers:
      float32     A3 0.051    B 0.015    D_new 0.049    (x: 8.1e-7 of the 3e-4)
      float64     A3 0.087    B 0.033    D_new 0.047    (x: 1.3e-15 of the 1e-9)
      complex64   A3 0.012    B 0.0079   D_new 0.011    (x: 8.9e-7)
      complex128  A3 0.012    B 0.050    D_new 0.011    (x: 2.4e-15)
    """
    p, alpha = _problem((Nb, F, K), dt)
    check_step(p, alpha, method, *_run_step(p, alpha, method))


# ---- whole solves ------------------------------------------------------------------------------------------------

def _solve_problem(dt, N, F, K, seed):
    rng = np.random.RandomState(seed)
    cplx = np.dtype(dt).kind == 'c'

    def randn(*s):
        return (rng.randn(*s) + 1j * rng.randn(*s)) if cplx else rng.randn(*s)
    Dt = randn(K, F)
    xt = 3.0 * randn(N, K) * (rng.uniform(size=(N, K)) < 0.2)
    y = (xt @ Dt + 0.1 * randn(N, F)).astype(dt)
    D0 = (Dt + 0.2 * randn(K, F)).astype(dt)
    mask = (rng.uniform(size=(N, F)) > 0.3).astype(np.float32 if ref.is_single(dt) else np.float64)
    return y, D0, mask


_SOLVE_KW = dict(tol=0.0, minibatch=48, maxiter=3, lasso_iter=10, random_seed=0)
SOLVE_ALPHA = 0.01
# single precision: error(GPU, float64 oracle) <= C_SINGLE x error(single-precision oracle, float64 oracle)
C_SINGLE = 8
_ORACLE = {}


def _oracle_solve(dt, method, work_dt=None):
    """(y, D0, mask) in dtype dt and oracle.dictionary_learning.solve on them, carried out in work_dt (dt itself, or
    the double type for a single-precision dt: the same rounded inputs, cast up).  Computed once, read-only."""
    from oracle import dictionary_learning as odl
    work_dt = work_dt or dt
    key = (dt, method, work_dt)
    if key not in _ORACLE:
        y, D0, mask = _solve_problem({'float32': 'float64', 'complex64': 'complex128'}.get(dt, dt), 203, 300, 20, seed=5)
        y, D0, mask = y.astype(dt), D0.astype(dt), mask.astype(np.float32 if ref.is_single(dt) else np.float64)
        rdt = np.float32 if ref.is_single(work_dt) else np.float64
        res = odl.solve(y.astype(work_dt), D0.astype(work_dt), SOLVE_ALPHA, lasso_method=method, mask=mask.astype(rdt),
                        **_SOLVE_KW)
        for a in (y, D0, mask) + tuple(res[1:]):
            a.setflags(write=False)
        _ORACLE[key] = (y, D0, mask, res)
    return _ORACLE[key]


@pytest.mark.parametrize('method', ['ista', 'fista', 'cd'])
@pytest.mark.parametrize('dt', DTYPES)
def test_mask_solve_against_oracle(dt, method):
    """dictionary_learning.solve(mask=...) against oracle.dictionary_learning.solve(mask=...): N = 203 in minibatches
    of 48 (the tail rows of each epoch are skipped), F = 300 (two channel strides), K = 20 (two pair passes), two
    epochs of 10 LASSO iterations.  Double precision: the project's 1e-7 for dictionary fixtures.  Single precision:
    no fixed number -- the oracle is also run in the single dtype, d_ref = _err(oracle_single, oracle_double) for
    D and for x, and the GPU must stay within C_SINGLE x d_ref of the double-precision oracle.  C_SINGLE is the smallest
    power of two that is at least twice the largest ratio measured on an MI355X:
                   ista          fista         cd           (error ratio for D, for x)
      float32    1.09, 1.79    0.81, 2.75    1.00, 1.14
      complex64  0.96, 2.66    1.09, 2.11    0.74, 0.72
    with d_ref about 5e-8 for D and 2e-7 to 4e-7 for x: the largest is 2.75, so C_SINGLE = 8.
    """
    from decomp_amd import dictionary_learning as dl
    single = ref.is_single(dt)
    y, D0, mask, (ito, Do, xo) = _oracle_solve(dt, method)
    it, D, x = dl.solve(y.copy(), D0.copy(), SOLVE_ALPHA, lasso_method=method, mask=mask.copy(), **_SOLVE_KW)
    assert it == ito == 3
    assert D.dtype == y.dtype and x.dtype == y.dtype and x.shape == (203, 20)
    if not single:
        eD, ex = _err(D, Do), _err(x, xo)
        print('mask solve', dt, method, 'D err %.3g x err %.3g' % (eD, ex))
        assert eD < 1e-7 and ex < 1e-7, (dt, method, eD, ex)
    else:
        _, _, _, (it2, D2, x2) = _oracle_solve(dt, method, {'float32': 'float64', 'complex64': 'complex128'}[dt])
        assert it2 == 3 and D2.dtype != Do.dtype and Do.dtype == y.dtype
        dD, dx = _err(Do, D2), _err(xo, x2)
        eD, ex = _err(D, D2), _err(x, x2)
        print('mask solve', dt, method, 'd_ref D %.3g x %.3g' % (dD, dx), 'gpu D %.3g x %.3g' % (eD, ex),
              'ratio D %.3g x %.3g' % (eD / dD, ex / dx))
        assert dD > 0 and dx > 0
        assert eD <= C_SINGLE * dD and ex <= C_SINGLE * dx, (dt, method, eD / dD, ex / dx)
    assert np.count_nonzero(x) > 0
    # rows no minibatch has visited keep the initial 1.0: the same rows as in the oracle's run
    assert np.array_equal(np.all(x == 1.0, axis=1), np.all(xo == 1.0, axis=1))
    assert np.all(xo == 1.0, axis=1).any()


def test_mask_solve_stops_mid_epoch():
    """The masked twin of test_gpu_dictionary.py::test_stop_test_fires_mid_epoch_speculative_step_is_discarded: float64,
    a tolerance taken from an oracle trace so that max|D - D_new| < tol first holds in the MIDDLE of epoch 2.  The GPU
    run returns the oracle's epoch number, dictionary and codes, the rows not yet visited included."""
    from decomp_amd import dictionary_learning as dl
    from oracle import dictionary_learning as odl
    rng = np.random.RandomState(17)
    N, F, K, mb = 203, 24, 5, 20
    Dt = rng.randn(K, F)
    xt = 2.0 * rng.randn(N, K) * (rng.uniform(size=(N, K)) < 0.4)
    y = xt @ Dt + 0.05 * rng.randn(N, F)
    D0 = Dt + 0.2 * rng.randn(K, F)
    mask = (rng.uniform(size=(N, F)) > 0.3).astype(np.float64)
    base = dict(minibatch=mb, maxiter=4, lasso_method='ista', lasso_iter=12, lasso_tol=1e-7, random_seed=5)
    trace = []
    odl.solve(y.copy(), D0.copy(), 0.02, tol=0.0, mask=mask.copy(), trace=trace, **base)
    n_loop = N // mb
    diffs = [t['maxdiff'] for t in trace]
    first_below = None
    for s in range(n_loop + 3, 2 * n_loop - 1):                 # well inside epoch 2
        cand = 0.5 * (diffs[s] + min(diffs[:s]))
        if diffs[s] < cand and all(d >= cand for d in diffs[:s]):
            first_below = (s, cand)
            break
    assert first_below is not None, diffs
    step, tol = first_below
    ito, Do, xo = odl.solve(y.copy(), D0.copy(), 0.02, tol=tol, mask=mask.copy(), **base)
    it, D, x = dl.solve(y.copy(), D0.copy(), 0.02, tol=tol, mask=mask.copy(), **base)
    assert ito == 2 and it == ito
    assert _err(D, Do) < 1e-8 and _err(x, xo) < 1e-8, (_err(D, Do), _err(x, xo))
    # rows of the interrupted epoch that no step has reached, and those only the first epoch reached, are the oracle's
    assert np.array_equal(np.all(x == 1.0, axis=1), np.all(xo == 1.0, axis=1)) and np.any(np.all(x == 1.0, axis=1))

"""GPU: decomp_amd.template_matching.orthogonal_pursuit (dcp_tm_omp_*) against the NumPy references of tm_omp_ref.py --
supports, coefficients, step counts, residual and orthogonality on the shared problems in all four dtypes, against
omp.solve on the dense operator, on edge atoms, at the sparsity cap, on both tiers of the greedy kernel, on degenerate
inputs, and bit for bit from run to run and from batch to single signal.

Signals whose reference selection margin is below delta (1e-4 single, 1e-8 double), and in tol runs signals whose
residual margin is below 1e-4, are left out of the support and coefficient comparison (at most 10 % per case,
asserted); residual and orthogonality are checked on every signal.  The bounds are 4 x what omp_gram in the test dtype
on the CPU shows against omp_residual in double, floor 64 eps (tm_omp_ref.Analysis.bounds)."""
import numpy as np
import pytest

import tm_omp_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = ['float32', 'float64', 'complex64', 'complex128']
SFX = {'float32': 'f32', 'float64': 'f64', 'complex64': 'c64', 'complex128': 'c128'}


def _precision(dt):
    return 'single' if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else 'double'


def _cplx(dt):
    return np.dtype(dt).kind == 'c'


def _lds_atoms(dt):
    from decomp_amd import _hip
    return getattr(_hip.load(), 'dcp_tm_omp_lds_atoms_' + SFX[np.dtype(dt).name])()


def _solve(an, dt, y=None):
    from decomp_amd import template_matching as tm
    N, stride, padding = an.geom
    y = an.y if y is None else y
    it, x = tm.orthogonal_pursuit(y.astype(dt), an.D.astype(dt), n_nonzero_coefs=an.n, tol=an.tol, stride=stride,
                                  padding=padding)
    assert isinstance(x, np.ndarray) and x.dtype == np.dtype(dt)
    return it, x


def _check_against(an, dt, it, x, tag, supports=True, max_left_out=ref.MAX_LEFT_OUT):
    """Supports, step counts and coefficients of a GPU result on the kept signals, residual and orthogonality on every
    signal, against an Analysis.  Returns the orthogonality bound."""
    precision = _precision(dt)
    assert x.shape == an.x.shape
    B = x.shape[0]
    keep = an.keep(precision)
    left_out = 1.0 - float(np.mean(keep))
    b_coef, b_orth, b_res = an.bounds(precision)
    nnz = np.count_nonzero(x.reshape(B, -1), axis=1)
    err = float(np.max(np.abs(x.astype(an.x.dtype) - an.x)[keep], initial=0.0)) / float(np.max(np.abs(an.x)))
    res, orth = an.metrics(x)
    print('%s %s: left out %.2f %%; coefficient error %.3g (bound %.3g); orthogonality %.3g (bound %.3g); residual '
          'excess %.3g (bound %.3g); steps %s; it %d' % (tag, np.dtype(dt).name, 100 * left_out, err, b_coef,
                                                         float(orth.max()), b_orth, float(res.max()), b_res,
                                                         sorted(set(an.steps.tolist())), it))
    assert np.all(np.isfinite(x))
    assert it == int(nnz.max())
    if supports:
        assert left_out <= max_left_out
        assert np.array_equal((x != 0)[keep], (an.x != 0)[keep])
        assert np.array_equal(nnz[keep], an.steps[keep])
        assert err <= b_coef
    assert float(orth.max()) <= b_orth
    assert float(res.max()) <= b_res
    return b_orth


# ---- 1. the shared cases --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case', sorted(ref.CASES))
def test_supports_coefficients_residual_and_orthogonality(case, dt):
    from decomp_amd import template_matching as tm
    B, T, S, N, stride, padding, nev = ref.CASES[case]
    an = ref.case_analysis(case, _cplx(dt), False)
    it, x = _solve(an, dt)
    b_orth = _check_against(an, dt, it, x, 'case %d' % case)
    assert it <= nev
    if case in (0, 1, 2):
        # what the re-fit adds: plain matching pursuit leaves its residual correlated with the atoms it took
        _, xm = tm.pursuit(an.y.astype(dt), an.D.astype(dt), n_nonzero_coefs=nev, stride=stride, padding=padding)
        orth_mp = ref.orthogonality(xm, an.y, an.D, N, stride, padding)
        print('case %d %s: pursuit orthogonality median %.3g, max %.3g' % (case, dt, np.median(orth_mp), orth_mp.max()))
        assert float(orth_mp.max()) >= 100 * b_orth and float(np.median(orth_mp)) >= 100 * b_orth


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case', sorted(ref.CASES))
def test_residual_stop(case, dt):
    """tol = 0.02 median |y|^2 and the step limit left at its default, min(T C, cap)."""
    an = ref.case_analysis(case, _cplx(dt), True)
    assert an.n is None
    _check_against(an, dt, *_solve(an, dt), tag='case %d tol' % case)


# ---- 2. omp.solve on the dense operator -----------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case', [0, 2])
def test_against_omp_on_the_dense_operator(case, dt):
    from decomp_amd import omp, template_matching as tm
    B, T, S, N, stride, padding, nev = ref.CASES[case]
    an = ref.case_analysis(case, _cplx(dt), False)
    it, x = _solve(an, dt)
    A = tm._temp2mat(an.D.astype(dt), N, stride, padding).reshape(-1, N)
    itd, xd = omp.solve(an.y.astype(dt), A, n_nonzero_coefs=nev)
    xd = xd.reshape(x.shape)
    keep = an.keep(_precision(dt))
    b_coef = an.bounds(_precision(dt))[0]
    err = float(np.max(np.abs(x.astype(an.x.dtype) - xd.astype(an.x.dtype))[keep])) / float(np.max(np.abs(an.x)))
    print('case %d %s: against dense omp.solve %.3g (bound %.3g)' % (case, dt, err, b_coef))
    assert np.array_equal((x != 0)[keep], (xd != 0)[keep])
    assert it == itd == nev
    assert err <= b_coef


# ---- 3. edge atoms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
def test_edge_atoms(dt):
    """Truncated atoms at both ends and an inside atom that overlaps the first: G by the explicit sum."""
    y, D, geom, x0 = ref.edge_problem(_cplx(dt))
    an = ref.Analysis(y, D, geom, n=3)
    assert np.array_equal(an.x != 0, x0 != 0)
    it, x = _solve(an, dt)
    _check_against(an, dt, it, x, 'edge')
    assert it == 3 and np.array_equal(x != 0, x0 != 0)


# ---- 4. at the cap ----------------------------------------------------------------------------------------------------
CAP_PROBLEMS = {False: (16, 2, 9, 400, 1, 'SAME', 64), True: (16, 2, 9, 300, 1, 'SAME', 32)}


@pytest.mark.parametrize('dt', DTYPES)
def test_at_the_cap(dt):
    """n_nonzero_coefs = cap events per signal.  Supports and coefficients are compared in double only: in single
    precision the reference itself leaves most of these signals within 1e-4 of a tie."""
    cplx = _cplx(dt)
    prob = CAP_PROBLEMS[cplx]
    cap = prob[-1]
    assert cap == ref.cap_of(cplx)
    an = ref.problem_analysis(300 + int(cplx), *prob, cplx)
    it, x = _solve(an, dt)
    _check_against(an, dt, it, x, 'cap', supports=_precision(dt) == 'double')
    assert it == cap and np.all(an.steps == cap)
    assert np.all(np.count_nonzero(x.reshape(x.shape[0], -1), axis=1) == cap)


# ---- 5. both tiers ----------------------------------------------------------------------------------------------------
# (T C, cplx) -> seed where the default (T C mod 1000) leaves out one of the four signals by the reference's own margins
# in single precision (seeds 672 and 1672: the tol run, resp. both runs)
TIER_SEEDS = {(28672, False): 2672}


@pytest.mark.parametrize('where', ['below', 'at', 'above'])
@pytest.mark.parametrize('dt', DTYPES)
def test_both_tiers(dt, where):
    """T = 2 and T C two atoms below, at and two atoms above the largest size whose correlations live in LDS; with
    tol the step limit is the cap, so the LDS tier runs with its largest carve."""
    L = _lds_atoms(dt)
    assert L == 112 * 1024 // np.dtype(dt).itemsize
    K = {'below': L - 2, 'at': L, 'above': L + 2}[where]
    B, T, S, stride, padding, nev = 4, 2, 9, 1, 'SAME', 12
    N = K // T - S + 1
    cplx = _cplx(dt)
    seed = TIER_SEEDS.get((K, cplx), K % 1000)
    for with_tol in (False, True):
        an = ref.problem_analysis(seed, B, T, S, N, stride, padding, nev, cplx, with_tol)
        assert an.x.shape == (B, T, K // T)
        _check_against(an, dt, *_solve(an, dt), tag='T C = %d (%s tier)%s' % (K, 'LDS' if K <= L else 'global',
                                                                              ' tol' if with_tol else ''))


@pytest.mark.parametrize('prob', [(4, 3, 200, 600, 1, 'SAME', 6), (2, 1, 600, 1300, 1, 'SAME', 4)])
@pytest.mark.parametrize('dt', DTYPES)
def test_windows_wider_than_the_workgroup(dt, prob):
    """T (2 dh + 1) = 3 x 399 > 1024: the correlation update of one support atom takes two passes over the templates;
    2 dh + 1 = 1199 > 1024: two passes over the window of one template."""
    for with_tol in (False, True):
        an = ref.problem_analysis(11, *prob, _cplx(dt), with_tol)
        _check_against(an, dt, *_solve(an, dt), tag='wide S = %d%s' % (prob[2], ' tol' if with_tol else ''))


# ---- 6. degenerate inputs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
def test_degenerate_inputs(dt):
    from decomp_amd import template_matching as tm
    rng = np.random.RandomState(9)
    D = rng.randn(3, 5).astype(dt)
    y = rng.randn(6, 40).astype(dt)
    y[2] = 0                                    # a zero signal: x = 0, no step
    it, x = tm.orthogonal_pursuit(y, D, n_nonzero_coefs=7)
    assert it == 7 and np.all(np.isfinite(x)) and np.all(x[2] == 0)
    assert np.all(np.count_nonzero(x.reshape(6, -1), axis=1)[[0, 1, 3, 4, 5]] == 7)
    for kw in (dict(n_nonzero_coefs=7), dict(tol=0.0)):
        it, x = tm.orthogonal_pursuit(np.zeros_like(y), D, **kw)
        assert it == 0 and np.all(x == 0)
    # two identical templates, tol = 0, n = 30: the twin of a taken atom is dependent on the support
    d = rng.randn(1, 6).astype(dt)
    D2 = np.concatenate([d, d])
    y = rng.randn(5, 50).astype(dt)
    it1, x1 = tm.orthogonal_pursuit(y, D2, n_nonzero_coefs=1)
    it, x = tm.orthogonal_pursuit(y, D2, n_nonzero_coefs=30, tol=0.0)
    assert 1 <= it <= 30 and np.all(np.isfinite(x))
    assert not np.any((x[:, 0] != 0) & (x[:, 1] != 0))
    dd = np.complex128 if _cplx(dt) else np.float64
    y64, D64 = y.astype(dd), D2.astype(dd)
    r30 = ref.residual_norm(x, y64, D64, 50, 1, 'SAME')
    r1 = ref.residual_norm(x1, y64, D64, 50, 1, 'SAME')
    assert np.all(r30 <= r1)
    # an empty batch
    it, x = tm.orthogonal_pursuit(y[:0], D2, n_nonzero_coefs=3, padding='VALID')
    assert it == 0 and x.shape == (0, 2, 45)


# ---- 7. reproducibility and the conventions of solve ----------------------------------------------------------------
def test_reproducible_and_the_conventions_of_solve():
    import torch
    from decomp_amd import template_matching as tm
    B, T, S, N, stride, padding, nev = ref.CASES[0]
    y, D = ref.case_problem(0, False)
    y, D = y.astype(np.float32), D.astype(np.float32)
    C = ref.otm.geometry(S, N, stride, padding)[0]
    it, x = tm.orthogonal_pursuit(y[:21].reshape(3, 7, N), D, n_nonzero_coefs=nev, stride=stride, padding=padding)
    it_flat, x_flat = tm.orthogonal_pursuit(y[:21], D, n_nonzero_coefs=nev, stride=stride, padding=padding)
    assert x.shape == (3, 7, T, C) and np.array_equal(x.reshape(21, T, C), x_flat) and it == it_flat
    it1, x1 = tm.orthogonal_pursuit(y[5], D, n_nonzero_coefs=nev, stride=stride, padding=padding)
    assert x1.shape == (T, C) and np.array_equal(x1, x_flat[5])
    yt, Dt = torch.from_numpy(y).cuda(), torch.from_numpy(D).cuda()
    kw = dict(n_nonzero_coefs=2 * nev, tol=1e-3, stride=stride, padding=padding)
    runs = [tm.orthogonal_pursuit(yt, Dt, **kw) for _ in range(2)]
    assert torch.is_tensor(runs[0][1]) and runs[0][1].is_cuda and runs[0][1].dtype == torch.float32
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    # a signal's result does not depend on the rest of the batch
    for b in (0, 13, B - 1):
        itb, xb = tm.orthogonal_pursuit(yt[b:b + 1], Dt, **kw)
        assert torch.equal(xb[0], runs[0][1][b])
    assert np.array_equal(runs[0][1].cpu().numpy(), tm.orthogonal_pursuit(y, D, **kw)[1])
    pred = tm.predict(runs[0][1], Dt, N, stride, padding)
    assert float((yt - pred).norm()) < 0.3 * float(yt.norm())
    with pytest.raises(TypeError):
        tm.orthogonal_pursuit(yt, D, n_nonzero_coefs=2)


@pytest.mark.parametrize('dt', DTYPES)
def test_batch_and_single_signal_agree_bit_for_bit_on_both_tiers(dt):
    from decomp_amd import template_matching as tm
    L = _lds_atoms(dt)
    for K in (L, L + 2):
        N = K // 2 - 8
        y, D, _ = ref.mp.make_problem(7, 3, 2, 9, N, 1, 'SAME', 8, _cplx(dt))
        y, D = y.astype(dt), D.astype(dt)
        it, x = tm.orthogonal_pursuit(y, D, n_nonzero_coefs=8)
        it2, x2 = tm.orthogonal_pursuit(y, D, n_nonzero_coefs=8)
        assert it == it2 == 8 and np.array_equal(x, x2)
        it1, x1 = tm.orthogonal_pursuit(y[1:2], D, n_nonzero_coefs=8)
        assert np.array_equal(x1[0], x[1])


# ---- the raw entry ----------------------------------------------------------------------------------------------------
def test_raw_entry_invalid_arguments_return_an_error():
    import ctypes
    import torch
    from decomp_amd import _arrays
    y = torch.ones((3, 40), dtype=torch.float32, device='cuda')
    D = torch.ones((2, 4), dtype=torch.float32, device='cuda')
    x = torch.zeros((3, 2, 43), dtype=torch.float32, device='cuda')      # C = 43, T C = 86 > cap
    lib, h = _arrays.lib_handle(y)
    it = ctypes.c_int(-1)

    def call(n, tol=-1.0, null=None, geom=(3, 2, 4, 40, 1, 1), fn=lib.dcp_tm_omp_f32, ptrs=None):
        p = {'Y': _arrays.ptr(y), 'D': _arrays.ptr(D), 'X': _arrays.ptr(x), 'it': ctypes.byref(it)}
        if null:
            p[null] = None
        rc = fn(h, p['Y'], p['D'], p['X'], *geom, n, float(tol), p['it'])
        return rc, lib.dcp_last_error_string(h).decode()
    for n in (0, -1, 65, 2 ** 40):
        rc, msg = call(n)
        assert rc == -1 and 'n_steps' in msg
    rc, msg = call(5, geom=(3, 2, 4, 4, 1, 0))                            # 'VALID', N = 4: T C = 2
    assert rc == -1 and 'n_steps' in msg
    rc, msg = call(2, tol=float('nan'))
    assert rc == -1 and 'NaN' in msg
    for null in ('Y', 'D', 'X', 'it'):
        rc, msg = call(2, null=null)
        assert rc == -1 and 'null' in msg
    rc, msg = call(2, geom=(3, 2, 41, 40, 1, 1))
    assert rc == -1 and 'geometry' in msg
    yc = torch.ones((3, 40), dtype=torch.complex64, device='cuda')
    rc = lib.dcp_tm_omp_c64(h, _arrays.ptr(yc), _arrays.ptr(yc), _arrays.ptr(yc), 3, 2, 4, 40, 1, 1, 33, -1.0,
                            ctypes.byref(it))
    assert rc == -1 and 'n_steps' in lib.dcp_last_error_string(h).decode()
    rc, msg = call(64)                                                     # the cap itself is accepted
    assert rc == 0 and torch.isfinite(x).all()

"""The CPU oracle against the golden vectors produced by the real reference
(oracle/make_golden.py).  This is what pins the oracle: every later GPU parity
test compares the HIP path with this oracle."""
import os

import numpy as np
import pytest

import oracle
from oracle import nmf as onmf, lasso as olasso, dictionary_learning as odl


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def _tol(dtype):
    # float64/complex128: same operations in the same order -> rounding only
    # float32: the reference promotes some intermediates (see oracle/lasso.py)
    return 1.0e-9 if np.dtype(dtype).itemsize >= 8 and np.dtype(dtype) != np.complex64 else 2.0e-4


def _close(a, b, tol):
    a = np.asarray(a)
    b = np.asarray(b)
    scale = max(1.0, float(np.max(np.abs(b)))) if b.size else 1.0
    return float(np.max(np.abs(a - b))) <= tol * scale if a.size else True


# ------------------------------------------------------------------ NMF ----
def _nmf_cases(golden_dir):
    g = _load(golden_dir, 'nmf_golden.npz')
    return g, [str(c) for c in g['cases']]


def test_nmf_trace_and_solve(golden_dir):
    g, cases = _nmf_cases(golden_dir)
    assert len(cases) == 24
    for name in cases:
        base, mtag = name.rsplit('_', 1)
        y, D0 = g[base + '/y'], g[base + '/D0']
        mask = g[base + '/mask'] if mtag == 'mask' else None
        lik = 'kl' if '_kl' in base else 'l2'
        tol = _tol(y.dtype)
        # per-iteration trace
        n = len(g[name + '/trace_maxdiff'])
        D = oracle.common.l2_strict(D0)
        x = np.ones((y.shape[0], D0.shape[0]), dtype=y.dtype)
        for i in range(n):
            x, D, diff = onmf.mu_step(y, x, D, mask, lik)
            ref = g[name + '/trace_maxdiff'][i]
            assert abs(diff - ref) <= tol * max(1.0, abs(ref)) + (1e-12 if tol < 1e-6 else 1e-6), (name, i)
            res = onmf.residual(y, x, D, mask)
            assert abs(res - g[name + '/trace_resid'][i]) <= max(tol, 1e-5 if y.dtype == np.float32 else 0) * g[name + '/trace_resid'][i] + 1e-12, (name, i)
        assert _close(D, g[name + '/trace_D'], tol), name
        assert _close(x, g[name + '/trace_x'], tol), name
        assert x.dtype == y.dtype and D.dtype == y.dtype
        # full solve
        it, Df, xf = onmf.solve(y, D0.copy(), tol=float(g[name + '/tol']),
                                maxiter=400, likelihood=lik, mask=mask)
        if y.dtype == np.float64:
            assert it == int(g[name + '/it']), name
            assert _close(Df, g[name + '/D'], tol), name
            assert _close(xf, g[name + '/x'], tol), name
        else:
            # float32: the stop iteration may move by rounding near tol
            assert abs(it - int(g[name + '/it'])) <= 3, name


def test_nmf_gram_formulation_drift(golden_dir):
    """The product computes x.(DD^T) and (x^T x).D; quantify the drift of that
    reformulation against the reference formulation (float32, 25 iterations):
    must stay far inside the 1e-5 residual tolerance of BASELINE.json."""
    g, _ = _nmf_cases(golden_dir)
    base = 'nmf_256x128k8_float32_l2'
    y, D0 = g[base + '/y'], g[base + '/D0']
    D = oracle.common.l2_strict(D0)
    x = np.ones((256, 8), np.float32)
    ref = g[base + '_nomask/trace_resid']
    for i in range(len(ref)):
        x, D, _ = onmf.mu_step_gram(y, x, D)
        assert abs(onmf.residual(y, x, D) - ref[i]) <= 1.0e-5 * ref[i]


# ---------------------------------------------------------------- LASSO ----
def test_lasso_prox_known_answers(golden_dir):
    g = _load(golden_dir, 'lasso_golden.npz')
    z = g['prox/z']
    # tests/test_lasso.py:21-33 hand values
    assert np.allclose(olasso.shrink_real(np.array([0.1, -2.0, 1.4]), 1.0),
                       [0.0, -1.0, 0.4])
    assert np.allclose(olasso.shrink_real(z, 1.0), [[0.0, -1.0, 0.4], [0.1, 2.0, -0.4]])
    assert np.allclose(olasso.shrink_real(z, 1.0), g['prox/real'])
    assert np.allclose(olasso.shrink_complex(z + z * 1.0j, 1.0), g['prox/complex45'])
    assert np.allclose(olasso.shrink_positive(z, 1.0), g['prox/positive'])
    # 90 degrees: shrinking i*z equals i*shrink(z)   (tests/test_lasso.py:42-45)
    zz = np.array([0.1, -2.0, 1.4])
    assert np.allclose(olasso.shrink_complex(zz * 1.0j, 1.0),
                       olasso.shrink_complex(zz + 0.0j, 1.0) * 1.0j)


def test_lasso_all_cases(golden_dir):
    g = _load(golden_dir, 'lasso_golden.npz')
    cases = [str(c) for c in g['cases']]
    assert len(cases) == 360
    for name in cases:
        base, mname, method, tag = name.split('/')
        y, A = g[base + '/y'], g[base + '/A']
        mask = None if mname == 'nomask' else g[base + '/' + mname]
        it, x = olasso.solve(y.copy(), A.copy(), float(g[name + '/alpha']),
                             tol=float(g[name + '/tol']), method=method,
                             maxiter=int(g[name + '/maxiter']),
                             mask=None if mask is None else mask.copy())
        xr = g[name + '/x']
        if y.dtype == np.float32:
            # reference promotes fista to float64 (NumPy>=2); compare loosely
            assert _close(x, xr, 5.0e-4), name
            if tag == 'exh':
                assert it == int(g[name + '/it']), name
        else:
            assert it == int(g[name + '/it']), name
            assert _close(x, xr, 1.0e-9), name
        assert x.shape == xr.shape


def test_lasso_parallel_cd_and_admm_cases(golden_dir):
    """lasso.py:448-523 and 586-657: the oracle performs the same
    operations on the same dtypes as the reference (including ADMM's silent promotion to
    double), so iteration counts and values agree to rounding for every dtype."""
    g = _load(golden_dir, 'lasso_extra_golden.npz')
    cases = [str(c) for c in g['cases']]
    assert len(cases) == 252
    n_raise = 0
    for name in cases:
        base, mname, method, tag = name.split('/')
        y, A = g[base + '/y'], g[base + '/A']
        mask = None if mname == 'nomask' else g[base + '/' + mname]
        kw = dict(tol=float(g[name + '/tol']), method=method, maxiter=int(g[name + '/maxiter']),
                  mask=None if mask is None else mask.copy())
        if str(g[name + '/raises']) == 'TypeError':
            n_raise += 1
            with pytest.raises(TypeError):
                olasso.solve(y.copy(), A.copy(), float(g[name + '/alpha']), **kw)
            continue
        it, x = olasso.solve(y.copy(), A.copy(), float(g[name + '/alpha']), **kw)
        xr = g[name + '/x']
        assert it == int(g[name + '/it']), name
        assert x.dtype == xr.dtype and x.shape == xr.shape, name
        assert _close(x, xr, 1.0e-9 if x.dtype.itemsize >= 8 and x.dtype != np.complex64
                      else 1.0e-5), name
    assert n_raise == 12


# ------------------------------------------------- dictionary learning -----
def test_dictionary_learning_all_cases(golden_dir):
    g = _load(golden_dir, 'dl_golden.npz')
    cases = [str(c) for c in g['cases']]
    assert len(cases) == 68
    for name in cases:
        parts = name.split('/')
        base = parts[0]
        y, D0, mask = g[base + '/y'], g[base + '/D0'], g[base + '/mask']
        if parts[1] == 'reftest':
            it, D, x = odl.solve(y.copy(), D0.copy(), 0.1, tol=1.0e-4,
                                 minibatch=100, maxiter=1000,
                                 lasso_method='acc_ista', lasso_iter=1000,
                                 random_seed=0)
        else:
            minibatch = int(parts[1][2:])
            lm = parts[2].rstrip('0123456789')
            li = int(parts[2][len(lm):])
            use_mask = parts[3] == 'mask'
            epochs = int(parts[4][2:])
            yy = y * mask if use_mask else y
            it, D, x = odl.solve(yy.copy(), D0.copy(), 0.1, tol=0.0,
                                 minibatch=minibatch, maxiter=epochs + 1,
                                 lasso_method=lm, lasso_iter=li,
                                 lasso_tol=1.0e-5, random_seed=0,
                                 mask=mask.copy() if use_mask else None)
        assert it == int(g[name + '/it']), name
        assert _close(D, g[name + '/D'], 1.0e-9), name
        assert _close(x, g[name + '/x'], 1.0e-9), name


def _run_dl_case(solve, g, name):
    """Re-run one case of dl_extra_golden.npz (names as oracle/make_golden.py::gen_dl_extra)."""
    parts = name.split('/')
    base = parts[0]
    y, D0 = g[base + '/y'], g[base + '/D0']
    if base.startswith('dlwide_'):
        lm = parts[1].rstrip('0123456789')
        li = int(parts[1][len(lm):])
        epochs = int(parts[2][2:])
        return solve(y.copy(), D0.copy(), 0.02, tol=0.0, minibatch=128, maxiter=epochs + 1,
                     lasso_method=lm, lasso_iter=li, lasso_tol=1.0e-5, random_seed=0)
    mask = g[base + '/mask']
    minibatch = int(parts[1][2:])
    lm = parts[2].rstrip('0123456789')
    li = int(parts[2][len(lm):])
    use_mask = parts[3] == 'mask'
    epochs = int(parts[4][2:])
    yy = y * mask if use_mask else y
    return solve(yy.copy(), D0.copy(), 0.1, tol=0.0, minibatch=minibatch, maxiter=epochs + 1,
                 lasso_method=lm, lasso_iter=li, lasso_tol=1.0e-5, random_seed=0,
                 mask=mask.copy() if use_mask else None)


def test_dictionary_learning_extra_cases(golden_dir):
    """float32 / complex64 runs of the reference's own test shapes and wide dictionaries
    (K = 160 / 80 atoms: several blocks of the product's blocked atom sweep)."""
    g = _load(golden_dir, 'dl_extra_golden.npz')
    cases = [str(c) for c in g['cases']]
    assert len(cases) == 48
    for name in cases:
        it, D, x = _run_dl_case(odl.solve, g, name)
        single = g[name + '/D'].dtype in (np.float32, np.complex64)
        assert D.dtype == g[name + '/D'].dtype and x.dtype == g[name + '/x'].dtype, name
        assert it == int(g[name + '/it']), name
        assert _close(D, g[name + '/D'], 2.0e-4 if single else 1.0e-9), name
        assert _close(x, g[name + '/x'], 2.0e-4 if single else 1.0e-9), name


# ------------------------------------------------------- stochastic MU NMF -----
def test_nmf_minibatch_all_cases(golden_dir):
    from oracle import nmf_minibatch as omb
    g = _load(golden_dir, 'nmf_minibatch_golden.npz')
    cases = [str(c) for c in g['cases']]
    assert len(cases) == 54
    for name in cases:
        parts = name.split('/')
        base, method = parts[0], parts[1]
        y, D0, mask = g[base + '/y'], g[base + '/D0'], g[base + '/mask']
        lik = 'kl' if base.endswith('_kl') else 'l2'
        if parts[2] == 'conv':
            it, D, x = omb.solve(y.copy(), D0.copy(), tol=3.0e-2, minibatch=30, maxiter=30,
                                 method=method, likelihood=lik, random_seed=0)
        else:
            it, D, x = omb.solve(y.copy(), D0.copy(), tol=0.0, minibatch=30,
                                 maxiter=int(parts[3][2:]), method=method, likelihood=lik,
                                 mask=mask.copy() if parts[2] == 'mask' else None, random_seed=0)
        tol = 1.0e-9 if y.dtype == np.float64 else 2.0e-4
        if y.dtype == np.float64 or parts[2] != 'conv':
            assert it == int(g[name + '/it']), name
            assert _close(D, g[name + '/D'], tol), name
            assert _close(x, g[name + '/x'], tol), name


def test_dictionary_minibatch_step_equals_solve():
    """oracle.dictionary_learning.minibatch_step (the one-step restatement the full-shape GPU gates and
    bench.py use) reproduces the per-step trace of oracle.dictionary_learning.solve -- which is pinned to the
    reference's fixtures above -- when driven with the same shuffles."""
    from oracle import dictionary_learning as odl
    from oracle.common import l2_strict
    rng = np.random.RandomState(5)
    for cplx in (False, True):
        y = rng.randn(60, 7) + (1j * rng.randn(60, 7) if cplx else 0)
        D0 = rng.randn(4, 7) + (1j * rng.randn(4, 7) if cplx else 0)
        trace = []
        odl.solve(y.copy(), D0.copy(), 0.1, tol=0.0, minibatch=20, maxiter=3, lasso_method='ista',
                  lasso_iter=10, lasso_tol=1e-5, random_seed=1, trace=trace)
        # replay: same RandomState stream, cumulative shuffles (dictionary_learning.py:131-133)
        r2 = np.random.RandomState(1)
        index = np.arange(60)
        ys, xs = y.copy(), np.ones((60, 4), dtype=D0.dtype)
        D = l2_strict(D0)
        A = np.zeros((4, 4), y.dtype)
        B = np.zeros((4, 7), y.dtype)
        count = 0
        for _ in range(2):
            r2.shuffle(index)
            ys, xs = ys[index], xs[index]
            for b in range(3):
                sl = slice(20 * b, 20 * b + 20)
                it2, xn, A, B, D, diff = odl.minibatch_step(ys[sl], xs[sl], D, A, B, count, 20, 0.1,
                                                            'ista', 10, 1e-5)
                xs[sl] = xn
                t = trace[count]
                assert it2 == t['lasso_it']
                assert np.array_equal(A, t['A']) and np.array_equal(B, t['B']) and np.array_equal(D, t['D'])
                assert diff == t['maxdiff']
                count += 1


# ------------------------------------------------- beta-divergence MU NMF -----
def test_nmf_beta_batch_and_minibatch_cases(golden_dir):
    """The oracle's beta parts reproduce the reference runs of nmf_beta_golden.npz: the batch MU cases
    (every beta, with and without a mask, 24 iterations) and the minibatch asg-mu / svrmu cases (beta = 0,
    16-row minibatches, 5 epochs).  The oracle runs in the fixture's dtype, as the reference did."""
    from oracle import nmf_minibatch as omb

    class Beta(object):      # an object spec, as decomp_amd's BetaDivergence
        def __init__(self, beta):
            self.beta = beta
    g = _load(golden_dir, 'nmf_beta_golden.npz')
    n = 0
    for si in (0, 1):
        for dt in ('float32', 'float64'):
            y, ym, D0, mask = (g['in/%d/%s/%s' % (si, dt, k)] for k in ('y', 'ym', 'D0', 'mask'))
            tol = _tol(dt)
            for beta in (0.0, 0.5, 1.5, 3.0):
                for masked in (0, 1):
                    yy, mm = (ym, mask) if masked else (y, None)
                    spec = 'is' if beta == 0.0 and masked else (Beta(beta) if si else beta)
                    it, D, x = onmf.solve(yy.copy(), D0.copy(), tol=0.0, maxiter=25, likelihood=spec,
                                          mask=None if mm is None else mm.copy())
                    key = 'mu/%d/%s/%s/%d/' % (si, dt, beta, masked)
                    assert it == 25 and D.dtype == np.dtype(dt), key
                    assert _close(D, g[key + 'D'], tol), key
                    assert _close(x, g[key + 'x'], tol), key
                    n += 1
    for dt in ('float32', 'float64'):
        y, D0 = g['in/0/%s/y' % dt], g['in/0/%s/D0' % dt]
        for method in ('asg-mu', 'svrmu'):
            trace = []
            it, D, x = omb.solve(y.copy(), D0.copy(), tol=0.0, minibatch=16, maxiter=6, method=method,
                                 likelihood='itakura-saito', random_seed=3, trace=trace)
            key = 'mb/%s/%s/' % (method, dt)
            assert it == int(g[key + 'it']), key
            assert _close(D, g[key + 'D'], _tol(dt)), key
            assert _close(x, g[key + 'x'], _tol(dt)), key
            assert len(trace) == 5 * (64 // 16) and all(t > 0 for t in trace), key
            n += 1
    assert n == 36


def test_nmf_minibatch_trace_and_beta_spec():
    """trace holds max|D - D_new| of every update, the stopping one included; beta 2 / 1 specs give the l2 /
    kl parts (the latter up to the [1, K] broadcast of the unmasked x negative part)."""
    from oracle import nmf_minibatch as omb
    rng = np.random.RandomState(2)
    y, D0 = rng.uniform(0.1, 1.0, (90, 12)), rng.uniform(0.1, 1.0, (3, 12))
    for method in ('asg-mu', 'gsag-mu', 'svrmu'):
        full = []
        omb.solve(y.copy(), D0.copy(), tol=0.0, minibatch=30, maxiter=4, method=method, random_seed=1,
                  trace=full)
        assert len(full) == (3 if method == 'gsag-mu' else 9)
        tol = 0.5 * (full[4] + full[5]) if method != 'gsag-mu' else 0.5 * (full[1] + full[2])
        stop = [i for i, t in enumerate(full) if t < tol][0]
        cut = []
        it, _, _ = omb.solve(y.copy(), D0.copy(), tol=tol, minibatch=30, maxiter=4, method=method,
                             random_seed=1, trace=cut)
        assert cut == full[:stop + 1]
        assert it == (stop // 3 + 1 if method != 'gsag-mu' else stop + 1)
    x, D = rng.uniform(0.1, 1.0, (90, 3)), D0
    for spec, name in ((2.0, 'l2'), (1.0, 'kl')):
        for mask in (None, (rng.uniform(size=y.shape) > 0.3).astype(float)):
            for parts in (onmf._parts_x, onmf._parts_d):
                a, b = parts(y, x, D, mask, spec)
                c, d = parts(y, x, D, mask, name)
                assert np.allclose(a, c, rtol=1e-12, atol=0)
                assert np.allclose(b, np.broadcast_to(d, b.shape), rtol=1e-12, atol=0)


# --------------------------------------------------------- template matching ----
def test_template_matching_solve_fixtures(golden_dir):
    """oracle.template_matching.solve reproduces every solve case recorded from the reference: the batch
    and minibatch loops, every LASSO method the fixtures hold (the dense ones and '_pos' included)."""
    from oracle import template_matching as otm
    g = _load(golden_dir, 'template_golden.npz')
    n = 0
    for name in g['solve_keys']:
        name = str(name)
        padding, stride, _, mb, method, maxiter, liter, tol, seed = [str(a) for a in g[name + '_args']]
        mb = None if mb == 'None' else int(mb)
        tol = float(tol)
        y, D0 = g[name + '_y'], g[name + '_D0']
        it, D, x = otm.solve(y.copy(), D0.copy(), 0.1, stride=int(stride), padding=padding, tol=tol,
                             minibatch=mb, size_of_minibatch=30 if mb else None, maxiter=int(maxiter),
                             lasso_method=method, lasso_iter=int(liter), random_seed=int(seed))
        it_ref, D_ref, x_ref = int(g[name + '_it']), g[name + '_D'], g[name + '_x']
        assert x.shape == x_ref.shape and D.shape == D_ref.shape, name
        n += 1
        if y.dtype in (np.float32, np.complex64):
            # the bound and the knife-edge rule of tests/test_gpu_template.py::test_solve_fixtures
            trace = g[name + '_trace']
            if it != it_ref:
                assert tol > 0 and bool(np.any(np.abs(trace - tol) < 1e-2 * tol)), (name, it, it_ref)
                continue
            lim = 2e-4
        else:
            assert it == it_ref, (name, it, it_ref)
            lim = 1e-8
        for a, b in ((D, D_ref), (x, x_ref)):
            err = float(np.max(np.abs(a - b))) / max(1e-30, float(np.max(np.abs(b))))
            assert err < lim, (name, err)
    assert n == 42


def test_template_matching_operators():
    """The closed-form operators: predict = x.A = sum over the taps of X; XXt, yX are the products of X;
    the running sums follow yX_sum += yX / it."""
    from oracle import template_matching as otm
    rng = np.random.RandomState(0)
    for S, N, s, padding in ((5, 40, 1, 'SAME'), (5, 40, 3, 'VALID'), (7, 40, 9, 'SAME'), (40, 40, 1, 'VALID')):
        C, Q = otm.geometry(S, N, s, padding)
        D = rng.randn(2, S) + 1j * rng.randn(2, S)
        x = rng.randn(3, 2, C) + 1j * rng.randn(3, 2, C)
        y = rng.randn(3, N) + 1j * rng.randn(3, N)
        A = otm.temp2mat(D, N, s, padding)
        X = otm.coef2mat(x, N, S, s, padding)
        for t in range(2):
            for c in range(C):
                for n in range(N):
                    k = n - s * c + Q
                    assert A[t, c, n] == (D[t, k] if 0 <= k < S else 0)
        p = otm.predict(x, D, N, s, padding)
        assert np.allclose(p, np.einsum('btkn,tk->bn', X, D), rtol=1e-13, atol=1e-13)
        XXt, yX = otm.statistics(y, x, S, s, padding)
        X2 = X.reshape(3, -1, N)
        assert np.allclose(XXt, np.einsum('bin,bjn->ij', X2, np.conj(X2)), rtol=1e-13, atol=1e-13)
        assert np.allclose(yX, np.einsum('bn,bin->i', y, X2), rtol=1e-13, atol=1e-13)
        X1, Y1 = otm.accumulate(XXt, yX, XXt, yX, 2)
        assert np.allclose(X1, 1.5 * XXt) and np.allclose(Y1, 1.5 * yX)

"""tests/dict_mask_ref.py (the float64 restatement test_gpu_dictionary_mask.py measures the masked step's kernels
against) pinned to oracle.dictionary_learning, the as-written restatement of the reference: the atom update against
atom_sweep_mask, and the statistics, dictionary and max|dD| of every step of a traced solve(mask=...), to 1e-12
relative.  No GPU."""
import numpy as np
import pytest

import dict_mask_ref as ref
from oracle import dictionary_learning as odl
from oracle import lasso as olasso
from oracle.common import RowBatches, l2_strict


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) / max(float(np.max(np.abs(b))), 1e-300)


@pytest.mark.parametrize('dt', ['float64', 'complex128'])
@pytest.mark.parametrize('fractional', [False, True])
def test_atom_update_equals_oracle_sweep(dt, fractional):
    p = ref.Problem(dt, 23, 19, 7, fractional, seed=4)
    A3, B = ref.stats(p.x0, p.y, p.m, p.A3_old, p.B_old, 0.75)
    # the statistics as the reference writes them (oracle/dictionary_learning.py:98-101)
    xH = np.conj(p.x0.T)
    A3_o = 0.75 * p.A3_old + np.tensordot(xH, np.expand_dims(p.x0, -2) * np.expand_dims(p.m, -1), axes=1)
    B_o = 0.75 * p.B_old + np.dot(xH, p.y * p.m)
    assert A3.shape == (7, 19, 7) and A3.dtype == p.dt and _rel(A3, A3_o) <= 1e-12 and _rel(B, B_o) <= 1e-12
    D_new, u, nrm, S = ref.atom_update(p.D, A3, B)
    D_o = odl.atom_sweep_mask(p.D, p.D, A3, B)
    assert _rel(D_new, D_o) <= 1e-12
    assert np.array_equal(D_new, u / nrm[:, None]) and np.all(nrm >= 1.0)
    # the bounds dominate the quantities they bound, and vanish where the problem promises zeros
    bA, bB = ref.stats_bounds(p.x0, p.y, p.m, p.A3_old, p.B_old, 0.75)
    assert np.all(bA >= np.abs(A3) * (1 - 1e-12)) and np.all(bB >= np.abs(B) * (1 - 1e-12))
    assert np.all(S >= np.abs(u) * (1 - 1e-12))
    assert not bA[p.kz].any() and not bA[:, :, p.kz].any() and not bB[p.kz].any()
    assert not bA[:, p.fz, :].any() and not bB[:, p.fz].any()
    assert np.count_nonzero(bA) > bA.size // 4
    # a zero code column: u_k = 0 / (F 1e-15) + D_k
    assert np.array_equal(u[p.kz], p.D[p.kz])
    assert ref.step(p.x0, p.y, p.m, p.D, p.A3_old, p.B_old, 0.75)[3] == float(np.max(np.abs(p.D - D_new)))


def test_problem_is_what_it_promises():
    for dt, frac in (('float32', False), ('complex64', True)):
        p = ref.Problem(dt, 37, 257, 17, frac, seed=1)
        assert p.D.dtype == p.dt and p.m.dtype == np.float32 and p.A3_old.shape == (17, 257, 17)
        assert np.max(np.abs(np.sum(np.abs(ref.up(p.D)) ** 2, axis=-1) - 1.0)) < 1e-6
        assert not p.x0[:, p.kz].any() and not p.A3_old[p.kz].any() and not p.A3_old[:, :, p.kz].any()
        assert not p.B_old[p.kz].any() and not p.m[:, p.fz].any() and not p.A3_old[:, p.fz].any()
        assert p.x0[0].any() and 0 < np.count_nonzero(p.x0) < p.x0.size // 2
        live = np.delete(p.m, p.fz, axis=1)
        if frac:
            assert live.min() > 0.0 and live.max() <= 1.0 and np.unique(live).size > 1000
        else:
            assert set(np.unique(live)) == {0.0, 1.0}
        assert ref.unit_roundoff(dt) == 2.0 ** -24 and ref.unit_roundoff('complex128') == 2.0 ** -53


@pytest.mark.parametrize('dt', ['float64', 'complex128'])
def test_step_equals_traced_oracle_solve(dt):
    """Every minibatch step of oracle.dictionary_learning.solve(mask=...): the helper, handed the step's inputs
    (the codes the LASSO returned, the statistics and dictionary the step before left), returns the trace's A, B,
    D and max|dD|."""
    rng = np.random.RandomState(8)
    cplx = dt == 'complex128'
    N, F, K, mb = 53, 11, 4, 12

    def randn(*s):
        return (rng.randn(*s) + 1j * rng.randn(*s)) if cplx else rng.randn(*s)
    Dt = randn(K, F)
    y = ((2.0 * randn(N, K) * (rng.uniform(size=(N, K)) < 0.4)) @ Dt + 0.1 * randn(N, F)).astype(dt)
    D0 = (Dt + 0.2 * randn(K, F)).astype(dt)
    mask = np.rint(rng.uniform(0.3, 1.0, size=(N, F)))
    kw = dict(tol=0.0, minibatch=mb, maxiter=3, lasso_method='ista', lasso_iter=7, lasso_tol=1e-6, random_seed=2)
    trace = []
    odl.solve(y.copy(), D0.copy(), 0.05, mask=mask.copy(), trace=trace, **kw)
    assert len(trace) == 2 * (N // mb)
    # the loop of oracle/dictionary_learning.py:80-110, every step restarted from the trace
    prng = np.random.RandomState(2)
    yb, xb, mk = RowBatches(y, mb), RowBatches(np.ones((N, K), dtype=dt), mb), RowBatches(mask, mb)
    index = np.arange(N)
    D, A3, B = l2_strict(D0), np.zeros((K, F, K), dtype=dt), np.zeros((K, F), dtype=dt)
    count = 0
    for it in range(1, 3):
        prng.shuffle(index)
        for b in (yb, xb, mk):
            b.shuffle(index)
        for y_mb, x_mb, m_mb in zip(yb, xb, mk):
            _, x_new = olasso.solve_fastpath(y_mb, D, 0.05, x=x_mb, tol=1e-6, maxiter=7, method='ista', mask=m_mb)
            x_mb[...] = x_new
            theta = count * mb + 1.0
            got = ref.step(x_new, y_mb, m_mb, D, A3, B, (theta - mb) / theta)
            t = trace[count]
            for a, name in zip(got[:3], ('A', 'B', 'D')):
                assert a.shape == t[name].shape and _rel(a, t[name]) <= 1e-12, (count, name, _rel(a, t[name]))
            assert abs(got[3] - t['maxdiff']) <= 1e-12 * t['maxdiff'], (count, got[3], t['maxdiff'])
            A3, B, D = t['A'], t['B'], t['D']
            count += 1
    assert count == len(trace)

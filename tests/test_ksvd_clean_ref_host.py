"""CPU: the NumPy restatement of K-SVD's atom replacement (tests/ksvd_clean_ref.py) -- it lowers the final objective
and leaves no atom unused on a start with duplicates, marks sequentially, breaks energy ties towards the lower row,
keeps the atoms it has no usable row for and does not read y at hidden entries -- the checks of
ksvd.solve(replace_atoms=, max_coherence=), which run before any GPU call, and the eight new symbols of the C ABI."""
import os
import re

import numpy as np
import pytest

import ksvd_clean_ref as cr
import ksvd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the loop ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [None, 'binary'])
def test_replacement_lowers_the_objective_and_leaves_no_atom_unused(kind):
    y, A, D0 = cr.recipe_start()
    m = cr.recipe_mask(kind)
    plain, cleaned = cr.recipe_loop(kind, False, 'double'), cr.recipe_loop(kind, True, 'double')
    o_plain = cr.objective(y, plain[-1][1], plain[-1][0], m)
    o_clean = cr.objective(y, cleaned[-1][1], cleaned[-1][0], m)
    unused_plain = int(np.sum(np.count_nonzero(plain[-1][1], axis=0) == 0))
    unused_clean = int(np.sum(np.count_nonzero(cleaned[-1][1], axis=0) == 0))
    rec = [int(np.sum(ksvd_ref.recovery(A, log[-1][0]) >= 0.99)) for log in (plain, cleaned)]
    print('%s: objective %.4f -> %.4f; unused atoms %d -> %d; planted atoms recovered %d -> %d'
          % (kind, o_plain, o_clean, unused_plain, unused_clean, rec[0], rec[1]))
    assert o_clean < o_plain
    assert unused_clean == 0
    assert cleaned[-1][3] is None                       # no pass on the iteration whose result is returned
    assert sum(len(e[3]['marked']) for e in cleaned[:-1]) >= 1
    if kind is None:                                    # the figures of the feature's description
        assert abs(o_plain - 0.0956) < 5e-5 and abs(o_clean - 0.0703) < 5e-5
        assert rec == [26, 30] and unused_plain == 1
        assert all(np.all(e[1][:, 3] == 0) for e in plain)          # the copy is never used without replacement


def test_returned_x_belongs_to_returned_D_and_the_jump_is_not_counted():
    log = cr.recipe_loop(None, True, 'double')
    first = log[0]
    assert len(first[3]['marked']) >= 1 and first[3]['replaced'].all()
    k = int(first[3]['marked'][0])
    assert not np.array_equal(first[0][k], first[4][k])               # replaced after the sweep
    y, _, D0 = cr.recipe_start()
    assert first[2] == float(np.max(np.abs(first[4] - ksvd_ref.normalise(D0))))   # maxdiff is the sweep's
    assert np.array_equal(log[-1][0], log[-1][4])


# ---- marking ----------------------------------------------------------------------------------------------------
def _gram(K, pairs, value=0.995):
    G = np.eye(K, dtype=np.result_type(value, np.float64))
    for a, b in pairs:
        G[a, b] = G[b, a] = value
    return G


def test_marking_rule_on_hand_made_gram_patterns():
    ones = np.ones(5, dtype=int)
    marked, margin = cr.mark(_gram(5, [(0, 1), (1, 2)]), ones, 0.99)           # a chain: only the middle
    assert list(marked) == [1] and abs(margin - 0.005) < 1e-12
    assert list(cr.mark(_gram(5, [(1, 3)]), ones, 0.99)[0]) == [3]              # a pair: the higher index
    assert list(cr.mark(_gram(5, [(1, 3)], -0.995), ones, 0.99)[0]) == [3]      # the sign does not matter
    assert list(cr.mark(_gram(5, [(1, 3)], 0.995j), ones, 0.99)[0]) == [3]
    cnt = ones.copy()
    cnt[1] = 0
    assert list(cr.mark(_gram(5, [(0, 1), (1, 2)]), cnt, 0.99)[0]) == [1]       # an unused atom marks no neighbour
    assert list(cr.mark(_gram(5, [(0, 1), (1, 2), (0, 2)]), ones, 0.99)[0]) == [1, 2]
    assert list(cr.mark(_gram(5, [(0, 1), (1, 2)]), cnt, None)[0]) == [1]       # no threshold: unused atoms only
    assert list(cr.mark(_gram(5, [(0, 1)]), ones, None)[0]) == []
    assert list(cr.mark(_gram(5, [(0, 1)], 0.99), ones, 0.99)[0]) == []         # strictly above the threshold


# ---- ranking and replacement --------------------------------------------------------------------------------------
def _tiny(N=6, F=5, K=4, seed=0):
    rng = np.random.RandomState(seed)
    D = ksvd_ref.normalise(rng.randn(K, F))
    x = np.zeros((N, K))
    x[:, 0] = 1.0                                           # atoms 1 .. K-1 are unused
    y = rng.randn(N, F)
    return y, x, D


def test_energy_ties_go_to_the_lower_row():
    top, margin = cr.rank(np.array([1.0, 3.0, 3.0, 0.5, 3.0]), 2)
    assert list(top) == [1, 2] and margin == 0.0
    y, x, D = _tiny()
    y[:] = y[0]                                             # identical rows: identical residuals
    Dn, info = cr.clean(y, x, D, y - x @ D, None, 0.99)
    assert list(info['marked']) == [1, 2, 3] and list(info['rows']) == [0, 1, 2]


def test_more_marked_atoms_than_rows_with_energy():
    y, x, D = _tiny()
    R = y - x @ D
    R[[0, 2, 3, 5]] = 0.0                                   # two rows with energy
    Dn, info = cr.clean(y, x, D, R, None, 0.99)
    assert list(info['marked']) == [1, 2, 3] and list(info['replaced']) == [True, True, False]
    assert set(info['rows'][:2]) == {1, 4}
    assert np.array_equal(Dn[3], D[3]) and np.array_equal(Dn[0], D[0])
    for k, i in zip(info['marked'][:2], info['rows'][:2]):
        assert np.allclose(Dn[k], y[i] / np.linalg.norm(y[i]), atol=1e-15)
    # fewer rows than marked atoms
    Dn, info = cr.clean(y[:2], x[:2], D, R[:2], None, 0.99)
    assert list(info['rows']) == [1, 0, -1] and list(info['replaced']) == [True, False, False]
    # a NaN energy keeps the atom
    R2 = y - x @ D
    R2[1, 2] = np.nan
    assert 1 not in cr.clean(y, x, D, R2, None, 0.99)[1]['rows'][:3]


def test_fills_do_not_see_each_other_and_come_from_the_rows_own_codes():
    y, x, D = _tiny(K=3)
    x[:, 1] = 0.5                                           # only atom 2 is unused; make atom 1 a copy of atom 0
    D[1] = D[0]
    m = np.ones_like(y)
    m[:, 1] = 0.0
    R = y - x @ D
    Dn, info = cr.clean(y, x, D, R, m, 0.99)
    assert list(info['marked']) == [1, 2]
    for k, i in zip(info['marked'], info['rows']):
        z = y[i].copy()
        z[1] = x[i] @ D[:, 1]                               # the old D, also for the second atom
        assert np.allclose(Dn[k], z / np.linalg.norm(z), atol=1e-15)


@pytest.mark.parametrize('kind', ['binary', 'weights'])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_y_at_hidden_entries_does_not_reach_the_result(kind, dt):
    import ksvd_mask_ref as mr
    y, x, D, m = mr.sweep_inputs(1, kind, 'random')
    x = x.copy()
    x[:, [4, 9]] = 0
    D = D.copy()
    D[7] = D[2]
    y2 = np.where(m > 0, y, 1e30)
    out = []
    for yy in (y, y2):
        yy, xx, DD = yy.astype(dt), x.astype(dt), D.astype(dt)
        out.append(cr.clean(yy, xx, DD, yy - xx @ DD, m, 0.99))       # R holds 1e30 at the hidden entries
    assert list(out[0][1]['marked']) == [4, 7, 9] and out[0][1]['replaced'].all()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1]['rows'], out[1][1]['rows'])


# ---- argument checks before any GPU call ------------------------------------------------------------------------
def _problem(dtype=np.float32, K=6):
    rng = np.random.RandomState(0)
    return rng.randn(40, 12).astype(dtype), rng.randn(K, 12).astype(dtype)


class _Reached(Exception):
    pass


@pytest.fixture
def no_gpu(monkeypatch):
    from decomp_amd import _arrays, _hip

    def boom(*a, **k):
        raise AssertionError('a GPU call was made before the argument check')
    monkeypatch.setattr(_arrays, 'to_device', boom)
    monkeypatch.setattr(_hip, 'load', boom)


def test_keyword_errors_before_any_gpu_call(no_gpu):
    from decomp_amd import ksvd
    y, D = _problem()
    for bad in (1, 0, 'yes', None, 1.0):
        with pytest.raises(ValueError, match='replace_atoms'):
            ksvd.solve(y, D, 3, replace_atoms=bad)
    for bad in (0.0, 1.0, -0.5, 1.5, float('nan'), float('inf'), '0.9', True, 1j):
        for rep in (False, True):                           # validated also where it has no effect
            with pytest.raises(ValueError, match='max_coherence'):
                ksvd.solve(y, D, 3, replace_atoms=rep, max_coherence=bad)
    for good in (0.5, 0.99, np.float32(0.9), None):
        with pytest.raises(AssertionError, match='GPU call'):
            ksvd.solve(y, D, 3, replace_atoms=True, max_coherence=good)
    with pytest.raises(AssertionError, match='GPU call'):
        ksvd.solve(y, D, 3, replace_atoms=np.bool_(True), mask=np.ones_like(y))


def test_dictionary_learning_does_not_take_the_new_keywords(no_gpu):
    from decomp_amd import dictionary_learning as dl
    y, D = _problem()
    with pytest.raises(TypeError):
        dl.solve(y, D, 0, method='ksvd', lasso_method='omp', lasso_iter=3, lasso_tol=None, replace_atoms=True)


def _entry_reached(monkeypatch, **kw):
    """The name of the library entry ksvd.solve calls first and the arguments after the handle, with host tensors
    standing in for device ones."""
    import torch
    from decomp_amd import _arrays, ksvd

    class Lib:
        def __getattr__(self, name):
            def call(h, *args):
                raise _Reached(name, args)
            return call
    monkeypatch.setattr(_arrays, 'to_device',
                        lambda a, device=None, copy=False: None if a is None else torch.from_numpy(np.array(a)))
    monkeypatch.setattr(_arrays, 'lib_handle', lambda t: (Lib(), None))
    monkeypatch.setattr(_arrays, 'l2_normalize_', lambda t, strict: t)
    y, D = _problem()
    with pytest.raises(_Reached) as e:
        ksvd.solve(y, D, 3, **kw)
    return e.value.args


def test_replace_atoms_false_reaches_the_gpu_with_todays_entry_name(monkeypatch):
    name, args = _entry_reached(monkeypatch)
    assert name == 'dcp_ksvd_step_f32' and len(args) + 1 == 11
    name, args = _entry_reached(monkeypatch, replace_atoms=False, max_coherence=0.5)
    assert name == 'dcp_ksvd_step_f32' and len(args) + 1 == 11
    name, args = _entry_reached(monkeypatch, mask=np.ones((40, 12), dtype=np.float32), replace_atoms=False)
    assert name == 'dcp_ksvd_mask_step_f32' and len(args) + 1 == 14
    name, args = _entry_reached(monkeypatch, replace_atoms=True, tol=0.25, maxiter=3)
    assert name == 'dcp_ksvd_clean_step_f32' and len(args) + 1 == 17
    assert args[2] == 0 and args[1].value is None                   # no mask: null, mask_ndim 0
    assert args[13] == 0.99 and args[14] == 0.25                    # max_coherence, stop_tol = tol
    name, args = _entry_reached(monkeypatch, replace_atoms=True, max_coherence=None, maxiter=2)
    assert args[13] == 0.0 and args[14] == float('inf')             # the last iteration allowed: never clean
    name, args = _entry_reached(monkeypatch, replace_atoms=True, mask=np.ones(12, dtype=np.float32))
    assert name == 'dcp_ksvd_clean_step_f32' and args[2] == 1 and args[1].value is not None


# ---- the C ABI lists the new entry points -----------------------------------------------------------------------
NEW_SYMBOLS = ['dcp_ksvd_clean_%s%s' % (what, sfx) for what in ('', 'step_') for sfx in ('f32', 'f64', 'c64', 'c128')]


def test_header_signatures_and_library_list_the_new_symbols():
    from decomp_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'decomp_hip.h')).read()
    assert len(NEW_SYMBOLS) == 8
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint %s\(dcp_handle\* h,' % name, header), name
        assert name in _hip.SIGNATURES, name
        n_args = len(_hip.SIGNATURES[name][1])
        assert n_args == (17 if '_step_' in name else 12), (name, n_args)
    # the pinned counts of the entries this one stands on
    assert all(len(_hip.SIGNATURES['dcp_ksvd_mask_step_' + s][1]) == 14 for s in ('f32', 'f64', 'c64', 'c128'))
    assert all(len(_hip.SIGNATURES['dcp_ksvd_mask_sweep_' + s][1]) == 11 for s in ('f32', 'f64', 'c64', 'c128'))
    if not os.path.exists(_hip.LIB_PATH):
        pytest.fail('libdecomp_hip.so is not built: %s' % _hip.LIB_PATH)
    import ctypes
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name

"""GPU: replacement of unused and duplicate atoms in K-SVD (decomp_amd.ksvd.solve(replace_atoms=True),
dcp_ksvd_clean_*, dcp_ksvd_clean_step_*) against the NumPy reference of ksvd_clean_ref.py.

The pass makes two kinds of discrete decisions: |G_kj| > mu and the order of the row energies.  A case is compared
only where the reference's two margins (the closest |G_kj| to mu, the smallest relative gap between consecutive
energies up to the first row not selected) exceed 64 eps of the working dtype; the inputs are built so that they do
(duplicates at |G| ~ 1, every other |G| < 0.9, rows scaled to distinct energies), and that is asserted, not skipped.
Then the marked set and the chosen rows must be the reference's exactly, and the new atoms equal within the
bounds_against convention: 4 x the difference between the NumPy pass in the working dtype and in double, floor 64 eps.
The entry returns D, not the rows: a replaced atom within that bound of the reference's z_i / |z_i| -- rows are
scaled random vectors, so no other row's direction is near -- identifies row i."""
import ctypes
import os
import re

import numpy as np
import pytest

import ksvd_clean_ref as cr
import ksvd_mask_ref as mr
import ksvd_ref
import omp_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ['float32', 'float64', 'complex64', 'complex128']
ERR_INVALID = -1
MU = cr.MU


def _constant(name, header):
    text = open(os.path.join(ROOT, 'decomp_amd', 'csrc', header)).read()
    return int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1))


SB = _constant('kKsvdSelBlock', 'ksvd_clean.hpp')     # rows per workgroup of the selection
LDS_BYTES = _constant('kKsvdLdsBytes', 'ksvd.hpp')


def _real(dt):
    return np.zeros(1, dtype=dt).real.dtype


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mask_dev(m, dt, offset=0):
    import torch
    if m is None:
        return None
    mt = _dev(np.asarray(m).astype(_real(dt)))
    if offset:
        whole = torch.zeros(mt.numel() + offset, dtype=mt.dtype, device=mt.device)
        whole[offset:] = mt.reshape(-1)
        mt = whole[offset:].view(mt.shape)
        assert mt.is_contiguous() and mt.data_ptr() % 16 != 0
    return mt


def _clean(y, m, x, D, mu=MU, expect_rc=0, mask_ndim=None, mask_offset=0, null=()):
    """dcp_ksvd_clean_* on host arrays: (D, n_marked, n_replaced, x after the call)."""
    from decomp_amd import _arrays, _hip
    yt, xt, Dt = _dev(y), _dev(x), _dev(D)
    mt = _mask_dev(m, y.dtype, mask_offset)
    N, F = y.shape
    K = D.shape[0]
    lib, h = _arrays.lib_handle(yt)
    nm, nr = ctypes.c_int(-1), ctypes.c_int(-1)
    name = 'dcp_ksvd_clean_' + _arrays.suffix(yt)
    ndim = (0 if mt is None else mt.dim()) if mask_ndim is None else mask_ndim
    p = lambda t, who: _arrays.ptr(None if who in null else t)          # noqa: E731
    rc = getattr(lib, name)(h, p(yt, 'y'), p(mt, 'm'), ndim, p(xt, 'x'), p(Dt, 'D'), N, F, K, float(mu),
                            None if 'nm' in null else ctypes.byref(nm), None if 'nr' in null else ctypes.byref(nr))
    if expect_rc != 0:
        assert rc == expect_rc, rc
        return Dt.cpu().numpy(), lib.dcp_last_error_string(h).decode(), None, xt.cpu().numpy()
    _hip.check(h, rc, name)
    return Dt.cpu().numpy(), nm.value, nr.value, xt.cpu().numpy()


def _step(y, m, D, s, clean=None, rows_per_pass=0):
    """One step on host arrays: dcp_ksvd_step_* / dcp_ksvd_mask_step_* (clean None) or dcp_ksvd_clean_step_* with
    clean = (max_coherence, stop_tol): (x, D, maxdiff, it, n_marked)."""
    import torch
    from decomp_amd import _arrays, _hip
    yt, Dt = _dev(y), _dev(D)
    mt = _mask_dev(m, y.dtype)
    N, F = y.shape
    K = D.shape[0]
    xt = torch.full((N, K), float('nan'), dtype=yt.dtype, device=yt.device)
    lib, h = _arrays.lib_handle(yt)
    md, it, nm = ctypes.c_double(-1.0), ctypes.c_int(-1), ctypes.c_int(-1)
    sfx = _arrays.suffix(yt)
    tail = (ctypes.byref(md), ctypes.byref(it))
    if clean is not None:
        name = 'dcp_ksvd_clean_step_' + sfx
        args = (_arrays.ptr(yt), _arrays.ptr(mt), 0 if mt is None else mt.dim(), _arrays.ptr(xt), _arrays.ptr(Dt), N, F,
                K, int(s), -1.0, int(rows_per_pass)) + tail + (float(clean[0]), float(clean[1]), ctypes.byref(nm))
    elif mt is None:
        name = 'dcp_ksvd_step_' + sfx
        args = (_arrays.ptr(yt), _arrays.ptr(xt), _arrays.ptr(Dt), N, F, K, int(s), -1.0) + tail
    else:
        name = 'dcp_ksvd_mask_step_' + sfx
        args = (_arrays.ptr(yt), _arrays.ptr(mt), mt.dim(), _arrays.ptr(xt), _arrays.ptr(Dt), N, F, K, int(s), -1.0,
                int(rows_per_pass)) + tail
    _hip.check(h, getattr(lib, name)(h, *args), name)
    return xt.cpu().numpy(), Dt.cpu().numpy(), md.value, it.value, nm.value


# ---- inputs with a known residual -------------------------------------------------------------------------------
def _random(rng, cplx, *shape):
    return rng.randn(*shape) + 1j * rng.randn(*shape) if cplx else rng.randn(*shape)


def _build(seed, N, F, K, cplx, copies=(), near=(), unused=(), mask=None, fill=0.3):
    """(y, x, D, m) in double, single-exact.  D: random unit atoms, then D[b] = D[a] for (a, b) in copies and
    D[b] = D[a] + 1e-3 noise for (a, b) in near.  x: about fill * N non-zeros per column, the columns in `unused`
    empty.  y: random rows, row i scaled by a factor of its own (1 .. 3, shuffled), so the residual energies are
    distinct.  mask: None, '1d', '2d' (weights in [0.25, 1), 30 % zeros)."""
    rng = np.random.RandomState(seed)
    D = ksvd_ref.normalise(_random(rng, cplx, K, F))
    for a, b in copies:
        D[b] = D[a]
    for a, b in near:
        D[b] = ksvd_ref.normalise((D[a] + 1e-3 * _random(rng, cplx, F))[None])[0]
    x = _random(rng, cplx, N, K) * (rng.rand(N, K) < fill)
    x[0, :] = 1.0                                                   # every column is used ...
    x[:, list(unused)] = 0                                          # ... but these
    y = _random(rng, cplx, N, F) * rng.permutation(1.0 + 2.0 * np.arange(N) / max(N, 1))[:, None]
    y, D = omp_ref.single_exact(y, D)
    x = omp_ref.single_exact(x, x)[0]
    m = None
    if mask is not None:
        shape = (F,) if mask == '1d' else (N, F)
        m = np.where(rng.rand(*shape) < mr.KEEP, 0.25 + 0.75 * rng.rand(*shape), 0)
        m = m.astype(np.float32).astype(np.float64)
    return y, x, D, m


def _check(dt, y, x, D, m, tag, mu=MU, ties=False, **kw):
    """One pass on the GPU against the reference in double; returns (D of the GPU, the reference's info)."""
    dt = np.dtype(dt)
    eps = float(np.finfo(dt).eps)
    yw, xw, Dw = y.astype(dt), x.astype(dt), D.astype(dt)
    Dr, info = cr.clean(y, x, D, y - x @ D, m, mu)
    Dn, info_w = cr.clean(yw, xw, Dw, yw - xw @ Dw, m, mu)
    # admissible: the reference's decisions are not within rounding of the other outcome
    assert info['coherence_margin'] > 64 * eps, (tag, info['coherence_margin'])
    if not ties:
        assert info['energy_margin'] > 64 * eps, (tag, info['energy_margin'])
    assert np.array_equal(info['marked'], info_w['marked']) and np.array_equal(info['rows'], info_w['rows'])
    bound = max(4 * float(np.max(np.abs(Dn - Dr))), 64 * eps)
    Dg, n_marked, n_replaced, xg = _clean(yw, m, xw, Dw, mu=mu if mu is not None else 0.0, **kw)
    err = float(np.max(np.abs(Dg - Dr))) if D.size else 0.0
    print('%s %s: marked %s rows %s; margins %.3g / %.3g; D error %.3g (bound %.3g)'
          % (tag, dt.name, list(info['marked']), list(info['rows']), info['coherence_margin'], info['energy_margin'],
             err, bound))
    assert Dg.dtype == dt and np.array_equal(xg, xw)                           # X is not touched
    assert n_marked == len(info['marked'])
    assert n_replaced == int(info['replaced'].sum())
    replaced = set(int(k) for k in info['marked'][info['replaced']])
    for k in range(D.shape[0]):
        if k in replaced:
            assert np.array_equal(Dg[k], Dw[k]) == np.array_equal(Dn[k], Dw[k]), 'atom %d was not replaced' % k
            assert abs(float(np.linalg.norm(Dg[k].astype(y.dtype))) - 1.0) <= 64 * eps
        else:
            assert np.array_equal(Dg[k], Dw[k]), 'atom %d is not to be replaced but changed' % k
    assert err <= bound
    return Dg, info


# ---- 1: the marked set, the chosen rows and the new atoms ---------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('F', [1, 37, 64, 257])
@pytest.mark.parametrize('mask', [None, '2d'])
def test_marked_set_rows_and_new_atoms(dt, F, mask):
    """N = 300, K = 7: atom 3 a copy of atom 0, atom 5 a near copy of atom 1, atom 6 unused.  F = 1 makes every atom
    parallel to atom 0: all but atom 0 are marked."""
    cplx = np.dtype(dt).kind == 'c'
    y, x, D, m = _build(300 + F, 300, F, 7, cplx, copies=[(0, 3)], near=[(1, 5)], unused=[6], mask=mask)
    Dg, info = _check(dt, y, x, D, m, 'F = %d mask %s' % (F, mask))
    assert list(info['marked']) == ([3, 5, 6] if F > 1 else [1, 2, 3, 4, 5, 6])
    if F > 1:
        assert info['replaced'].all()
        if mask is None:                                    # the row, explicitly: the nearest direction among all rows
            yn = ksvd_ref.normalise(y)
            for k, i in zip(info['marked'], info['rows']):
                assert int(np.argmax(np.abs(yn @ Dg[k].astype(y.dtype).conj()))) == i


def test_row_longer_than_the_lds_slice():
    F = 4100
    assert F * 16 > LDS_BYTES
    y, x, D, m = _build(411, 40, F, 3, True, copies=[(0, 1)], unused=[2], mask='2d')
    _, info = _check('complex128', y, x, D, m, 'F = %d' % F)
    assert list(info['marked']) == [1, 2]


@pytest.mark.parametrize('dt', DTYPES)
def test_one_row_one_atom_and_fewer_rows_than_marked_atoms(dt):
    cplx = np.dtype(dt).kind == 'c'
    y, x, D, m = _build(421, 1, 20, 3, cplx, copies=[(0, 1)], unused=[2], mask='2d')
    m[0, 0], m[0, 1] = 0.5, 0.0
    _, info = _check(dt, y, x, D, m, 'N = 1')                               # two marked atoms, one row
    assert list(info['marked']) == [1, 2] and list(info['rows']) == [0, -1]
    assert list(info['replaced']) == [True, False]
    y, x, D, m = _build(422, 30, 20, 1, cplx, unused=[0])
    _, info = _check(dt, y, x, D, None, 'K = 1, unused')                    # n_marked = K
    assert list(info['marked']) == [0] and info['replaced'].all()
    y, x, D, m = _build(423, 30, 20, 1, cplx)
    _, info = _check(dt, y, x, D, None, 'K = 1, used')                      # n_marked = 0
    assert list(info['marked']) == []
    y, x, D, m = _build(424, 2, 9, 7, cplx, unused=range(7))                # x = 0: all K marked, two rows
    _, info = _check(dt, y, x, D, None, 'N = 2 < n_marked = 7')
    assert list(info['marked']) == list(range(7)) and int(info['replaced'].sum()) == 2
    assert list(info['rows'][2:]) == [-1] * 5


@pytest.mark.parametrize('dt', ['float32', 'complex128'])
def test_nothing_marked_leaves_d_bitwise(dt):
    y, x, D, m = _build(431, 300, 37, 7, np.dtype(dt).kind == 'c', mask='2d')
    _, info = _check(dt, y, x, D, m, 'nothing marked')
    assert list(info['marked']) == []
    # a copy is not marked without a threshold
    y, x, D, m = _build(432, 300, 37, 7, np.dtype(dt).kind == 'c', copies=[(0, 3)], unused=[2])
    _, info = _check(dt, y, x, D, None, 'no threshold', mu=None)
    assert list(info['marked']) == [2]


@pytest.mark.parametrize('dt', ['float32', 'float64'])
def test_one_row_more_than_the_selection_block(dt):
    """N = SB + 1: the last row is alone in the second workgroup and has the largest energy, the last row of the
    first workgroup the second largest."""
    N = SB + 1
    y, x, D, m = _build(441, N, 8, 7, False, copies=[(0, 3), (1, 5)], unused=[6], fill=0.02)
    y, x = y.copy(), x.copy()
    x[[SB - 1, N - 1]] = 0                                  # their residual is y
    top = float(np.max(np.sum((y - x @ D) ** 2, axis=1)))
    y[N - 1] *= np.float32(np.sqrt(1.5 * top / np.sum(y[N - 1] ** 2)))
    y[SB - 1] *= np.float32(np.sqrt(1.2 * top / np.sum(y[SB - 1] ** 2)))
    _, info = _check(dt, y, x, D, None, 'N = SB + 1')
    assert list(info['marked']) == [3, 5, 6] and list(info['rows'][:2]) == [N - 1, SB - 1]


@pytest.mark.parametrize('ndim', [1, 2])
@pytest.mark.parametrize('offset', [0, 1])
def test_mask_shapes_and_base_pointer_off_16_bytes(ndim, offset):
    """float64, F = 64: the rows allow 16-byte loads; with the mask 8 bytes off a 16-byte boundary the energies take
    the scalar path.  Both give the reference's result."""
    y, x, D, m = _build(451, 300, 64, 7, False, copies=[(2, 4)], unused=[1], mask='1d' if ndim == 1 else '2d')
    _, info = _check('float64', y, x, D, m, 'mask_ndim %d offset %d' % (ndim, offset), mask_offset=offset)
    assert list(info['marked']) == [1, 4] and info['replaced'].all()


@pytest.mark.parametrize('dt', DTYPES)
def test_all_zero_mask_row_is_never_chosen(dt):
    cplx = np.dtype(dt).kind == 'c'
    y, x, D, m = _build(461, 300, 37, 7, cplx, copies=[(0, 3)], unused=[6], mask='2d')
    y = y.copy()
    y[17] *= 1000.0                                         # by far the largest residual, all of it hidden
    m[17, :] = 0.0
    _, info = _check(dt, y, x, D, m, 'hidden top row')
    assert 17 not in list(info['rows']) and info['replaced'].all()
    # every row hidden: nothing has energy, every marked atom is kept
    Dg, info = _check(dt, y, x, D, np.zeros_like(m), 'all hidden')
    assert list(info['marked']) == [3, 6] and not info['replaced'].any()


# ---- 2: ties, repeatability, hidden entries ---------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
def test_energy_ties_go_to_the_lower_row(dt):
    """Rows with x = 0 whose y differ by signs alone have bitwise equal residual energies, whatever the summation
    order, and different directions, so the new atoms show which rows were taken.  The tied rows sit in both
    selection workgroups and at their border; three atoms are marked, four rows tie for the top."""
    cplx = np.dtype(dt).kind == 'c'
    N = SB + 6
    y, x, D, m = _build(471, N, 12, 7, cplx, unused=[2, 4, 6], fill=0.02)
    y, x = y.copy(), x.copy()
    tied = [5, SB - 1, SB, SB + 5]
    signs = np.where(np.random.RandomState(3).rand(4, 12) < 0.5, -1.0, 1.0)
    base = 50.0 * y[5]
    for t, i in enumerate(tied):
        y[i] = base * signs[t]
    x[tied] = 0
    _, info = _check(dt, y, x, D, None, 'ties', ties=True)
    assert info['energy_margin'] == 0.0
    assert list(info['marked']) == [2, 4, 6] and list(info['rows']) == tied[:3]
    # the same under a mask that hides the same column in every tied row
    m = np.ones((N, 12))
    m[tied, 4] = 0.0
    _, info = _check(dt, y, x, D, m, 'ties, masked', ties=True)
    assert list(info['rows']) == tied[:3]


@pytest.mark.parametrize('dt', DTYPES)
def test_bitwise_repeatable(dt):
    cplx = np.dtype(dt).kind == 'c'
    y, x, D, m = _build(481, 300, 64, 7, cplx, copies=[(0, 3)], near=[(1, 5)], unused=[6], mask='2d')
    dt = np.dtype(dt)
    a = _clean(y.astype(dt), m, x.astype(dt), D.astype(dt))
    b = _clean(y.astype(dt), m, x.astype(dt), D.astype(dt))
    assert a[1] == b[1] == 3 and a[2] == b[2] == 3 and a[0].tobytes() == b[0].tobytes()


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('mask', ['1d', '2d'])
def test_y_at_hidden_entries_does_not_reach_d(dt, mask):
    cplx = np.dtype(dt).kind == 'c'
    dt = np.dtype(dt)
    y, x, D, m = _build(491, 300, 64, 7, cplx, copies=[(0, 3)], near=[(1, 5)], unused=[6], mask=mask)
    hidden = np.broadcast_to(m, y.shape) == 0
    assert hidden.any()
    poisoned = np.where(hidden, 1e30, y)
    a = _clean(y.astype(dt), m, x.astype(dt), D.astype(dt))
    b = _clean(poisoned.astype(dt), m, x.astype(dt), D.astype(dt))
    assert a[1] == b[1] == 3 and a[2] == b[2] == 3
    assert np.all(np.isfinite(b[0])) and a[0].tobytes() == b[0].tobytes()


# ---- 3: the step entry ------------------------------------------------------------------------------------------
def _recipe(dt, kind):
    """(y, the start normalised as ksvd.solve normalises it, the mask, the sparsity)"""
    from decomp_amd import _arrays
    y, _, D0 = cr.recipe_start()
    D0 = _arrays.l2_normalize_(_dev(D0.astype(dt)), strict=True).cpu().numpy()
    m = cr.recipe_mask(kind)
    return y.astype(dt), D0, None if m is None else m.copy(), ksvd_ref.CASES[1][4]


@pytest.mark.parametrize('dt', ['float32', 'float64'])
@pytest.mark.parametrize('kind', [None, 'weights'])
def test_step_entry_without_and_with_the_pass(dt, kind):
    """stop_tol = +inf: bitwise the plain step, and the marked atoms are counted.  stop_tol = 0: bitwise the plain step
    followed by dcp_ksvd_clean_*, which recomputes R -- the residual the step maintains differs from it by rounding, far
    inside the energy margin of this input."""
    y, D0, m, S = _recipe(dt, kind)
    plain = _step(y, m, D0, S)
    off = _step(y, m, D0, S, clean=(MU, np.inf))
    assert plain[0].tobytes() == off[0].tobytes() and plain[1].tobytes() == off[1].tobytes()
    assert plain[2] == off[2] and plain[3] == off[3]
    ref = cr.recipe_loop(kind, True, 'double', cr.ITERATIONS)[0][3]
    assert ref['coherence_margin'] > 64 * np.finfo(dt).eps and ref['energy_margin'] > 64 * np.finfo(dt).eps
    assert off[4] == len(ref['marked']) >= 1
    on = _step(y, m, D0, S, clean=(MU, 0.0))
    after = _clean(y, m, plain[0], plain[1])
    assert on[4] == after[1] == off[4] and after[2] == off[4]
    assert on[0].tobytes() == plain[0].tobytes()                               # X is the plain step's
    assert on[1].tobytes() == after[0].tobytes() and on[1].tobytes() != plain[1].tobytes()
    assert on[2] == plain[2]                                                    # the jump is not in maxdiff
    # a gate above maxdiff: no pass
    gated = _step(y, m, D0, S, clean=(MU, 2.0 * plain[2]))
    assert gated[1].tobytes() == plain[1].tobytes() and gated[4] == off[4]
    # without a threshold the unused copy is still marked
    none = _step(y, m, D0, S, clean=(0.0, 0.0))
    assert none[4] == off[4] and none[1].tobytes() == on[1].tobytes()


# ---- 4: end to end ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['float32', 'float64'])
@pytest.mark.parametrize('kind', [None, 'weights'])
def test_end_to_end(dt, kind):
    """ITERATIONS iterations on the start with duplicates.  Iteration by iteration through the step entry: the marked
    and replaced atoms are the double reference's while its margins stay admissible and the coder takes the
    reference's supports; after that only the objective is compared, by the convention of the other end-to-end tests:
    <= the double reference's x (1 + m), m = 4 x the relative gap of the NumPy loop in the working dtype, floor 1e-3.
    ksvd.solve is those steps bit for bit, NumPy and torch; its x belongs to its D; with replacement the objective
    ends below the one without; maxiter = 2 never cleans."""
    import torch
    from decomp_amd import ksvd
    dt = np.dtype(dt)
    eps = float(np.finfo(dt).eps)
    precision = 'single' if dt == np.float32 else 'double'
    y64, _, D64 = cr.recipe_start()
    y, D0, m, S = _recipe(dt, kind)
    n = cr.ITERATIONS
    ref = cr.recipe_loop(kind, True, 'double', n)
    work = cr.recipe_loop(kind, True, precision, n)
    # the steps by hand
    D = D0
    admissible = True
    for it in range(1, n + 1):
        stop = 0.0 if it < n else np.inf
        plain = _step(y, m, D, S)
        x, D, maxdiff, _, n_marked = _step(y, m, D, S, clean=(MU, stop))
        assert x.tobytes() == plain[0].tobytes() and maxdiff == plain[2]
        info = ref[it - 1][3]
        admissible = admissible and np.array_equal(x != 0, ref[it - 1][1] != 0)   # the coder took the same supports
        if info is None:                                    # the last iteration: x belongs to D
            assert D.tobytes() == plain[1].tobytes()
            continue
        admissible = admissible and info['coherence_margin'] > 64 * eps and info['energy_margin'] > 64 * eps
        if admissible:
            changed = [k for k in range(D.shape[0]) if not np.array_equal(D[k], plain[1][k])]
            assert n_marked == len(info['marked']), it
            assert changed == [int(k) for k in info['marked'][info['replaced']]], it
        print('iteration %d: %s' % (it, 'marked %s, as the reference' % list(info['marked']) if admissible
                                    else 'not compared (supports or margins)'))
    it, Ds, xs = ksvd.solve(y, cr.recipe_start()[2].astype(dt), S, tol=0.0, maxiter=n + 1, mask=m, replace_atoms=True)
    assert it == n + 1 and Ds.tobytes() == D.tobytes() and xs.tobytes() == x.tobytes()
    mt = None if m is None else _dev(m.astype(dt))
    itt, Dt, xt = ksvd.solve(_dev(y), _dev(cr.recipe_start()[2].astype(dt)), S, tol=0.0, maxiter=n + 1, mask=mt,
                             replace_atoms=True)
    assert itt == it and isinstance(Dt, torch.Tensor) and Dt.is_cuda
    assert Dt.cpu().numpy().tobytes() == Ds.tobytes() and xt.cpu().numpy().tobytes() == xs.tobytes()
    obj = cr.objective(y64, xs, Ds, m)
    obj_ref = cr.objective(y64, ref[-1][1], ref[-1][0], m)
    obj_work = cr.objective(y64, work[-1][1], work[-1][0], m)
    tol = max(4 * abs(obj_work - obj_ref) / obj_ref, 1e-3)
    _, Dp, xp = ksvd.solve(y, cr.recipe_start()[2].astype(dt), S, tol=0.0, maxiter=n + 1, mask=m)
    obj_plain = cr.objective(y64, xp, Dp, m)
    print('%s %s: objective %.6g (reference %.6g, NumPy %s loop %.6g, m %.3g); without replacement %.6g'
          % (dt.name, kind, obj, obj_ref, precision, obj_work, tol, obj_plain))
    assert obj <= obj_ref * (1 + tol)
    assert obj < obj_plain
    assert int(np.sum(np.count_nonzero(xs, axis=0) == 0)) == 0
    # (consistency -- the returned x belongs to the returned D -- is the last iteration of the loop above: its D is
    # the plain step's, bit for bit, and ksvd.solve returns exactly that pair)
    # maxiter = 2: one iteration, the last one allowed: no pass
    a = ksvd.solve(y, cr.recipe_start()[2].astype(dt), S, tol=0.0, maxiter=2, mask=m, replace_atoms=True)
    b = ksvd.solve(y, cr.recipe_start()[2].astype(dt), S, tol=0.0, maxiter=2, mask=m)
    assert a[0] == b[0] == 2 and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


# ---- 5: ABI errors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
def test_clean_abi_errors_leave_x_and_d_untouched(dt):
    dt = np.dtype(dt)
    y, x, D, m = _build(501, 60, 24, 5, dt.kind == 'c', copies=[(0, 3)], unused=[4], mask='2d')
    y, x, D = y.astype(dt), x.astype(dt), D.astype(dt)

    def refused(what, mask=m, **kw):
        Dg, msg, _, xg = _clean(y, mask, x, D, expect_rc=ERR_INVALID, **kw)
        assert np.array_equal(xg, x) and np.array_equal(Dg, D), what
        assert msg, what
        return msg
    for bad in (-1, 3):
        assert 'mask_ndim' in refused('mask_ndim', mask_ndim=bad)
    assert 'mask_ndim' in refused('a mask with mask_ndim 0', mask_ndim=0)
    assert 'mask_ndim' in refused('no mask with mask_ndim 2', mask=None, mask_ndim=2)
    assert 'NaN' in refused('NaN threshold', mu=float('nan'))
    for who in ('y', 'x', 'D', 'nm', 'nr'):
        assert 'null' in refused('null ' + who, null=(who,))
    Dg, n_marked, n_replaced, _ = _clean(y, m, x, D)
    assert n_marked == n_replaced == 2 and not np.array_equal(Dg, D)


def test_clean_step_abi_errors():
    import torch
    from decomp_amd import _arrays
    y, x, D, m = _build(502, 50, 24, 5, False, mask='2d')
    yt, Dt, mt = (_dev(a.astype(np.float32)) for a in (y, D, m))
    xt = torch.zeros((50, 5), dtype=torch.float32, device='cuda')
    lib, h = _arrays.lib_handle(yt)
    md, it, nm = ctypes.c_double(-1.0), ctypes.c_int(-1), ctypes.c_int(-1)

    def call(M=mt, ndim=2, s=3, tol=-1.0, rpp=0, mu=MU, stop=0.0, nm_out=True):
        rc = lib.dcp_ksvd_clean_step_f32(h, _arrays.ptr(yt), _arrays.ptr(M), ndim, _arrays.ptr(xt), _arrays.ptr(Dt), 50,
                                         24, 5, s, tol, rpp, ctypes.byref(md), ctypes.byref(it), mu, stop,
                                         ctypes.byref(nm) if nm_out else None)
        return rc, lib.dcp_last_error_string(h).decode()
    D_in = Dt.clone()
    for kw, word in ((dict(ndim=0), 'mask_ndim'), (dict(ndim=3), 'mask_ndim'), (dict(ndim=-1), 'mask_ndim'),
                     (dict(M=None), 'null'), (dict(M=None, ndim=1), 'null'), (dict(s=0), 'n_nonzero'),
                     (dict(s=6), 'n_nonzero'), (dict(tol=float('nan')), 'NaN'), (dict(rpp=-1), 'rows_per_pass'),
                     (dict(mu=float('nan')), 'max_coherence'), (dict(stop=float('nan')), 'stop_tol'),
                     (dict(nm_out=False), 'null')):
        rc, msg = call(**kw)
        print(kw, '->', msg)
        assert rc == ERR_INVALID and msg, kw
        assert word.lower() in msg.lower(), (kw, msg)
        assert torch.equal(Dt, D_in) and not bool(xt.any())
    rc, msg = call()
    assert rc == 0 and nm.value == 0 and bool(xt.any())
    rc, msg = call(M=None, ndim=0)
    assert rc == 0

"""NumPy reference for the replacement of unused and duplicate atoms in K-SVD
(decomp_amd.ksvd.solve(replace_atoms=True), decomp_amd/csrc/ksvd_clean.hpp) and the problems its tests share.  Test infrastructure only.  Everything runs in the
dtype it is given.

One cleaning pass, on what a sweep leaves behind: x [N, K], D [K, F], R = y - x D, the weights m (None: 1) and
cnt_k = the non-zeros of column k of x:
  marking      k = 0 .. K-1 in order, G = D D^H: atom k is marked if cnt_k == 0, or if mu is given and there is a
               j < k, itself not marked, with |G_kj| > mu
  ranking      e_i = sum_f m_if |R_if|^2 over the entries with m_if > 0 (0 where !(e_i > 0)); rows by e descending,
               ties to the lower row
  replacement  the j-th marked atom takes the j-th row i: z = y_i where m_i > 0, x_i D elsewhere (from the row's
               non-zeros); D[k] = z / |z| if e_i > 0 and |z| > 0, else the atom is kept.  x is not touched.
The loop runs the pass at the end of an iteration that is followed by another one: maxdiff >= tol and it < maxiter - 1.
"""
import functools

import numpy as np

import ksvd_mask_ref
import ksvd_ref
import omp_mask_ref
import omp_ref

MU = 0.99
RECIPE_ITERATIONS = 12
ITERATIONS = ksvd_ref.ITERATIONS      # of the end-to-end GPU comparison


def _real_dtype(a):
    return np.zeros(1, dtype=a.dtype).real.dtype


def mark(G, cnt, mu):
    """(the marked atoms ascending, the smallest | |G_kj| - mu | over the pairs compared (inf: none))."""
    K = len(cnt)
    A = np.abs(G)
    flag = np.zeros(K, dtype=bool)
    margin = np.inf
    for k in range(K):
        if cnt[k] == 0:
            flag[k] = True
            continue
        js = np.flatnonzero(~flag[:k])
        if mu is None or js.size == 0:
            continue
        a = A[k, js]
        margin = min(margin, float(np.min(np.abs(a.astype(np.float64) - float(A.dtype.type(mu))))))
        flag[k] = bool(np.any(a > A.dtype.type(mu)))
    return np.flatnonzero(flag), margin


def energies(R, m):
    """e_i = sum_f m_if |R_if|^2 in the real dtype of R; an entry with m_if > 0 false does not enter at all."""
    if m is None:
        return np.sum(np.abs(R) ** 2, axis=1)
    m = np.broadcast_to(np.asarray(m).astype(_real_dtype(R)), R.shape)
    seen = m > 0
    with np.errstate(over='ignore', invalid='ignore'):
        return np.sum(np.where(seen, m * np.abs(np.where(seen, R, 0)) ** 2, 0), axis=1)


def rank(e, n):
    """(the first min(n, N) rows of the order (e descending, i ascending), e taken as 0 where !(e > 0); the smallest
    relative gap between consecutive energies from the first selected row to the first row not selected)."""
    key = np.where(e > 0, e, 0).astype(np.float64)
    order = np.argsort(-key, kind='stable')
    top = order[:n]
    margin = np.inf
    for r in range(min(n, len(order) - 1)):
        hi, lo = key[order[r]], key[order[r + 1]]
        if hi > 0:
            margin = min(margin, float((hi - lo) / hi))
    return top, margin


def clean(y, x, D, R, m, mu):
    """One pass on copies: (D, info).  info: marked, rows (the row each marked atom was offered, -1: none left),
    replaced (bool per marked atom), coherence_margin, energy_margin."""
    D = D.copy()
    cnt = np.count_nonzero(x, axis=0)
    marked, cmargin = mark(D @ D.conj().T, cnt, mu)
    e = energies(R, m)
    top, emargin = rank(e, len(marked))
    rows = np.full(len(marked), -1, dtype=np.int64)
    rows[:len(top)] = top
    replaced = np.zeros(len(marked), dtype=bool)
    new = {}
    mm = None if m is None else np.broadcast_to(np.asarray(m), y.shape)
    for j, k in enumerate(marked):
        i = rows[j]
        if i < 0 or not e[i] > 0:
            continue
        if mm is None:
            z = y[i].copy()
        else:
            nz = np.flatnonzero(x[i] != 0)
            z = np.where(mm[i] > 0, y[i], x[i, nz] @ D[nz])
        nrm = np.sqrt(np.sum(np.abs(z) ** 2))
        if nrm > 0:
            new[k] = z / nrm
            replaced[j] = True
    for k, d in new.items():            # every z is formed from the D of the end of the sweep
        D[k] = d
    return D, dict(marked=marked, rows=rows, replaced=replaced, coherence_margin=cmargin, energy_margin=emargin)


def solve(y, D, s, m=None, replace=True, mu=MU, tol=1e-3, maxiter=1000, coef_tol=None, log=None):
    """The loop of ksvd.solve(replace_atoms=replace): (it, D, x).  log receives per iteration
    (D after the pass, x, maxdiff, the pass's info or None, D before the pass)."""
    D = ksvd_ref.normalise(D)
    x = np.zeros((y.shape[0], D.shape[0]), dtype=D.dtype)
    m2 = None if m is None else np.ascontiguousarray(np.broadcast_to(np.asarray(m).astype(_real_dtype(D)), y.shape))
    for it in range(1, maxiter):
        if m2 is None:
            x = omp_ref.omp_lstsq(y, D, s, tol=coef_tol)[0]
            x, D_new, R = ksvd_ref.sweep(y, x, D)
        else:
            x = omp_mask_ref.reference(y, D, m2, s, tol=coef_tol)[0]
            x, D_new, R = ksvd_mask_ref.sweep(y, x, D, m2)
        maxdiff = float(np.max(np.abs(D_new - D)))
        D, swept, info = D_new, D_new, None
        if replace and it < maxiter - 1 and maxdiff >= tol:
            D, info = clean(y, x, D, R, m2, mu)
        if log is not None:
            log.append((D.copy(), x.copy(), maxdiff, info, swept.copy()))
        if maxdiff < tol:
            return it, D, x
    return maxiter, D, x


def objective(y, x, D, m):
    return ksvd_ref.objective(y, x, D) if m is None else ksvd_mask_ref.objective(y, x, D, m)


# ---- computed once per session, never modified ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def recipe_start():
    """Case 1's data with a random start that holds a duplicate (atom 3 = atom 0) and a near-duplicate
    (atom 5 = atom 1 + 1e-3 noise): (y, A, D0) in double, single-exact."""
    seed, N, F, K, S, cplx = ksvd_ref.CASES[1]
    y, A, _ = ksvd_ref.case_problem(1)
    D = ksvd_ref.random_start(101, K, F, cplx).copy()
    D[3] = D[0]
    D[5] = D[1] + 1e-3 * np.random.RandomState(7).randn(F)
    D = omp_ref.single_exact(D, D)[1]
    return omp_ref._freeze(y, A, D)


def recipe_mask(kind):
    return None if kind is None else ksvd_mask_ref.case_mask(1, kind)


@functools.lru_cache(maxsize=None)
def recipe_loop(kind, replace, precision, iterations=RECIPE_ITERATIONS):
    """`iterations` iterations of solve() on the recipe (kind: None, 'binary' or 'weights'): the log."""
    dt = omp_ref.precision_dtype(False, precision)
    y, _, D0 = recipe_start()
    log = []
    S = ksvd_ref.CASES[1][4]
    it, _, _ = solve(y.astype(dt), D0.astype(dt), S, m=recipe_mask(kind), replace=replace, tol=0.0,
                     maxiter=iterations + 1, log=log)
    assert it == iterations + 1 and len(log) == iterations
    return tuple(log)

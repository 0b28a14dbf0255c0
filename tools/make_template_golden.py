#!/usr/bin/env python3
"""Generate tests/golden/template_golden.npz from the REAL reference's template_matching module.

    python tools/make_template_golden.py --ref <path of the reference checkout> [--out tests/golden]

The reference needs ``chainer.utils.conv_nd.im2col_nd_cpu``; chainer is not installed, so empty stub
modules stand in for it (as oracle/make_golden.py does) and this script supplies a NumPy im2col of its
own.  Before anything is written, the reference's own tests/test_template.py::TestUtils run against that
stub; any failure aborts.  The reference is loaded from where it lies under the alias ``decomp_ref``;
nothing of it is copied -- the fixture holds seeded inputs and the reference's outputs only.
"""
import argparse
import importlib.util
import os
import sys
import unittest

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def im2col_nd_cpu(img, ksize, stride, pad, pval=0, cover_all=False, dilate=None):
    """1-D im2col: img [n, c, L] -> [n, c, k, out], out = (L + 2 pad - k) // s + 1."""
    (k,), (s,), (p,) = tuple(ksize), tuple(stride), tuple(pad)
    padded = np.pad(img, ((0, 0), (0, 0), (p, p)), mode='constant', constant_values=pval)
    out = (img.shape[2] + 2 * p - k) // s + 1
    idx = np.arange(k)[:, None] + s * np.arange(out)[None, :]
    return padded[:, :, idx]


def load_reference(ref_root):
    from oracle.make_golden import load_reference as load_base
    ref = load_base(ref_root)
    sys.modules['chainer.utils.conv_nd'].im2col_nd_cpu = im2col_nd_cpu
    import decomp_ref.template_matching  # noqa: F401
    return ref


def check_reference_utils(ref_root):
    """tests/test_template.py::TestUtils of the reference, run against the stub; True when all pass."""
    sys.modules.setdefault('decomp', sys.modules['decomp_ref'])
    tdir = os.path.join(ref_root, 'tests')
    spec = importlib.util.spec_from_file_location('decomp_ref_tests', os.path.join(tdir, '__init__.py'),
                                                  submodule_search_locations=[tdir])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules['decomp_ref_tests'] = pkg
    spec.loader.exec_module(pkg)
    spec = importlib.util.spec_from_file_location('decomp_ref_tests.test_template',
                                                  os.path.join(tdir, 'test_template.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules['decomp_ref_tests.test_template'] = mod
    spec.loader.exec_module(mod)
    suite = unittest.defaultTestLoader.loadTestsFromTestCase(mod.TestUtils)
    res = unittest.TextTestRunner(verbosity=1).run(suite)
    return res.wasSuccessful() and res.testsRun >= 3


# (size, n_template, template_size): the shapes of test_dot, test_valid and test_same
GEOM_SHAPES = [(99, 3, 29), (300, 4, 29), (301, 4, 29), (301, 3, 29), (301, 3, 28),
               (100, 1, 9), (101, 1, 9), (102, 1, 9), (7, 2, 3), (6, 2, 3)]


def gen_geometry(tm, data):
    rng = np.random.RandomState(0)
    keys = []
    for (size, T, S) in GEOM_SHAPES:
        for stride in (1, 2, 3, 4):
            for padding in ('VALID', 'SAME'):
                key = 'geom_%d_%d_%d_%d_%s' % (size, T, S, stride, padding)
                # small integers: every product is exact in all four dtypes, and the arrays compress
                D = rng.randint(-4, 5, size=(T, S)).astype(np.float64)
                C = tm._coef_size(S, size, stride, padding)
                x = rng.randint(-4, 5, size=(2, T, C)).astype(np.float64)
                data[key + '_C'] = np.array(C)
                data[key + '_D'] = D
                data[key + '_x'] = x
                data[key + '_predict'] = tm.predict(x, D, size, stride=stride, padding=padding)
                if size <= 102:   # the dense matrices of the long signals would not fit the budget
                    data[key + '_dmat'] = tm._temp2mat(D, size, stride, padding, np)
                    data[key + '_xmat'] = tm._coef2mat(x, size, S, stride, padding, np)
                keys.append(key)
    data['geom_keys'] = np.array(keys)


def problem(seed, batch, dtype):
    """The data recipe of the reference test (T = 3, S = 10, N = 100, stride 1, SAME)."""
    from decomp_ref import template_matching as tm
    rng = np.random.RandomState(seed)
    cplx = np.dtype(dtype).kind == 'c'

    def randn(*shape):
        v = rng.randn(*shape)
        return v + 1j * rng.randn(*shape) if cplx else v
    Dtrue = randn(3, 10) + randn(10) * 0.5
    C = tm._coef_size(10, 100, 1, 'SAME')
    shape = (3, C) if batch is None else (batch, 3, C)
    xtrue = randn(*shape)
    xtrue = xtrue * np.rint(rng.uniform(0.49, 1, size=xtrue.size).reshape(xtrue.shape))
    y = tm.predict(xtrue, Dtrue, 100, stride=1)
    y = y + randn(*y.shape) * 0.1
    D = Dtrue + randn(*Dtrue.shape) * 1.0
    return y.astype(dtype), D.astype(dtype)


# (name, dtype, padding, stride, batch (None: 1-D y), minibatch, method, maxiter, lasso_iter, tol)
SOLVE_CASES = []
for _dt in ('float32', 'float64', 'complex64', 'complex128'):
    _real = _dt.startswith('float')
    SOLVE_CASES += [
        ('a', _dt, 'SAME', 1, None, None, 'acc_ista', 5, 10, 0.0),
        ('b', _dt, 'SAME', 1, 3, None, 'ista', 4, 12, 0.0),
        ('c', _dt, 'VALID', 2, 3, None, 'fista', 4, 11, 0.0),
        ('d', _dt, 'SAME', 1, None, 3, 'acc_ista', 5, 10, 0.0),
        ('e', _dt, 'VALID', 1, 3, 4, 'ista', 4, 10, 0.0),
        ('f', _dt, 'SAME', 1, 3, None, 'acc_ista', 60, 20, 2.0e-2),
        ('g', _dt, 'SAME', 1, None, 3, 'fista', 80, 20, 3.0e-2),
        ('h', _dt, 'SAME', 1, 3, None, 'cd', 3, 5, 0.0),
        ('i', _dt, 'VALID', 1, None, None, 'parallel_cd', 3, 5, 0.0),
        ('j', _dt, 'VALID', 1, 3, 3, 'admm', 3, 5, 0.0),
    ]
    if _real:
        SOLVE_CASES.append(('k', _dt, 'SAME', 1, None, None, 'acc_ista_pos', 4, 10, 0.0))


class _Recorder(object):
    """Stands in for the reference module's ``normalize`` / ``minibatch_index`` names and records
    the templates after every outer iteration and the drawn windows."""
    def __init__(self, normalize, minibatch_index):
        self._normalize, self._mbi = normalize, minibatch_index
        self.D, self.index = [], []

    def l2_strict(self, *a, **k):
        out = self._normalize.l2_strict(*a, **k)
        self.D.append(out)
        return out

    def l2(self, *a, **k):
        out = self._normalize.l2(*a, **k)
        self.D.append(out)
        return out

    def minibatch_index(self, *a, **k):
        out = self._mbi(*a, **k)
        self.index.append(np.stack(out, 0))
        return out


def gen_solve(tm, data):
    names = []
    for seed, (tag, dt, padding, stride, batch, mb, method, maxiter, liter, tol) in enumerate(SOLVE_CASES):
        y, D0 = problem(seed, batch, dt)
        rec = _Recorder(tm.normalize, tm.minibatch_index)
        tm.normalize, tm.minibatch_index = rec, rec.minibatch_index
        try:
            it, D, x = tm.solve(y.copy(), D0.copy(), 0.1, stride=stride, padding=padding, tol=tol,
                                minibatch=mb, size_of_minibatch=30 if mb else None, maxiter=maxiter,
                                lasso_method=method, lasso_iter=liter, random_seed=seed)
        finally:
            tm.normalize, tm.minibatch_index = rec._normalize, rec._mbi
        trace = np.array([np.max(np.abs(a - b)) for a, b in zip(rec.D[:-1], rec.D[1:])])
        name = 'solve_%s_%s' % (tag, dt)
        data[name + '_y'] = y
        data[name + '_D0'] = D0
        data[name + '_D'] = D
        data[name + '_x'] = x
        data[name + '_it'] = np.array(it)
        data[name + '_trace'] = trace
        data[name + '_index'] = (np.stack(rec.index, 0).astype(np.int64) if rec.index
                                 else np.zeros((0, 2, 0), np.int64))
        data[name + '_args'] = np.array([padding, str(stride), str(batch), str(mb), method, str(maxiter),
                                         str(liter), repr(tol), str(seed)])
        names.append(name)
        print('%-28s it=%3d  last max|dD|=%.3g' % (name, it, trace[-1] if len(trace) else np.nan))
    data['solve_keys'] = np.array(names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    a = ap.parse_args()
    ref = load_reference(a.ref)
    if not check_reference_utils(a.ref):
        sys.exit('the reference TestUtils fail against the im2col stub: nothing written')
    tm = ref.template_matching
    data = {}
    gen_geometry(tm, data)
    gen_solve(tm, data)
    path = os.path.join(a.out, 'template_golden.npz')
    np.savez_compressed(path, **data)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()

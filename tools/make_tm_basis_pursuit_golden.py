#!/usr/bin/env python3
"""Generate tests/golden/tm_basis_pursuit_golden.npz from the REAL reference's lasso module.

    python tools/make_tm_basis_pursuit_golden.py --ref <path of the reference checkout> [--out tests/golden]

The reference has no multichannel templates; what template_matching.basis_pursuit promises for D [T, Ch, S] is the
reference's own ``decomp.lasso.solve`` on the dense operator A [T C, Ch N] with y flattened to [B, Ch N].  This script
records exactly that for a handful of small cases (tests/tm_basis_pursuit_ref.GOLDEN_CASES: the four dtypes, the three
methods, two '_pos' cases, 'SAME' and 'VALID', stride 1 and 2).  The reference is loaded from where it lies under the
alias ``decomp_ref`` (oracle.make_golden.load_reference); nothing of it is copied -- the fixture holds seeded inputs
and the reference's outputs only.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    a = ap.parse_args()
    from oracle.make_golden import load_reference
    ref = load_reference(a.ref)
    import tm_basis_pursuit_ref as bp
    import tm_multichannel_ref as mc
    data = {}
    for seed, (tag, dtype, method, stride, padding, maxiter, tol) in enumerate(bp.GOLDEN_CASES):
        y, D, x0, alpha = bp.golden_inputs(seed, dtype, stride, padding)
        B, Ch, N = y.shape
        A = mc.dense_operator(D, N, stride, padding)
        it, x = ref.lasso.solve(y.reshape(B, -1).copy(), A.copy(), alpha, x=x0.reshape(B, -1).copy(), tol=tol,
                                method=method, maxiter=maxiter)
        for name, v in (('y', y), ('D', D), ('x0', x0), ('alpha', np.array(alpha)), ('A', A), ('x', np.asarray(x)),
                        ('it', np.array(it))):
            data['%s_%s' % (tag, name)] = v
        print('%s %-10s %-13s stride %d %-5s it=%d nonzero %d / %d' % (tag, dtype, method, stride, padding, it,
                                                                      int(np.sum(np.asarray(x) != 0)), x.size))
    data['keys'] = np.array([c[0] for c in bp.GOLDEN_CASES])
    path = os.path.join(a.out, 'tm_basis_pursuit_golden.npz')
    np.savez_compressed(path, **data)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()

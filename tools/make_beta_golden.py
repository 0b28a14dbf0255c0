#!/usr/bin/env python3
"""Generate tests/golden/nmf_beta_golden.npz from the REAL reference (build machine only).

    python tools/make_beta_golden.py --ref REFERENCE_ROOT [--out tests/golden]

The reference is loaded with oracle.make_golden.load_reference (imported, not modified).  The beta-divergence
MU rule is defined here as a subclass of the reference's own ``grads.Likelihood`` -- its extension point --
and run through the reference's ``nmf.solve``.  The fixture holds data only: seeded inputs and the
reference's outputs.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(64, 48, 4), (101, 20, 3)]
BETAS = [0.0, 0.5, 1.5, 3.0]
DTYPES = ['float32', 'float64']
MAXITER = 25
MB_METHODS = ['asg-mu', 'svrmu']
MB_SEED, MB_SIZE, MB_MAXITER = 3, 16, 6


def beta_inputs(seed, N, F, K, dtype):
    """Positive data from a true factorisation (gamma-like multiplicative noise); zeros only where the mask
    is zero."""
    rng = np.random.RandomState(seed)
    Dt = rng.uniform(0.1, 1.0, size=(K, F))
    xt = rng.uniform(0.1, 1.0, size=(N, K))
    y = xt.dot(Dt) * rng.uniform(0.7, 1.3, size=(N, F))
    D0 = Dt * rng.uniform(0.5, 1.5, size=(K, F))
    mask = (rng.uniform(size=(N, F)) >= 0.3).astype(np.float64)
    ym = y * mask
    return y.astype(dtype), ym.astype(dtype), D0.astype(dtype), mask.astype(dtype)


def key(*parts):
    return '/'.join(str(p) for p in parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='root of the reference checkout (holds decomp/)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    a = ap.parse_args()
    from oracle.make_golden import load_reference
    ref = load_reference(a.ref)
    import decomp_ref.nmf_methods.grads as rgrads

    class RefBeta(rgrads.Likelihood):
        """The beta parts R1 = (y o M) V^(beta-2), R2 = M V^(beta-1), V = x d + 1e-15, on the reference's
        extension point; update_x / update_d are the reference's own."""
        def __init__(self, beta):
            self.beta = beta

        def _parts(self, y, x, d, mask):
            V = x.dot(d) + 1.0e-15
            if mask is None:
                return y * V ** (self.beta - 2.0), V ** (self.beta - 1.0)
            return y * mask * V ** (self.beta - 2.0), mask * V ** (self.beta - 1.0)

        def grad_x(self, y, x, d, mask):
            r1, r2 = self._parts(y, x, d, mask)
            return r1.dot(d.T), r2.dot(d.T)

        def grad_d(self, y, x, d, mask):
            r1, r2 = self._parts(y, x, d, mask)
            return x.T.dot(r1), x.T.dot(r2)

    out = {}
    for si, (N, F, K) in enumerate(SHAPES):
        for dt in DTYPES:
            y, ym, D0, mask = beta_inputs(100 + si, N, F, K, dt)
            out[key('in', si, dt, 'y')] = y
            out[key('in', si, dt, 'ym')] = ym
            out[key('in', si, dt, 'D0')] = D0
            out[key('in', si, dt, 'mask')] = mask
            for beta in BETAS:
                for masked in (0, 1):
                    yy, mm = (ym, mask) if masked else (y, None)
                    it, D, x = ref.nmf.solve(yy.copy(), D0.copy(), tol=0.0, maxiter=MAXITER,
                                             likelihood=RefBeta(beta), mask=mm)
                    assert it == MAXITER and np.all(np.isfinite(D)) and np.all(np.isfinite(x))
                    out[key('mu', si, dt, beta, masked, 'D')] = D
                    out[key('mu', si, dt, beta, masked, 'x')] = x
    # one early stop per dtype (beta = 0, unmasked, shape 0): a tol whose stopping iteration does not move
    # when tol moves by +-1 %, so that rounding cannot flip the comparison
    for dt in DTYPES:
        y, _, D0, _ = beta_inputs(100, *SHAPES[0], dt)
        chosen = None
        for tol in np.geomspace(1e-3, 3e-3, 25):
            tol = float('%.3g' % tol)
            its = [ref.nmf.solve(y.copy(), D0.copy(), tol=t, maxiter=400, likelihood=RefBeta(0.0))[0]
                   for t in (tol * 0.99, tol, tol * 1.01)]
            if its[0] == its[1] == its[2] and 2 < its[1] < 400:
                chosen = tol
                break
        assert chosen is not None
        it, D, x = ref.nmf.solve(y.copy(), D0.copy(), tol=chosen, maxiter=400, likelihood=RefBeta(0.0))
        out[key('stop', dt, 'tol')] = np.array(chosen)
        out[key('stop', dt, 'it')] = np.array(it)
        out[key('stop', dt, 'D')] = D
        out[key('stop', dt, 'x')] = x
    # minibatch methods, beta = 0, unmasked, shape 0
    for dt in DTYPES:
        y, _, D0, _ = beta_inputs(100, *SHAPES[0], dt)
        for method in MB_METHODS:
            it, D, x = ref.nmf.solve(y.copy(), D0.copy(), tol=0.0, minibatch=MB_SIZE, maxiter=MB_MAXITER,
                                     method=method, likelihood=RefBeta(0.0), random_seed=MB_SEED)
            out[key('mb', method, dt, 'it')] = np.array(it)
            out[key('mb', method, dt, 'D')] = D
            out[key('mb', method, dt, 'x')] = x
    path = os.path.join(a.out, 'nmf_beta_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()

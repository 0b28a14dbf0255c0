"""CPU: decomp_amd.template_matching -- public surface, geometry against the reference's recorded
im2col matrices (restated here in closed form, the formulas the kernels implement), minibatch draws and
argument errors raised before any GPU call."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _g():
    return np.load(os.path.join(GOLDEN, 'template_golden.npz'), allow_pickle=False)


def _parse(key):
    _, size, T, S, stride, padding = key.split('_')
    return int(size), int(T), int(S), int(stride), padding


def closed_form(S, N, stride, padding):
    pad = N - 1 if padding == 'SAME' else N - S
    C = (S + 2 * pad - N) // stride + 1
    return C, stride * (C - 1) - pad


def temp2mat_np(D, N, stride, padding):
    T, S = D.shape
    C, Q = closed_form(S, N, stride, padding)
    out = np.zeros((T, C, N), D.dtype)
    for c in range(C):
        for n in range(N):
            k = n - stride * c + Q
            if 0 <= k < S:
                out[:, c, n] = D[:, k]
    return out


def coef2mat_np(x, N, S, stride, padding):
    B, T, C = x.shape
    C2, Q = closed_form(S, N, stride, padding)
    assert C == C2
    out = np.zeros((B, T, S, N), x.dtype)
    for c in range(C):
        for k in range(S):
            n = stride * c - Q + k
            if 0 <= n < N:
                out[:, :, k, n] = x[:, :, c]
    return out


def test_public_names():
    from decomp_amd import template_matching as tm
    import decomp_amd
    assert decomp_amd.template_matching is tm
    for name in ('solve', 'solve_fastpath', 'solve_batch', 'solve_minibatch', 'predict', '_coef_size',
                 '_temp2mat', '_coef2mat', 'Minibatcher'):
        assert callable(getattr(tm, name)), name
    assert tm._JITTER == 1.0e-15
    from decomp_amd.utils.data import minibatch_index
    assert tm.minibatch_index is minibatch_index


def test_coef_size_matches_fixtures():
    from decomp_amd import template_matching as tm
    g = _g()
    for key in g['geom_keys']:
        size, T, S, stride, padding = _parse(str(key))
        assert tm._coef_size(S, size, stride, padding) == int(g[key + '_C']), key
        assert closed_form(S, size, stride, padding)[0] == int(g[key + '_C']), key


def test_closed_form_im2col_matches_reference():
    g = _g()
    n = 0
    for key in g['geom_keys']:
        key = str(key)
        if key + '_dmat' not in g.files:
            continue
        size, T, S, stride, padding = _parse(key)
        D, x = g[key + '_D'], g[key + '_x']
        np.testing.assert_array_equal(temp2mat_np(D, size, stride, padding), g[key + '_dmat'], err_msg=key)
        np.testing.assert_array_equal(coef2mat_np(x, size, S, stride, padding), g[key + '_xmat'], err_msg=key)
        # predict = x . A  (tensordot over (t, c))
        np.testing.assert_allclose(np.tensordot(x, g[key + '_dmat'], 2), g[key + '_predict'], rtol=0, atol=1e-9)
        n += 1
    assert n >= 40


def test_minibatch_index_reproduces_draws():
    from decomp_amd.utils.data import minibatch_index
    g = _g()
    n = 0
    for name in g['solve_keys']:
        name = str(name)
        idx = g[name + '_index']
        if idx.shape[0] == 0:
            continue
        args = g[name + '_args']
        mb, seed = int(args[3]), int(args[8])
        y = g[name + '_y']
        B = 1 if y.ndim == 1 else y.shape[0]
        rng = np.random.RandomState(seed)
        for draw in idx:
            rows, starts = minibatch_index((B, y.shape[-1] - 30), mb, rng)
            np.testing.assert_array_equal(rows, draw[0])
            np.testing.assert_array_equal(starts, draw[1])
        n += 1
    assert n >= 8
    sl = minibatch_index((5,), None, np.random.RandomState(0))
    assert sl == (slice(None, None, None),)


def _problem():
    rng = np.random.RandomState(0)
    return rng.randn(2, 50), rng.randn(3, 5)


def test_errors_before_any_gpu_call(monkeypatch):
    from decomp_amd import template_matching as tm, _arrays, _hip
    from decomp_amd.utils.exceptions import DtypeMismatchError

    def no_gpu(*a, **k):
        raise AssertionError('a GPU call was made before the argument check')
    monkeypatch.setattr(_arrays, 'to_device', no_gpu)
    monkeypatch.setattr(_hip, 'load', no_gpu)
    y, D = _problem()
    with pytest.raises(NotImplementedError):
        tm.solve(y, D, 0.1, mask=np.ones_like(y))
    with pytest.raises(ValueError):
        tm.solve(y, D, 0.1, minibatch=3)
    with pytest.raises(DtypeMismatchError):
        tm.solve(y, D.astype(np.float32), 0.1)
    with pytest.raises(DtypeMismatchError):
        tm.solve(y, D, 0.1, x=np.zeros((2, 3, 54), np.float32))


def test_no_cpu_fallback(monkeypatch):
    """Valid arguments without a usable GPU raise HipLibraryError: nothing is computed on the host."""
    import torch
    from decomp_amd import template_matching as tm, _hip
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    y, D = _problem()
    with pytest.raises(_hip.HipLibraryError):
        tm.solve(y, D, 0.1, maxiter=3)
    with pytest.raises(_hip.HipLibraryError):
        tm.predict(np.zeros((3, 54)), D, 50)


def _cpu_device(monkeypatch):
    """Route the module's device plumbing to host torch tensors and record the kernel calls instead of
    making them: what reaches a kernel can then be inspected without a GPU."""
    import torch
    from decomp_amd import template_matching as tm, _arrays
    calls = []

    def to_device(a, device=None, copy=False):
        if a is None:
            return None
        t = a if _arrays.is_torch(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.clone() if copy else t.contiguous()

    def record(t, name, *args):
        calls.append((name, t.dtype, [a.dtype for a in args if _arrays.is_torch(a)]))
    monkeypatch.setattr(_arrays, 'to_device', to_device)
    monkeypatch.setattr(tm, '_call', record)
    return calls


def test_predict_mixed_dtypes_are_promoted(monkeypatch):
    """predict(x, D) with x and D of different dtypes computes in the promoted dtype (the reference's
    tensordot promotes): no kernel ever receives an operand of another dtype than the one it is built for."""
    import torch
    from decomp_amd import template_matching as tm
    calls = _cpu_device(monkeypatch)
    C = tm._coef_size(5, 50, 1, 'SAME')
    cases = [(np.float64, np.float32, torch.float64), (np.float32, np.float64, torch.float64),
             (np.float32, np.complex64, torch.complex64), (np.complex64, np.float64, torch.complex128)]
    for xdt, Ddt, want in cases:
        del calls[:]
        out = tm.predict(np.zeros((2, 3, C), xdt), np.ones((3, 5), Ddt), 50)
        assert out.dtype == np.dtype({torch.float64: np.float64, torch.complex64: np.complex64,
                                      torch.complex128: np.complex128}[want])
        (name, dt, argdts), = calls
        assert name == 'predict' and dt == want and all(a == want for a in argdts), calls


def test_kernel_arguments_checked_before_the_call():
    """The single entry into the library refuses operands whose dtype or device differs from the
    problem's, before any library or GPU call."""
    import torch
    from decomp_amd import template_matching as tm
    from decomp_amd.utils.exceptions import DtypeMismatchError
    x = torch.zeros((1, 3, 54), dtype=torch.float64)
    with pytest.raises(DtypeMismatchError):
        tm._call(x, 'predict', x, torch.zeros((3, 5), dtype=torch.float32), 1, 3, 5, 50, 1, 1, x)
    with pytest.raises(ValueError):
        tm._call(x, 'predict', x, torch.zeros((5, 3), dtype=torch.float64).t(), 1, 3, 5, 50, 1, 1, x)


def test_public_loops_check_dtypes_before_any_gpu_call(monkeypatch):
    from decomp_amd import template_matching as tm, _arrays
    from decomp_amd.utils.exceptions import DtypeMismatchError

    def no_gpu(*a, **k):
        raise AssertionError('a GPU call was made before the argument check')
    monkeypatch.setattr(_arrays, 'to_device', no_gpu)
    y, D = _problem()
    x = np.zeros((2, 3, 54), np.float32)
    with pytest.raises(DtypeMismatchError):
        tm.solve_batch(y, D, 0.1, x, 1, 'SAME', 1e-4, 3, 'acc_ista', 10, 1e-5, None)
    with pytest.raises(DtypeMismatchError):
        tm.solve_minibatch(y, D, 0.1, x, 1, 'SAME', 1e-4, 3, 10, 3, 'acc_ista', 10, 1e-5,
                           np.random.RandomState(0), None)


def test_minibatch_windows_past_the_coefficients():
    """With stride > 1 a window's coefficient slice starts at the SAMPLE offset and can run past C; the
    reference fails inside np.stack with a ValueError, and so does the draw here (before any gather)."""
    from decomp_amd import template_matching as tm
    N, S, w = 100, 10, 30
    for padding in ('SAME', 'VALID'):
        C = tm._coef_size(S, N, 2, padding)
        cw = tm._coef_size(S, w, 2, padding)
        with pytest.raises(ValueError):
            tm._draw_windows(np.random.RandomState(0), 3, N, w, 3, C, cw)
    # stride 1: every start fits, and the draw is minibatch_index's
    C, cw = tm._coef_size(S, N, 1, 'SAME'), tm._coef_size(S, w, 1, 'SAME')
    rows, starts = tm._draw_windows(np.random.RandomState(0), 3, N, w, 3, C, cw)
    r2, s2 = tm.minibatch_index((3, N - w), 3, np.random.RandomState(0))
    np.testing.assert_array_equal(rows, r2)
    np.testing.assert_array_equal(starts, s2)

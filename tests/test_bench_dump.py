"""bench.py --dump-outputs on host tensors: float .npy files within 64 MB, the row sample of x fixed by its seed."""
import os

import numpy as np
import torch

import bench


def _dump(tmp_path, name, rows, K=256, F=4096):
    D = torch.arange(K * F, dtype=torch.float32).reshape(K, F)
    x = torch.arange(rows * K, dtype=torch.float32).reshape(rows, K)
    out = str(tmp_path / name)
    shapes = bench.dump_outputs(out, D, x)
    files = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert set(files) == set(shapes) and all(f.endswith('.npy') for f in os.listdir(out))
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= 64 * 10 ** 6
    np.testing.assert_array_equal(files['D'], D.numpy())
    return files, x.numpy()


def test_full_shape_dump_is_a_fixed_row_sample(tmp_path):
    a, x = _dump(tmp_path, 'a', bench.N_ROWS)
    b, _ = _dump(tmp_path, 'b', bench.N_ROWS)
    rows = a['x_rows'].astype(np.int64)
    assert a['x'].shape == (bench.DUMP_X_ROWS, bench.N_ATOMS)
    assert np.all(np.diff(rows) > 0) and rows[-1] < bench.N_ROWS
    np.testing.assert_array_equal(a['x'], x[rows])
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def test_small_x_is_written_whole(tmp_path):
    files, x = _dump(tmp_path, 'small', 1000)
    assert 'x_rows' not in files
    np.testing.assert_array_equal(files['x'], x)

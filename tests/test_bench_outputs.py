"""CPU: what `bench.py --dump-outputs DIR` writes -- every array as float64 DIR/<name>.npy, and past
the size limit the same fixed, seeded sample of the frequency axis for every array and every run."""
import os

import numpy as np

from test_bench_launcher import _import_bench


def test_small_outputs_are_written_whole(tmp_path):
    bench = _import_bench()
    rng = np.random.default_rng(1)
    F = rng.standard_normal((3, 3, 50, 2))
    infid = rng.standard_normal(3)
    n = bench.dump_outputs(str(tmp_path / 'out'), {'filter_function': F, 'infidelity': infid},
                           omega_axis={'filter_function': -2})
    assert n == F.nbytes + infid.nbytes
    got = np.load(tmp_path / 'out' / 'filter_function.npy')
    assert got.dtype == np.float64 and np.array_equal(got, F)
    assert np.array_equal(np.load(tmp_path / 'out' / 'infidelity.npy'), infid)


def test_large_outputs_keep_one_seeded_sample_of_the_frequencies(tmp_path):
    bench = _import_bench()
    W = 1000
    omega = np.arange(W, dtype=float)
    # every element carries its frequency index, so that the sample can be read back
    R = np.broadcast_to(omega[:, None], (3, 16, W, 2)).copy()
    F = np.broadcast_to(omega[:, None], (3, 3, W, 2)).copy()
    infid = np.ones(3)
    arrays = {'control_matrix': R, 'filter_function': F, 'infidelity': infid}
    limit = (R.nbytes + F.nbytes)//4
    axes = {'control_matrix': -2, 'filter_function': -2}
    n = bench.dump_outputs(str(tmp_path / 'a'), arrays, omega_axis=axes, limit=limit)
    bench.dump_outputs(str(tmp_path / 'b'), arrays, omega_axis=axes, limit=limit)
    assert n <= limit
    Ra, Fa = (np.load(tmp_path / 'a' / f'{k}.npy') for k in ('control_matrix', 'filter_function'))
    idx = Ra[0, 0, :, 0]
    assert 0 < len(idx) < W and np.all(np.diff(idx) > 0)
    assert np.array_equal(Fa[0, 0, :, 0], idx)
    assert np.array_equal(np.load(tmp_path / 'a' / 'infidelity.npy'), infid)
    for k in ('control_matrix', 'filter_function', 'infidelity'):
        assert np.array_equal(np.load(tmp_path / 'a' / f'{k}.npy'), np.load(tmp_path / 'b' / f'{k}.npy'))
    assert sorted(os.listdir(tmp_path / 'a')) == ['control_matrix.npy', 'filter_function.npy', 'infidelity.npy']

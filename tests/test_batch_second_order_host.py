"""CPU-only: the workspace and chunk queries of the batched frequency shifts (ffk_batch_frequency_shifts), the
eligibility predicate, and the grouping and pass splitting of ff.frequency_shifts on stub pulses."""
import numpy as np
import pytest

import filter_functions_amd as ff
from filter_functions_amd import _lib, batch, batch_second_order, processes

CONFIG2 = dict(W=4096, N=16, A=3, G=256, d=4, n_idx=3, s_ndim=1)


def ws_bytes(P, W, N, A, G, d, n_idx, s_ndim):
    return _lib.load().ffk_batch_frequency_shifts_workspace_bytes(P, W, N, A, G, d, n_idx, s_ndim)


def chunk(W, N, A, G, d):
    return _lib.load().ffk_batch_frequency_shifts_chunk(W, N, A, G, d)


class Stub:
    """What grouping reads of a pulse: dimension, segments, noise operators, basis."""

    def __init__(self, d, G, A, basis):
        self.c_opers = np.zeros((2, d, d))
        self.dt = np.ones(G)
        self.n_opers = np.zeros((A, d, d))
        self.basis = basis


def test_exported():
    assert 'frequency_shifts' in ff.__all__ and ff.frequency_shifts is batch_second_order.frequency_shifts
    assert 'frequency_shifts' in batch_second_order.__all__
    for name in ('ffk_batch_frequency_shifts', 'ffk_batch_frequency_shifts_chunk',
                 'ffk_batch_frequency_shifts_workspace_bytes'):
        assert name in _lib.SIGNATURES
    import inspect
    for f in (ff.cumulant_functions, ff.error_transfer_matrices):
        assert inspect.signature(f).parameters['second_order'].default is False
    assert 'second order' not in processes.decay_amplitudes.__doc__.split('not offered')[0].split('.')[-1]


@pytest.mark.parametrize('shape', [CONFIG2, dict(W=500, N=4, A=2, G=100, d=2, n_idx=2, s_ndim=2),
                                   dict(W=35, N=16, A=4, G=5, d=4, n_idx=2, s_ndim=3),
                                   dict(W=1, N=4, A=1, G=1, d=2, n_idx=1, s_ndim=1),
                                   dict(W=10, N=25, A=2, G=4, d=5, n_idx=2, s_ndim=3),
                                   dict(W=4097, N=64, A=9, G=1000, d=8, n_idx=9, s_ndim=2)])
def test_workspace_query_is_linear_in_the_pulses(shape):
    sizes = {P: ws_bytes(P, **shape) for P in (1, 2, 4, 8, 9, 64, 65535)}
    assert all(v > 0 for v in sizes.values())
    step = sizes[2] - sizes[1]
    assert step > 0
    for P, v in sizes.items():
        assert v == sizes[1] + (P - 1)*step, P


def test_a_pulse_of_config_2_takes_a_fraction_of_its_second_order_filter_function():
    W, N, A = (CONFIG2[k] for k in ('W', 'N', 'A'))
    F2 = 16*A*A*N*N*W                                   # 151 MB on the single path
    per_pulse = ws_bytes(2, **CONFIG2) - ws_bytes(1, **CONFIG2)
    assert per_pulse <= F2//8
    assert len(batch_second_order.split_group(list(range(16)), W, N, A, 256, 4, 3, 1)) == 1


def test_queries_return_zero_for_what_the_entry_refuses():
    assert ws_bytes(2, **CONFIG2) > 0
    for bad in [dict(P=0), dict(P=65536), dict(d=1), dict(d=17), dict(d=9, N=81), dict(A=0), dict(N=0), dict(W=0),
                dict(G=0), dict(n_idx=0), dict(n_idx=4), dict(s_ndim=0), dict(s_ndim=4)]:
        args = dict(CONFIG2, P=2)
        args.update(bad)
        assert ws_bytes(**args) == 0, bad
    assert chunk(0, 16, 3, 256, 4) == 0 and chunk(64, 16, 3, 0, 4) == 0 and chunk(5, 81, 1, 2, 9) == 0


def mfma_tile(AN, d):
    """the single launcher's rule, restated: the largest square wave tile (16, 32, 48 rows) whose operands fit in
    LDS twice per CU (79 KiB); 0: the vector kernel"""
    d2 = d*d
    for mt in range(min(3, -(-AN//16)), 0, -1):
        if 16*((2*16*mt + 16*mt)*(d2 + 1) + 4*(3*d2 + 6*16*mt + 2*16*mt)) <= 79*1024:
            return mt
    return 0


@pytest.mark.parametrize('d', range(2, 17))
def test_eligible_shapes_are_those_of_the_matrix_core_kernel(d):
    for A in (1, 2, 3, 9):
        for N in (d*d, 4):
            assert (chunk(64, N, A, 8, d) > 0) == (mfma_tile(A*N, d) > 0), (d, A, N)
    assert (mfma_tile(d*d, d) > 0) == (d <= 8)          # d = 6 is the dimension of the smaller tile
    assert mfma_tile(2*36, 6) == 2 and mfma_tile(3*16, 4) == 3 and mfma_tile(64, 8) == 1


def test_chunk_depends_on_the_shape_alone():
    for W in (1, 5, 35, 500, 2047):
        assert chunk(W, 16, 3, 256, 4) == chunk(35, 16, 4, 5, 4) == 16
    for W in (2048, 4096, 65536):
        assert chunk(W, 16, 3, 256, 4) == 32
    c = chunk(35, 16, 4, 5, 4)
    assert chunk(2*c + 3, 16, 4, 5, 4) == c and c % 4 == 0
    # nothing of the query's arguments is the number of pulses
    assert _lib.SIGNATURES['ffk_batch_frequency_shifts_chunk'][1].__len__() == 5


def test_grouping_by_shape_basis_and_selection():
    b2, b2_twin, b3 = ff.Basis.pauli(1), ff.Basis.pauli(1), ff.Basis.ggm(2)
    pulses = [Stub(2, 6, 2, b2), Stub(2, 7, 2, b2), Stub(2, 6, 2, b2_twin), Stub(2, 6, 2, b3), Stub(2, 6, 3, b2),
              Stub(2, 6, 2, b2), Stub(2, 7, 2, b2)]
    idx_of = [[0, 1]]*5 + [[1]] + [[0, 1]]
    groups = batch_second_order.group_members(pulses, range(len(pulses)), idx_of)
    assert groups == [[0, 2], [1, 6], [3], [4], [5]]
    assert batch_second_order.group_members(pulses, [6, 2, 0], idx_of) == [[2, 0], [6]]


def test_groups_are_split_by_the_workspace_query():
    W, N, A, G, d = 4096, 16, 3, 256, 4
    per_pulse, fixed = batch_second_order.pulse_bytes(W, N, A, G, d, 3, 1)
    assert per_pulse == ws_bytes(2, **CONFIG2) - ws_bytes(1, **CONFIG2) and fixed + per_pulse == ws_bytes(1, **CONFIG2)
    members = list(range(10))
    parts = batch_second_order.split_group(members, W, N, A, G, d, 3, 1, budget=fixed + 4*per_pulse)
    assert [i for part in parts for i in part] == members
    assert all(2 <= len(part) <= 4 for part in parts) and len(parts) == 3
    assert all(ws_bytes(len(part), **CONFIG2) <= fixed + 4*per_pulse for part in parts)
    assert batch_second_order.split_group(members, W, N, A, G, d, 3, 1) == [members]
    assert batch.PASS_BYTES >= ws_bytes(16, **CONFIG2)


def test_argument_errors_need_no_gpu():
    lib = _lib.load()
    z = np.zeros(4096)
    p = z.ctypes.data
    idx = np.array([0, 0], dtype=np.int32)

    def call(P=2, W=5, N=4, A=2, G=3, d=2, s_ndim=1, n_idx=1, index=idx):
        return lib.ffk_batch_frequency_shifts(P, p, p, p, p, W, p, N, p, A, p, p, p, G, d, p, s_ndim, index.ctypes.data,
                                              n_idx, p)
    for bad in [dict(P=0), dict(P=65536), dict(d=1), dict(d=17), dict(W=0), dict(G=0), dict(s_ndim=0), dict(s_ndim=4),
                dict(n_idx=0), dict(n_idx=3), dict(n_idx=2), dict(d=9, N=81),
                dict(index=np.array([2], dtype=np.int32))]:
        assert call(**bad) == _lib.FFK_EINVAL, bad
        assert lib.ffk_last_error()
    with pytest.raises(ValueError):
        ff.frequency_shifts([Stub2(['a']), Stub2(['a', 'b'])], z[:5], z[:5])
    out = ff.frequency_shifts([], z[:5], z[:5])
    assert out.shape == (0,) and out.dtype == np.float64
    for f in (ff.cumulant_functions, ff.error_transfer_matrices):
        assert f([], z[:5], z[:5], second_order=True).shape == (0,)


class Stub2:
    """What the output-shape check reads of a pulse."""

    def __init__(self, identifiers):
        self.n_oper_identifiers = np.array(identifiers)
        self.basis = np.zeros((4, 2, 2))

"""CPU-only: the workspace and chunk queries of the batched gradient pass (ffk_batch_filter_function_derivative), and the
routing, grouping and pass splitting of ff.infidelity_derivatives / ff.filter_function_derivatives on stub pulses."""
import numpy as np
import pytest

import filter_functions_amd as ff
from filter_functions_amd import _lib, batch, batch_gradient

CONFIG2 = dict(W=4096, A=3, H=3, G=256, d=4)


def ws_bytes(P, want_dF, W, A, H, G, d):
    return _lib.load().ffk_batch_filter_function_derivative_workspace_bytes(P, W, A, H, G, d, want_dF)


class Stub:
    """What routing and grouping read of a pulse: the dimension of its control operators and its segments."""

    def __init__(self, d, G):
        self.c_opers = np.zeros((2, d, d))
        self.dt = np.ones(G)


def test_exported():
    for name in ('infidelity_derivatives', 'filter_function_derivatives'):
        assert name in ff.__all__ and getattr(ff, name) is getattr(batch_gradient, name)
        assert name in batch_gradient.__all__
    for name in ('ffk_batch_filter_function_derivative', 'ffk_batch_filter_function_derivative_chunk',
                 'ffk_batch_filter_function_derivative_workspace_bytes'):
        assert name in _lib.SIGNATURES


@pytest.mark.parametrize('want_dF', [0, 1])
@pytest.mark.parametrize('shape', [CONFIG2, dict(W=500, A=2, H=2, G=100, d=2), dict(W=70, A=3, H=2, G=17, d=3),
                                   dict(W=1, A=1, H=1, G=1, d=2), dict(W=4097, A=4, H=8, G=1000, d=4)])
def test_workspace_query_is_linear_in_the_pulses(shape, want_dF):
    sizes = {P: ws_bytes(P, want_dF, **shape) for P in (1, 2, 4, 8, 9, 64, 65535)}
    assert all(v > 0 for v in sizes.values())
    step = sizes[2] - sizes[1]
    assert step > 0
    for P, v in sizes.items():
        assert v == sizes[1] + (P - 1)*step, P


def test_a_pulse_of_config_2_takes_an_eighth_of_the_running_sums_at_most():
    W, A, H, G, d = (CONFIG2[k] for k in 'WAHGd')
    ycum = 16*G*A*d*d*W                                    # what the single path holds per pulse
    assert ws_bytes(8, 0, **CONFIG2) - ws_bytes(4, 0, **CONFIG2) <= 4*ycum//8
    assert ws_bytes(8, 1, **CONFIG2) - ws_bytes(4, 1, **CONFIG2) <= 4*ycum//8 + 4*8*A*G*H*W
    # ... so a pass of batch.PASS_BYTES holds at least ten of them
    assert ws_bytes(10, 0, **CONFIG2) <= batch.PASS_BYTES
    assert len(batch_gradient.split_group(list(range(10)), W, A, H, G, d, False)) == 1


def test_queries_reject_what_the_entry_rejects():
    assert ws_bytes(2, 0, **CONFIG2) > 0
    for bad in [dict(P=0), dict(P=65536), dict(d=1), dict(d=5), dict(A=0), dict(A=5), dict(H=0), dict(H=9), dict(W=0),
                dict(G=0)]:
        args = dict(CONFIG2, P=2, want_dF=0)
        args.update(bad)
        assert ws_bytes(**args) == 0, bad
    chunk = _lib.load().ffk_batch_filter_function_derivative_chunk
    assert chunk(0, 4, 64) == 0 and chunk(16, 5, 64) == 0 and chunk(16, 1, 64) == 0 and chunk(16, 4, 0) == 0


@pytest.mark.parametrize('d', [2, 3, 4])
@pytest.mark.parametrize('W', [1, 70, 500, 4096])
def test_chunk_length_depends_on_the_shape_alone(d, W):
    chunk = _lib.load().ffk_batch_filter_function_derivative_chunk
    for G in (1, 2, 7, 8, 9, 17, 100, 128, 129, 256, 1000, 65535):
        L = chunk(G, d, W)
        assert 1 <= L <= G
        assert -(-G//L) <= 16 or L == 8          # at most 16 chunks once a pulse has 128 segments or more
        assert L == chunk(G, d, W)
    # short pulses share one chunk length: a pulse of 2 L + 1 segments has two full chunks and a ragged one
    L = chunk(17, d, W)
    assert chunk(2*L + 1, d, W) == L and -(-(2*L + 1)//L) == 3


def test_shapes_the_batched_route_takes():
    ok = batch_gradient.batchable_shape
    assert ok(2, 1, 1) and ok(3, 4, 8) and ok(4, 3, 3)
    assert not ok(5, 1, 1) and not ok(8, 3, 3) and not ok(1, 1, 1)
    assert not ok(4, 5, 3) and not ok(4, 3, 9)
    assert not ok(4, 0, 3) and not ok(4, 3, 0)


def test_groups_by_dimension_segments_and_selected_indices():
    pulses = [Stub(2, 10), Stub(2, 10), Stub(2, 11), Stub(3, 10), Stub(2, 10), Stub(3, 10), Stub(4, 5)]
    n = len(pulses)
    c_idx_of = [[0, 1]]*n
    n_idx_of = [[0]]*n
    groups = batch_gradient.group_members(pulses, range(n), c_idx_of, n_idx_of)
    assert groups == [[0, 1, 4], [2], [3, 5], [6]]
    # other selected control or noise indices (or their order): another group
    c_idx_of = [[0, 1], [1, 0], [0, 1], [0, 1], [0, 1], [0], [0, 1]]
    assert batch_gradient.group_members(pulses, range(n), c_idx_of, n_idx_of) == [[0, 4], [1], [2], [3], [5], [6]]
    n_idx_of = [[0], [0], [0], [0], [1], [0], [0]]
    assert batch_gradient.group_members(pulses, range(n), [[0, 1]]*n, n_idx_of) == [[0, 1], [2], [3, 5], [4], [6]]
    # only the listed members are grouped
    assert batch_gradient.group_members(pulses, [1, 4, 6], [[0, 1]]*n, [[0]]*n) == [[1, 4], [6]]
    assert batch_gradient.group_members(pulses, [], c_idx_of, n_idx_of) == []


def test_passes_stay_under_the_budget():
    W, A, H, G, d = (CONFIG2[k] for k in 'WAHGd')
    per_pulse, fixed = batch_gradient.pulse_bytes(W, A, H, G, d, False)
    assert fixed >= 0 and ws_bytes(7, 0, **CONFIG2) == fixed + 7*per_pulse
    members = list(range(64))
    passes = batch_gradient.split_group(members, W, A, H, G, d, False)
    assert [i for chunk in passes for i in chunk] == members
    sizes = [len(chunk) for chunk in passes]
    assert max(sizes) - min(sizes) <= 1 and min(sizes) >= 2
    assert all(ws_bytes(len(chunk), 0, **CONFIG2) <= batch.PASS_BYTES for chunk in passes)
    assert len(passes) == -(-64//((batch.PASS_BYTES - fixed)//per_pulse))
    # with the filter-function derivative a pulse takes 75 MB more: more passes
    assert len(batch_gradient.split_group(members, W, A, H, G, d, True)) > len(passes)
    # a tiny budget: two pulses per pass; a small shape: one pass, of 65535 pulses at most
    assert all(len(c) == 2 for c in batch_gradient.split_group(members, W, A, H, G, d, False, budget=1))
    assert len(batch_gradient.split_group(members, 70, 1, 1, 4, 2, False)) == 1
    assert batch_gradient.MAX_PULSES == 65535
    big = batch_gradient.split_group(list(range(70000)), 2, 1, 1, 1, 2, False)
    assert len(big) == 2 and max(len(c) for c in big) <= 65535


def test_empty_list():
    for out in (ff.infidelity_derivatives([], np.ones(3), np.arange(3.0)),
                ff.filter_function_derivatives([], np.arange(3.0))):
        assert out.shape == (0,) and out.dtype == np.float64

"""CPU-only: the grouping and pass splitting of ff.decay_amplitudes / cumulant_functions / error_transfer_matrices
on stub pulses, and the bytes counted per pass against the library's workspace query."""
import numpy as np
import pytest

import filter_functions_amd as ff
from filter_functions_amd import _lib, batch, processes


class Stub:
    """What the grouping reads of a pulse: its basis and its noise operators."""

    def __init__(self, basis, n_nops):
        self.basis = basis
        self.n_opers = np.zeros((n_nops,) + np.shape(basis)[1:])


@pytest.fixture(scope='module')
def bases():
    return dict(p1=ff.Basis.pauli(1), g2=ff.Basis.ggm(2), p2=ff.Basis.pauli(2), g3=ff.Basis.ggm(3))


def test_groups_by_shape_basis_and_indices(bases):
    p1_again = ff.Basis.pauli(1)
    pulses = [Stub(bases['p1'], 1), Stub(bases['p2'], 3), Stub(p1_again, 1), Stub(bases['g2'], 1),
              Stub(bases['p1'], 2), Stub(bases['p2'], 3), Stub(bases['p1'], 1), Stub(bases['g3'], 1)]
    idx_of = [[0], [0, 1, 2], [0], [0], [0], [0, 1, 2], [0], [0]]
    groups = processes.group_members(pulses, range(len(pulses)), idx_of)
    # equal shape and equal basis content share a group (an equal copy of the basis too), in input order; another
    # basis of the same shape, another number of noise operators or another dimension does not
    assert sorted(groups) == [[0, 2, 6], [1, 5], [3], [4], [7]]
    # other selected indices: another group
    idx_of[5] = [0, 2, 1]
    assert sorted(processes.group_members(pulses, range(len(pulses)), idx_of)) == [[0, 2, 6], [1], [3], [4], [5], [7]]
    # only the listed members are grouped
    assert processes.group_members(pulses, [2, 6, 7], idx_of) == [[2, 6], [7]]
    assert processes.group_members(pulses, [], idx_of) == []


def test_shapes_the_batched_route_takes():
    assert processes.batchable_shape(16, 3, 4) and processes.batchable_shape(4, 1, 2)
    assert processes.batchable_shape(9, 4, 3)
    assert not processes.batchable_shape(64, 3, 8)       # more than one tile
    assert not processes.batchable_shape(16, 3, 8)       # a truncated basis of a larger dimension
    assert not processes.batchable_shape(16, 5, 4)       # more than four noise operators
    assert processes.pairs_of(3, 1) == 3 and processes.pairs_of(3, 2) == 3 and processes.pairs_of(3, 3) == 9


@pytest.mark.parametrize('W', [1, 31, 32, 255, 256, 257, 301, 4096, 4097, 16384, 16385, 100000])
def test_frequency_chunks_depend_on_the_grid_alone(W):
    chunks = processes.decay_chunks(W)
    assert 1 <= chunks <= 64
    length = -(-W//chunks)
    assert length <= 256 + 32 or chunks >= 63       # about 256 frequencies each until 64 chunks are reached
    # partials of `chunks` planes: the workspace query grows by exactly the planes' bytes from one member to two
    lib = _lib.load()
    one = lib.ffk_resident_batch_processes_workspace_bytes(64, 0, 3, 16, W, 4, 3, 2)
    two = lib.ffk_resident_batch_processes_workspace_bytes(128, 0, 3, 16, W, 4, 3, 2)
    planes = chunks if chunks > 1 else 0
    cumulant = 3*(2*16*16*16 + 2*16*256)
    assert two - one == 64*(8 + 4 + 8*256*(3*(2 + planes) + 1) + cumulant)


@pytest.mark.parametrize('A,N,W,d,n_idx,s_ndim', [(3, 16, 4096, 4, 3, 1), (3, 16, 4096, 4, 3, 2), (3, 16, 4096, 4, 2, 3),
                                                   (1, 4, 301, 2, 1, 1), (4, 9, 77, 3, 4, 3), (2, 4, 1, 2, 2, 2),
                                                   (4, 16, 16384, 4, 4, 3), (3, 16, 96, 4, 3, 2)])
def test_bytes_counted_per_pass_cover_the_workspace_query(A, N, W, d, n_idx, s_ndim):
    lib = _lib.load()
    fixed = processes.fixed_bytes(A, N, W, d, n_idx, s_ndim)
    for P in (1, 2, 7, 64, 1050):
        for host in (False, True):
            if P*processes.pairs_of(n_idx, s_ndim) > 65535:
                continue
            need = lib.ffk_resident_batch_processes_workspace_bytes(P, P if host else 0, A, N, W, d, n_idx, s_ndim)
            assert need > 0
            counted = fixed + P*processes.member_bytes(A, N, W, d, n_idx, s_ndim, host)
            assert need <= counted, (P, host)
            # ... and not by much: at most the fixed share and one alignment granule per array more
            assert counted - need <= fixed + 16*256, (P, host)


@pytest.mark.parametrize('args,nbytes', [((1, 0, 1, 4, 1, 2, 1, 1), 5376), ((3, 1, 2, 4, 8, 2, 2, 3), 20992),
                                         ((64, 0, 3, 16, 4096, 4, 3, 1), 10534656),
                                         ((5, 5, 4, 9, 300, 3, 4, 2), 1090560),
                                         ((7, 0, 1, 16, 257, 4, 1, 3), 213248)])
def test_workspace_query_values(args, nbytes):
    """The layout of the pass is part of what callers size their passes by: recorded values."""
    assert _lib.load().ffk_resident_batch_processes_workspace_bytes(*args) == nbytes


def test_workspace_query_rejects_what_the_entry_rejects():
    q = _lib.load().ffk_resident_batch_processes_workspace_bytes
    assert q(64, 0, 3, 16, 4096, 4, 3, 1) > 0
    for bad in [(0, 0, 3, 16, 4096, 4, 3, 1), (65536, 0, 3, 16, 4096, 4, 3, 1), (64, 65, 3, 16, 4096, 4, 3, 1),
                (64, 0, 3, 17, 4096, 5, 3, 1), (64, 0, 3, 16, 0, 4, 3, 1), (64, 0, 3, 16, 4096, 3, 3, 1),
                (64, 0, 3, 16, 4096, 4, 4, 1), (64, 0, 3, 16, 4096, 4, 3, 4), (64, 0, 3, 16, 4096, 4, 0, 1),
                (64, -1, 3, 16, 4096, 4, 3, 1), (64, 0, 3, 16, 4096, 17, 3, 1)]:
        assert q(*bad) == 0, bad


def test_split_into_passes():
    members = list(range(1000))
    kw = dict(A=3, N=16, W=4096, d=4, n_idx=3, s_ndim=2, single_qubit=False)
    # resident members are small: one pass
    assert processes.split_group(members, [False]*1000, **kw) == [members]
    # host arrays carry their table rows (3.1 MB each): a gibibyte holds 341 of them at most
    passes = processes.split_group(members, [True]*1000, **kw)
    assert [i for chunk in passes for i in chunk] == members
    per = processes.member_bytes(3, 16, 4096, 4, 3, 2, True)
    fixed = processes.fixed_bytes(3, 16, 4096, 4, 3, 2)
    assert all(fixed + len(chunk)*per <= batch.PASS_BYTES for chunk in passes)
    assert len(passes) == -(-1000//((batch.PASS_BYTES - fixed)//per))
    sizes = [len(chunk) for chunk in passes]
    assert max(sizes) - min(sizes) <= 1
    # one host array in the group: every member is counted with a row (an upper bound)
    assert processes.split_group(members, [True] + [False]*999, **kw) == passes
    # at most 65535 members per launch; cross-spectra: 65535 cumulant functions per launch
    many = list(range(70000))
    tiny = dict(A=1, N=4, W=8, d=2, n_idx=1)
    assert [len(c) for c in processes.split_group(many, [False]*70000, s_ndim=1, single_qubit=True, **tiny)] == \
        [35000, 35000]
    assert processes.max_members(3, 3, False) == 65535//9 and processes.max_members(3, 3, True) == 65535
    chunks = processes.split_group(many, [False]*70000, A=3, N=9, W=8, d=3, n_idx=3, s_ndim=3, single_qubit=False)
    assert all(len(c)*9 <= 65535 for c in chunks) and sum(len(c) for c in chunks) == 70000
    # a budget smaller than one member still makes progress
    assert processes.split_group([1, 2, 3], [True]*3, budget=1, **kw) == [[1], [2, 3]]       # (batch.split_passes: two at least)
    assert processes.split_group([], [], **kw) == []


def test_public_names_and_empty_lists():
    for name in ('decay_amplitudes', 'cumulant_functions', 'error_transfer_matrices'):
        assert name in ff.__all__
        out = getattr(ff, name)([], np.ones(4), np.linspace(1, 2, 4))
        assert out.shape == (0,) and out.dtype == np.float64

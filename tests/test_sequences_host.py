"""CPU side of ff.concatenate_sequences: which sequences take the batched route, the CSR packing and the length
order, pass splitting under the byte budget, the workspace query without a GPU and the new kernels' resources."""
import numpy as np
import pytest

import filter_functions_amd as ff
from filter_functions_amd import _lib, batch, sequences
from test_kernel_resources import kernels  # noqa: F401  (the module's fixture)


def gate(noise=('X',), d=2):
    """A one-segment gate (control on X and Y) carrying the noise operators *noise*."""
    P = ff.util.paulis
    if d == 2:
        ops = {'X': P[1]/2, 'Z': P[3]/2}
        return ff.PulseSequence([[P[1]/2, [0.3], 'X'], [P[2]/2, [0.1], 'Y']],
                                [[ops[name], [1.0], name] for name in noise], [1.0])
    return ff.PulseSequence([[np.kron(P[1], P[1])/2, [0.3], 'XX']], [[np.kron(P[1], P[0])/2, [1.0], 'XI']], [1.0])


def cached(pulse, omega):
    """A control matrix (zeros) and the total propagator in the caches, without a GPU."""
    A, N = len(pulse.n_opers), len(pulse.basis)
    pulse.cache_control_matrix(omega, np.zeros((A, N, len(omega)), dtype=complex))
    pulse._data['total_propagator'] = np.eye(pulse.d, dtype=complex)
    return pulse


def plan_of(seq, calc_filter_function=None, which='fidelity', omega=None):
    from filter_functions_amd.pulse_sequence import _validated_sequence
    return sequences._plan(*_validated_sequence(seq), calc_filter_function, which, omega)


def test_eligibility():
    omega = np.linspace(0.1, 1.0, 5)
    a, b = cached(gate(), omega), cached(gate(), omega)
    plan = plan_of([a, b, a])
    assert plan is not None
    assert list(plan['index']) == [0, 1, 0] and plan['A'] == 1 and np.array_equal(plan['pulse'].omega, omega)
    assert plan_of([a]) is None                                         # length 1: a deep copy, by the loop
    assert plan_of([a, b], calc_filter_function=False) is None
    assert plan_of([a, b], which='generalized') is None
    other = cached(gate(), np.linspace(0.1, 2.0, 5))
    assert plan_of([a, other]) is None                                  # gates on different grids: the loop decides
    assert plan_of([a, b], omega=np.linspace(0.1, 3.0, 5)) is None      # gates recomputed on another grid: the loop
    missing = cached(gate(noise=('Z',)), omega)
    assert plan_of([a, missing]) is None                                # a noise operator missing at a position
    two = cached(gate(noise=('X', 'Z')), omega)
    assert plan_of([two, two])['A'] == 2
    d4 = cached(gate(d=4), omega)
    assert plan_of([d4, d4]) is None                                    # d = 4: the loop
    plain = gate()
    assert plan_of([plain, plain]) is None                              # nothing cached, nothing forced: the loop
    assert plan_of([plain, plain], omega=omega, calc_filter_function=True) is None   # the loop computes the gates
    no_total = cached(gate(), omega)
    del no_total._data['total_propagator']
    assert plan_of([a, no_total]) is None
    with pytest.raises(TypeError):
        plan_of([a, 3])


def test_grouping_by_grid_basis_and_operators():
    w1, w2 = np.linspace(0.1, 1.0, 5), np.linspace(0.1, 2.0, 5)
    a, b = cached(gate(), w1), cached(gate(), w2)
    two = cached(gate(noise=('X', 'Z')), w1)
    plans = [plan_of([a, a]), plan_of([b, b]), plan_of([two, two]), plan_of([a, a, a]), plan_of([b, b])]
    assert sequences.group_plans(plans) == [[0, 3], [1, 4], [2]]


def test_csr_packing_and_length_order():
    indices = [np.array([3, 1]), np.array([0]), np.array([2, 2, 2, 1]), np.array([1, 0])]
    offsets, index, order = sequences.pack_sequences(indices)
    assert offsets.tolist() == [0, 2, 3, 7, 9]
    assert index.tolist() == [3, 1, 0, 2, 2, 2, 1, 1, 0]
    assert order.tolist() == [2, 0, 3, 1]                               # longest first, stable among equals
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))                                 # the inverse permutation
    assert [indices[order[r]].tolist() for r in rank] == [i.tolist() for i in indices]
    for p, i in enumerate(indices):
        assert index[offsets[p]:offsets[p + 1]].tolist() == i.tolist()


def test_pass_splitting_under_the_budget():
    per = sequences.pass_bytes(1000, 1, 8192, 24)
    assert per >= 16*(4 + 1)*8192
    members = list(range(1050))
    chunks = batch.split_passes(members, per, budget=64*per)
    assert sum(chunks, []) == members
    assert all(len(c) <= 64 for c in chunks) and max(map(len, chunks)) - min(map(len, chunks)) <= 1
    assert batch.split_passes(members, sequences.pass_bytes(152, 1, 301, 24)) == [members]


def test_workspace_query_needs_no_gpu():
    lib = _lib.load()
    small = lib.ffk_concatenate_sequences_workspace_bytes(24, 1, 10, 0, 2, 1, 4, 301, 0, 0)
    more = lib.ffk_concatenate_sequences_workspace_bytes(24, 2, 20, 0, 2, 1, 4, 301, 0, 0)
    assert small > 16*4*301 and more > small
    assert more - small <= sequences.pass_bytes(10, 1, 301, 24) + 4096
    assert lib.ffk_concatenate_sequences_workspace_bytes(24, 2, 20, 0, 4, 1, 16, 301, 0, 0) == 0   # d = 4
    assert lib.ffk_concatenate_sequences_workspace_bytes(24, 2, 20, 0, 2, 5, 4, 301, 0, 0) == 0    # A = 5
    assert lib.ffk_concatenate_sequences_workspace_bytes(24, 2, 20, 0, 2, 1, 4, 301, 1, 1) > more


@pytest.mark.parametrize('args,nbytes', [((24, 1, 10, 0, 2, 1, 4, 301, 0, 0), 148992),
                                         ((24, 2, 20, 0, 2, 1, 4, 301, 0, 0), 173056),
                                         ((24, 2, 20, 3, 2, 2, 4, 301, 2, 2), 366336),
                                         ((3, 2, 5, 1, 2, 4, 4, 7, 4, 3), 14592),
                                         ((1, 1, 1, 0, 2, 1, 4, 1, 1, 1), 4096)])
def test_workspace_query_values(args, nbytes):
    """The layout of the pass is part of what callers size their passes by: recorded values."""
    assert _lib.load().ffk_concatenate_sequences_workspace_bytes(*args) == nbytes


def test_new_kernels_resources(kernels):  # noqa: F811
    found = {name: k for name, k in kernels.items() if 'sequences_' in name and 'kernel' in name}
    assert sum('sequences_front_kernel' in n for n in found) == 1
    assert sum('sequences_rule_kernel' in n for n in found) == 8          # A = 1..4, staged and not
    for name, k in found.items():
        assert k['.private_segment_fixed_size'] == 0, name
        assert k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, name
        # explicit __launch_bounds__: 256 (front, unstaged rule), 512 / 1024 (staged rule)
        assert k['.max_flat_workgroup_size'] in (256, 512, 1024), name
        if k['.max_flat_workgroup_size'] == 1024:
            assert k['.vgpr_count'] <= 128, name

"""Host logic of the batched entry points (no GPU): grouping, order restoration, the split of a group into
passes under the byte budget, argument checks that need no device."""
import numpy as np
import pytest

import filter_functions_amd as ff
from filter_functions_amd import batch


def pulse(d=2, G=3, A=1, seed=0, basis=None):
    rng = np.random.default_rng(seed)
    X = ff.util.paulis[1] if d == 2 else np.diag(np.arange(d) - (d - 1)/2)
    Z = ff.util.paulis[3] if d == 2 else np.diag(np.arange(d)[::-1] - (d - 1)/2)
    return ff.PulseSequence([[X, rng.standard_normal(G)]], [[Z, np.ones(G)]]*A if A == 1 else
                            [[Z, np.ones(G), f'B{a}'] for a in range(A)], np.ones(G), basis)


def test_groups_by_shape_and_basis_in_input_order():
    pulses = [pulse(G=3), pulse(G=4), pulse(G=3, seed=1), pulse(d=3, G=3), pulse(G=4, seed=2),
              pulse(G=3, seed=3, basis=ff.Basis(np.asarray(ff.Basis.pauli(1))[[0, 2, 1, 3]])), pulse(G=3, seed=4), pulse(d=3, G=5)]
    idx = [np.arange(len(p.n_opers)) for p in pulses]
    groups = batch.group_pulses(pulses, range(len(pulses)), idx)
    assert sorted(groups) == [[0, 2, 6], [1, 4]]         # d = 3 pulses differ in G; pulse 5's basis differs
    assert all(g == sorted(g) for g in groups)
    # only the eligible ones, and groups of one are left to the single route
    assert batch.group_pulses(pulses, [0, 1, 2], idx) == [[0, 2]]
    # the selected noise operators are part of the key
    idx[2] = np.array([0, 0])
    assert [0, 2] not in batch.group_pulses(pulses, [0, 2], idx)


def test_split_under_the_byte_budget():
    members = list(range(10))
    assert batch.split_passes(members, 1) == [members]
    parts = batch.split_passes(members, 300, budget=1000)
    assert [i for p in parts for i in p] == members
    assert all(2 <= len(p) <= 3 for p in parts) and len(parts) == 4
    parts = batch.split_passes(members, 10**12, budget=1000)       # never fewer than two pulses a pass
    assert [len(p) for p in parts] == [2]*5
    assert [len(p) for p in batch.split_passes(members, 1, max_pulses=4)] == [3, 3, 4]
    assert batch.split_passes([], 1) == []
    # the estimate grows with every axis
    base = batch.pass_bytes(256, 4, 3, 16, 4096, 3)
    for k in range(6):
        args = [256, 4, 3, 16, 4096, 3]
        args[k] *= 2
        assert batch.pass_bytes(*args) > base


def test_arguments_checked_before_the_device():
    omega = np.linspace(0.1, 10, 50)
    assert ff.get_filter_functions([], omega).shape == (0,)
    assert ff.get_filter_functions([], omega).dtype == np.complex128
    assert ff.infidelities([], 1/omega, omega).shape == (0,)
    assert ff.infidelities([], 1/omega, omega).dtype == np.float64
    with pytest.raises(ValueError):          # unknown identifier, as ff.infidelity
        ff.infidelities([pulse(), pulse(seed=1)], 1/omega, omega, n_oper_identifiers=['nope'])
    with pytest.raises(ValueError):          # different numbers of selected noise operators
        ff.infidelities([pulse(A=1), pulse(A=2)], 1/omega, omega)
    with pytest.raises(ValueError):
        ff.get_filter_functions([pulse(A=1), pulse(A=2)], omega)
    with pytest.raises(ValueError):
        ff.infidelities([pulse()], 1/omega, omega, which='nonsense')
    assert 'get_filter_functions' in ff.__all__ and 'infidelities' in ff.__all__
    assert ff.get_filter_functions.__doc__ and ff.infidelities.__doc__

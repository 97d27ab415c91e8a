"""CPU side of ff.sequence_infidelities: which gate sets take the batched route, how index arrays are read, the
workspace query without a GPU, the ABI in header, exports and binding, and the new kernels' resources."""
import ctypes
import importlib

import numpy as np
import pytest

import filter_functions_amd as ff
from filter_functions_amd import _lib
from test_kernel_resources import kernels  # noqa: F401  (the module's fixture)
from test_sequences_host import cached, gate

si = importlib.import_module('filter_functions_amd.sequence_infidelities')      # (ff.<name> is the function)


def two_qubit(noise=('XI',), basis=None):
    P = ff.util.paulis
    ops = {'XI': np.kron(P[1], P[0])/2, 'IX': np.kron(P[0], P[1])/2, 'ZI': np.kron(P[3], P[0])/2,
           'IZ': np.kron(P[0], P[3])/2, 'ZZ': np.kron(P[3], P[3])/2}
    return ff.PulseSequence([[np.kron(P[1], P[1])/2, [0.3], 'XX']], [[ops[n], [1.0], n] for n in noise], [1.0],
                            basis=basis)


def test_eligibility_of_gate_sets():
    omega = np.linspace(0.1, 1.0, 5)
    a, b = cached(gate(), omega), cached(gate(), omega)
    plan = si.eligibility([a, b])
    assert plan['d'] == 2 and plan['N'] == 4 and plan['A'] == 1 and plan['basis'] is a.basis
    assert si.eligibility([]) is None
    pauli2 = ff.Basis.pauli(2)
    q = [two_qubit(basis=pauli2), two_qubit(basis=pauli2)]
    plan = si.eligibility(q)
    assert plan['d'] == 4 and plan['N'] == 16 and plan['A'] == 1
    assert si.eligibility([two_qubit(), two_qubit()])['N'] == 16                 # the default basis, equal arrays
    assert si.eligibility([two_qubit(basis=pauli2), two_qubit()]) is None        # two bases
    assert si.eligibility([a, q[0]]) is None                                     # two dimensions
    three = ff.PulseSequence([[np.diag([1.0, 0.0, -1.0]), [0.3], 'Z']], [[np.diag([1.0, -1.0, 0.0]), [1.0], 'N']],
                             [1.0])
    assert si.eligibility([three, three]) is None                                # d = 3
    assert si.eligibility([a, cached(gate(noise=('Z',)), omega)]) is None        # another operator
    assert si.eligibility([cached(gate(noise=('X', 'Z')), omega), a]) is None    # one operator more
    assert si.eligibility([gate(noise=('X', 'Z')), gate(noise=('X', 'Z'))])['A'] == 2
    four = ('IX', 'IZ', 'XI', 'ZI')
    assert si.eligibility([two_qubit(four), two_qubit(four)])['A'] == 4
    five = ('IX', 'IZ', 'XI', 'ZI', 'ZZ')
    assert si.eligibility([two_qubit(five), two_qubit(five)]) is None            # A = 5
    # equal identifiers, another operator array behind them
    P = ff.util.paulis
    other = ff.PulseSequence([[P[1]/2, [0.3], 'X'], [P[2]/2, [0.1], 'Y']], [[P[3]/2, [1.0], 'X']], [1.0])
    assert si.eligibility([a, other]) is None
    # a basis that is not traceless
    full = ff.Basis([np.eye(2), P[1], P[2], P[3]])
    if not full.istraceless:
        g = ff.PulseSequence([[P[1]/2, [0.3], 'X']], [[P[1]/2, [1.0], 'X']], [1.0], basis=full)
        assert si.eligibility([g, g]) is None


def test_index_arrays():
    got = si.index_arrays([[0, 2, -1], np.array([3], dtype=np.uint8), (1, 1)], 4)
    assert [g.tolist() for g in got] == [[0, 2, 3], [3], [1, 1]]
    assert all(g.dtype == np.int32 for g in got)
    for bad in ([4], [-5], [0, 7]):
        with pytest.raises(IndexError):
            si.index_arrays([bad], 4)
    with pytest.raises(ValueError):
        si.index_arrays([[0], []], 4)
    with pytest.raises(ValueError):
        si.index_arrays([[[0, 1]]], 4)
    for bad in ([0.0, 1.0], [True, False], ['a']):
        with pytest.raises(TypeError):
            si.index_arrays([bad], 4)
    omega = np.linspace(0.1, 1.0, 5)
    a = cached(gate(), omega)
    with pytest.raises(TypeError):
        ff.sequence_infidelities([a, 3], [[0]], 1/omega, omega)
    with pytest.raises(ValueError):
        ff.sequence_infidelities([a], [], 1/omega, omega)
    with pytest.raises(IndexError):
        ff.sequence_infidelities([a], [[1]], 1/omega, omega)


def test_pass_bytes_cover_the_workspace():
    query = _lib.load().ffk_sequence_infidelities_workspace_bytes
    for d, A, W, T, P, G, n_idx, s_ndim in ((2, 1, 301, 24, 1050, 152, 1, 1), (4, 2, 301, 27, 1050, 152, 2, 3),
                                            (4, 4, 70, 40, 7, 1000, 4, 3)):
        n_out = n_idx*n_idx if s_ndim == 3 else n_idx
        bound = P*si.pass_bytes(G, d, A, W, n_out) + si.table_bytes(T, d, A, W)
        assert query(T, P, P*G, T, d, A, d*d, W, n_idx, s_ndim) <= bound


def test_workspace_query_needs_no_gpu():
    query = _lib.load().ffk_sequence_infidelities_workspace_bytes
    base = query(24, 2, 20, 0, 2, 1, 4, 301, 1, 1)
    assert base > 2*16*301
    assert query(24, 200, 218, 0, 2, 1, 4, 301, 1, 1) > query(24, 2, 218, 0, 2, 1, 4, 301, 1, 1)      # grows with P
    assert query(24, 2, 20, 3, 2, 1, 4, 301, 1, 1) >= base + 3*16*4*301                              # host rows
    d4 = query(24, 2, 20, 0, 4, 1, 16, 301, 1, 1)
    assert d4 > base                                                                                 # d = 4
    assert query(24, 200, 218, 0, 4, 1, 16, 301, 1, 1) > query(24, 2, 218, 0, 4, 1, 16, 301, 1, 1)
    assert query(24, 2, 20, 3, 4, 2, 16, 301, 1, 1) >= query(24, 2, 20, 0, 4, 2, 16, 301, 1, 1) + 3*16*2*16*301
    assert query(24, 2, 20, 0, 4, 4, 16, 301, 4, 3) > d4
    assert query(24, 2, 20, 0, 3, 1, 9, 301, 1, 1) == 0       # d = 3
    assert query(24, 2, 20, 0, 4, 5, 16, 301, 1, 1) == 0      # A = 5
    assert query(24, 2, 20, 0, 2, 5, 4, 301, 1, 1) == 0
    assert query(24, 2, 20, 0, 4, 1, 4, 301, 1, 1) == 0       # N != d^2
    assert query(24, 2, 20, 0, 2, 1, 16, 301, 1, 1) == 0
    assert query(24, 2, 20, 0, 4, 1, 16, 301, 2, 1) == 0      # more selected operators than there are
    assert query(24, 2, 1, 0, 4, 1, 16, 301, 1, 1) == 0       # fewer positions than sequences
    assert query(24, 2, 20, 0, 4, 1, 16, 301, 0, 0) > 0       # no spectrum: the other outputs


def test_the_existing_queries_return_what_they_returned():
    lib = _lib.load()
    assert lib.ffk_concatenate_sequences_workspace_bytes(24, 2, 20, 3, 2, 2, 4, 301, 2, 2) == 366336
    assert lib.ffk_concatenate_sequences_workspace_bytes(3, 2, 5, 1, 2, 4, 4, 7, 4, 3) == 14592
    assert lib.ffk_concatenate_sequences_workspace_bytes(24, 2, 20, 0, 4, 1, 16, 301, 0, 0) == 0
    corr = lib.ffk_sequence_correlation_infidelities_workspace_bytes
    assert corr(24, 2, 20, 0, 4, 1, 16, 301, 1, 1) == 0
    assert corr(24, 2, 20, 0, 2, 1, 4, 301, 1, 1) == 201728
    assert lib.ffk_resident_batch_processes_workspace_bytes(8, 2, 2, 16, 301, 4, 2, 1) == 745984


def test_binding_header_and_exports_agree():
    """test_abi's agreement, with the new entries in all three places."""
    import test_abi
    names = test_abi.header_symbols()
    for name in ('ffk_sequence_infidelities', 'ffk_sequence_infidelities_workspace_bytes'):
        assert name in names and name in _lib.SIGNATURES
    test_abi.test_library_exports_every_declared_symbol()
    test_abi.test_binding_table_matches_header()


def test_bad_arguments_are_refused_before_the_device():
    lib = _lib.load()
    res, args = _lib.SIGNATURES['ffk_sequence_infidelities']
    assert lib.ffk_sequence_infidelities(*[None if a is ctypes.c_void_p else 0 for a in args]) == _lib.FFK_EINVAL
    assert 'NULL' in lib.ffk_last_error().decode()


def _check(name, k):
    assert k['.private_segment_fixed_size'] == 0, name
    assert k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, name
    assert k['.max_flat_workgroup_size'] == 256, name
    # 256 threads are four wavefronts, one per SIMD: the whole file of 512 registers (accumulation registers included)
    assert k['.vgpr_count'] >= k.get('.agpr_count', 0)
    assert k['.vgpr_count'] <= 512, (name, k['.vgpr_count'], k.get('.agpr_count'))


def test_new_kernels_resources(kernels):  # noqa: F811
    front = {name: k for name, k in kernels.items() if 'sequences4_front_kernel' in name}
    rule = {name: k for name, k in kernels.items() if 'sequences4_rule_kernel' in name}
    assert len(front) == 1 and len(rule) == 8, (sorted(front), sorted(rule))        # A = 1..4, staged and not
    for a in range(1, 5):
        assert sum(f'ILi{a}E' in name for name in rule) == 2, (a, sorted(rule))
    for name, k in {**front, **rule}.items():
        _check(name, k)
    for name, k in rule.items():
        assert k['.group_segment_fixed_size'] == 0, name       # (the staged tables are sized at the launch)
        assert k.get('.agpr_count', 0) >= 64, name             # the accumulator tiles of the matrix instructions

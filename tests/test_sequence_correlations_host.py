"""CPU side of ff.sequence_correlation_infidelities: how index arrays are read, which sequences take the batched
route, the completion step, the byte account of a pass against the workspace queries, the order of the results after
pass splitting, and the ABI of the new entry in header, exports and binding."""
import ctypes

import numpy as np
import pytest

import filter_functions_amd as ff
from filter_functions_amd import _lib, batch, correlations
from filter_functions_amd import sequence_correlations as sc
from test_sequence_infidelities_host import two_qubit
from test_sequences_host import cached, gate

OMEGA = np.linspace(0.1, 1.0, 5)


class Routes:
    """_run_pass and the loop's two calls replaced: which sequences went where."""

    def __init__(self, monkeypatch):
        self.passes, self.looped = [], []

        def fake_pass(gates, indices, plan, omega, S, idx):
            self.passes.append([i.tolist() for i in indices])
            return [np.full((len(i), len(i), len(idx)), 1.0) for i in indices]

        def fake_concatenate(pulses, calc_pulse_correlation_FF=False, omega=None, **kwargs):
            assert calc_pulse_correlation_FF is True
            self.looped.append(len(pulses))
            return list(pulses)

        def fake_infidelity(pulse, spectrum, omega, n_oper_identifiers=None, which='total'):
            assert which == 'correlations'
            return np.full((len(pulse), len(pulse), 1), -1.0)
        monkeypatch.setattr(sc, '_run_pass', fake_pass)
        monkeypatch.setattr(ff, 'concatenate', fake_concatenate)
        monkeypatch.setattr(ff, 'infidelity', fake_infidelity)


def single_qubit_set(noise=('X',)):
    return [cached(gate(noise=noise), OMEGA) for _ in range(3)]


def two_qubit_set(noise=('XI',)):
    return [cached(two_qubit(noise), OMEGA) for _ in range(3)]


def test_index_rules_and_their_exceptions(monkeypatch):
    routes = Routes(monkeypatch)
    for gates in (single_qubit_set(), two_qubit_set()):
        S = 1/OMEGA
        got = ff.sequence_correlation_infidelities(gates, [[0, 2, -1], np.array([-3, 1], dtype=np.int8)], S, OMEGA)
        assert routes.passes.pop() == [[0, 2, 2], [0, 1]]                      # negative indices wrap
        assert [g.shape for g in got] == [(3, 3, 1), (2, 2, 1)]
        for bad in ([[0, 3]], [[-4, 0]]):
            with pytest.raises(IndexError):
                ff.sequence_correlation_infidelities(gates, bad, S, OMEGA)
        for bad in ([[0, 1], []], [], [[[0, 1]]]):
            with pytest.raises(ValueError):
                ff.sequence_correlation_infidelities(gates, bad, S, OMEGA)
        for bad in ([[0.0, 1.0]], [[True, False]]):
            with pytest.raises(TypeError):
                ff.sequence_correlation_infidelities(gates, bad, S, OMEGA)
        with pytest.raises(TypeError):
            ff.sequence_correlation_infidelities(gates + [3], [[0, 1]], S, OMEGA)
    assert routes.passes == [] and routes.looped == []


def test_the_loops_exceptions_for_a_bad_spectrum_and_bad_identifiers(monkeypatch):
    Routes(monkeypatch)
    gates = two_qubit_set()
    with pytest.raises(ValueError) as error:
        ff.sequence_correlation_infidelities(gates, [[0, 1]], np.ones(4), OMEGA)
    with pytest.raises(ValueError) as expected:
        ff.util.parse_spectrum(np.ones(4), OMEGA, np.array([0]))
    assert str(error.value) == str(expected.value)
    with pytest.raises(ValueError) as error:
        ff.sequence_correlation_infidelities(gates, [[0, 1]], 1/OMEGA, OMEGA, n_oper_identifiers=['Q'])
    with pytest.raises(ValueError) as expected:
        ff.util.get_indices_from_identifiers(gates[0].n_oper_identifiers, ['Q'])
    assert str(error.value) == str(expected.value)


@pytest.mark.parametrize('make', [single_qubit_set, two_qubit_set])
def test_routing_is_per_sequence(monkeypatch, make):
    routes = Routes(monkeypatch)
    gates = make()
    S = 1/OMEGA
    seqs = [[0, 1], [2], [0, 1]*128, [0, 1]*128 + [2], [1, 2, 0]]
    got = ff.sequence_correlation_infidelities(gates, seqs, S, OMEGA)
    assert [len(i) for i in routes.passes.pop()] == [2, 256, 3]                # one pass, input order
    assert routes.looped == [1, 257]                                           # one gate and 257 gates: the loop
    assert [g.shape[0] for g in got] == [2, 1, 256, 257, 3]
    assert [g[0, 0, 0] for g in got] == [1.0, -1.0, 1.0, -1.0, 1.0]
    del routes.looped[:]
    # a complex spectrum without an imaginary part stays; with one, and cross-spectra, follow the loop
    ff.sequence_correlation_infidelities(gates, seqs[:1], S*(1 + 0j), OMEGA)
    assert len(routes.passes) == 1 and routes.looped == []
    ff.sequence_correlation_infidelities(gates, seqs[:1], S*(1 + 1j), OMEGA)
    ff.sequence_correlation_infidelities(gates, seqs[:1], np.ones((1, 1, 5)), OMEGA)
    assert len(routes.passes) == 1 and routes.looped == [2, 2]


def test_spectra_of_two_dimensions_and_selected_operators(monkeypatch):
    seen = []

    def fake_pass(gates, indices, plan, omega, S, idx):
        seen.append((plan['d'], plan['A'], S.shape, S.dtype, idx.tolist(), idx.dtype))
        return [np.zeros((len(i), len(i), len(idx))) for i in indices]
    monkeypatch.setattr(sc, '_run_pass', fake_pass)
    gates = two_qubit_set(('IX', 'XI', 'ZZ'))
    ff.sequence_correlation_infidelities(gates, [[0, 1]], np.ones((2, 5), dtype=int), OMEGA,
                                         n_oper_identifiers=['ZZ', 'IX'])
    assert seen == [(4, 3, (2, 5), np.float64, [2, 0], np.int32)]


def test_ineligible_sets_run_the_loop(monkeypatch):
    routes = Routes(monkeypatch)
    P = ff.util.paulis
    three = [cached(ff.PulseSequence([[np.diag([1.0, 0.0, -1.0]), [0.3 + 0.1*k], 'Z']],
                                     [[np.diag([1.0, -1.0, 0.0]), [1.0], 'N']], [1.0]), OMEGA) for k in range(2)]
    full = ff.Basis([np.diag([1.0, 0.0]), np.diag([0.0, 1.0]), P[1]/np.sqrt(2), P[2]/np.sqrt(2)])
    assert not full.istraceless
    with_trace = [cached(ff.PulseSequence([[P[1]/2, [0.3], 'X']], [[P[1]/2, [1.0], 'X']], [1.0], basis=full), OMEGA)
                  for _ in range(2)]
    differing = [cached(gate(), OMEGA),
                 cached(ff.PulseSequence([[P[1]/2, [0.3], 'X'], [P[2]/2, [0.1], 'Y']], [[P[3]/2, [1.0], 'X']], [1.0]),
                        OMEGA)]
    mixed = [cached(gate(), OMEGA), cached(two_qubit(), OMEGA)]
    for gates in (three, with_trace, differing, mixed):
        assert sc.eligibility(gates) is None
        got = ff.sequence_correlation_infidelities(gates, [[0, 1], [1, 1, 0]], 1/OMEGA, OMEGA)
        assert routes.passes == [] and routes.looped == [2, 3]
        assert [g[0, 0, 0] for g in got] == [-1.0, -1.0]
        del routes.looped[:]
    # an eligible set of which a gate does not know its total propagator
    gates = two_qubit_set()
    del gates[1]._data['total_propagator']
    ff.sequence_correlation_infidelities(gates, [[0, 1]], 1/OMEGA, OMEGA)
    assert routes.passes == [] and routes.looped == [2]


def test_the_completion_step_is_one_call(monkeypatch):
    routes = Routes(monkeypatch)
    calls = []

    def fake_completion(pulses, omega):
        calls.append(list(pulses))
        for p in pulses:
            cached(p, omega)
    monkeypatch.setattr(batch, 'get_filter_functions', fake_completion)
    gates = two_qubit_set() + [two_qubit(), two_qubit()]
    other = cached(two_qubit(), np.linspace(0.1, 2.0, 5))                 # cached on another grid
    gates.append(other)
    ff.sequence_correlation_infidelities(gates, [[0, 3], [5, 4, 1]], 1/OMEGA, OMEGA)
    assert len(calls) == 1 and [id(g) for g in calls[0]] == [id(g) for g in gates[3:]]
    assert routes.passes == [[[0, 3], [5, 4, 1]]] and routes.looped == []
    ff.sequence_correlation_infidelities(gates, [[0, 3]], 1/OMEGA, OMEGA)
    assert len(calls) == 1                                                # nothing is missing any more


def test_w_below_two_gives_zeros():
    one = np.array([0.7])
    gates = [cached(two_qubit(), one) for _ in range(2)]
    got = ff.sequence_correlation_infidelities(gates, [[0, 1, 0]], [1.0], one)
    assert got[0].shape == (3, 3, 1) and not got[0].any()


def test_pass_and_table_bytes_bound_the_workspace_queries():
    lib = _lib.load()
    queries = {2: lib.ffk_sequence_correlation_infidelities_workspace_bytes,
               4: lib.ffk_sequence_correlation_infidelities4_workspace_bytes}
    checked = 0
    for d, query in queries.items():
        for A in (1, 2, 3, 4):
            for W in (2, 7, 301):
                for G in (1, 2, 17, 152, 256):
                    for P, T in ((1, 1), (3, 24), (1050, 27)):
                        for n_idx in {1, A}:
                            for s_ndim in (1, 2):
                                asked = query(T, P, P*G, T, d, A, d*d, W, n_idx, s_ndim)
                                bound = P*sc.pass_bytes(G, d, A, W, n_idx) + sc.table_bytes(T, d, A, W)
                                assert 0 < asked <= bound, (d, A, W, G, P, T, n_idx, s_ndim, asked, bound)
                                checked += 1
    assert checked > 1000
    # functions of the shape alone, growing with every axis
    assert sc.pass_bytes(152, 4, 1, 301, 1) > sc.pass_bytes(152, 2, 1, 301, 1) > sc.pass_bytes(151, 2, 1, 301, 1)
    assert sc.pass_bytes(152, 4, 1, 301, 1) >= 152*8*256 + 8*152*256*(1 + correlations.slabs(301))
    assert sc.table_bytes(25, 4, 2, 301) > sc.table_bytes(24, 4, 2, 301) >= 24*16*2*16*301


def test_the_new_query_needs_no_gpu_and_refuses_other_shapes():
    query = _lib.load().ffk_sequence_correlation_infidelities4_workspace_bytes
    base = query(24, 2, 20, 0, 4, 1, 16, 301, 1, 1)
    assert base > 8*20*20*(1 + correlations.slabs(301)) + 8*20*256
    assert query(24, 200, 218, 0, 4, 1, 16, 301, 1, 1) > query(24, 2, 218, 0, 4, 1, 16, 301, 1, 1)      # grows with P
    assert query(24, 2, 40, 0, 4, 1, 16, 301, 1, 1) > base                                              # ... n_index
    assert query(24, 2, 20, 3, 4, 1, 16, 301, 1, 1) >= base + 3*16*16*301                               # host rows
    assert query(24, 2, 20, 0, 3, 1, 9, 301, 1, 1) == 0       # d = 3
    assert query(24, 2, 20, 0, 2, 1, 4, 301, 1, 1) == 0       # d = 2 has its own entry
    assert query(24, 2, 20, 0, 4, 1, 4, 301, 1, 1) == 0       # N != d^2
    assert query(24, 2, 20, 0, 4, 5, 16, 301, 1, 1) == 0      # A = 5
    assert query(24, 2, 20, 0, 4, 1, 16, 301, 1, 3) == 0      # cross-spectra
    assert query(24, 2, 20, 0, 4, 1, 16, 301, 2, 1) == 0      # more selected operators than there are
    assert query(24, 2, 1, 0, 4, 1, 16, 301, 1, 1) == 0       # fewer positions than sequences
    old = _lib.load().ffk_sequence_correlation_infidelities_workspace_bytes
    assert old(24, 2, 20, 0, 3, 1, 9, 301, 1, 1) == 0 and old(24, 2, 20, 0, 2, 1, 4, 301, 1, 3) == 0
    assert old(24, 2, 20, 0, 2, 1, 4, 301, 1, 1) == 201728    # what it returned before


def test_pass_splitting_keeps_input_order(monkeypatch):
    passes = []

    def fake_pass(gates, indices, plan, omega, S, idx):
        passes.append([len(i) for i in indices])
        return [np.full((len(i), len(i), 1), float(i[0])) for i in indices]
    monkeypatch.setattr(sc, '_run_pass', fake_pass)
    gates = [cached(two_qubit(), OMEGA) for _ in range(9)]
    lengths = [2, 5, 3, 2, 4, 7, 2, 3, 6]
    seqs = [[k] + [(k + j) % 9 for j in range(1, m)] for k, m in enumerate(lengths)]
    monkeypatch.setattr(sc, 'PASS_BYTES', 3*sc.pass_bytes(7, 4, 1, 5, 1) + sc.table_bytes(9, 4, 1, 5))
    got = ff.sequence_correlation_infidelities(gates, seqs, 1/OMEGA, OMEGA)
    assert passes == [[2, 5, 3], [2, 4, 7], [2, 3, 6]]
    assert [g.shape for g in got] == [(m, m, 1) for m in lengths]
    assert [g[0, 0, 0] for g in got] == list(range(9))


def test_only_the_gates_a_pass_uses_are_in_its_table(monkeypatch):
    """The arguments of the C entry: the table of a pass holds the used gates, the indices are renumbered."""
    seen = {}

    class Lib:
        def ffk_sequence_correlation_infidelities4(self, handles, slots, table, U, tau, T, offsets, index, P, *rest):
            seen.update(T=T, P=P, n_handles=len(handles), index=np.ctypeslib.as_array(
                ctypes.cast(ctypes.c_void_p(index), ctypes.POINTER(ctypes.c_int32)), (5,)).tolist())
            return 0
    monkeypatch.setattr(_lib, 'load', lambda: Lib())
    gates = [cached(two_qubit(), OMEGA) for _ in range(6)]
    sc._run_pass(gates, [np.array([4, 1], dtype=np.int32), np.array([5, 4, 4], dtype=np.int32)],
                 sc.eligibility(gates), OMEGA, 1/OMEGA, np.array([0], dtype=np.int32))
    assert seen == dict(T=3, P=2, n_handles=3, index=[1, 0, 2, 1, 1])


def test_binding_header_and_exports_agree():
    """test_abi's agreement, with the new entries in all three places."""
    import test_abi
    names = test_abi.header_symbols()
    for name in ('ffk_sequence_correlation_infidelities4', 'ffk_sequence_correlation_infidelities4_workspace_bytes'):
        assert name in names and name in _lib.SIGNATURES
    assert _lib.SIGNATURES['ffk_sequence_correlation_infidelities4'] == \
        _lib.SIGNATURES['ffk_sequence_correlation_infidelities']
    test_abi.test_library_exports_every_declared_symbol()
    test_abi.test_binding_table_matches_header()


def test_bad_arguments_are_refused_before_the_device():
    lib = _lib.load()
    res, args = _lib.SIGNATURES['ffk_sequence_correlation_infidelities4']
    assert lib.ffk_sequence_correlation_infidelities4(*[None if a is ctypes.c_void_p else 0 for a in args]) \
        == _lib.FFK_EINVAL
    assert 'NULL' in lib.ffk_last_error().decode()

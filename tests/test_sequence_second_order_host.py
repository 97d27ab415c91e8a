"""CPU side of ff.sequence_frequency_shifts and of second_order=True on ff.sequence_cumulant_functions /
ff.sequence_error_transfer_matrices: the ABI in header, exports and binding, the workspace query without a GPU and the
Python byte counts that bound it, the new kernels' resources, which calls take the batched route, how stacked spectra
are read and what happens to a (spectrum, sequence) whose result is not finite (the passes, the gates' own shifts and
the loop replaced by stand-ins: no GPU)."""
import ctypes

import numpy as np
import pytest

import filter_functions_amd as ff
from filter_functions_amd import _lib
from filter_functions_amd import sequence_processes as sp
from filter_functions_amd import sequence_second_order as so
from test_kernel_resources import kernels  # noqa: F401  (the module's fixture)
from test_sequence_infidelities_host import two_qubit
from test_sequences_host import cached, gate


def test_public_names():
    assert 'sequence_frequency_shifts' in ff.__all__ and 'sequence_frequency_shifts' in so.__all__
    assert ff.sequence_frequency_shifts is so.sequence_frequency_shifts and ff.sequence_second_order is so
    # the index rules, the gate checks and the reading of stacked spectra are the existing ones
    from filter_functions_amd.sequence_infidelities import eligibility, index_arrays
    assert so.index_arrays is index_arrays and so.eligibility is eligibility
    assert so.stacked_spectra is sp.stacked_spectra


def test_binding_header_and_exports_agree():
    import test_abi
    names = test_abi.header_symbols()
    for name in ('ffk_sequence_frequency_shifts', 'ffk_sequence_frequency_shifts_workspace_bytes'):
        assert name in names and name in _lib.SIGNATURES
    test_abi.test_library_exports_every_declared_symbol()
    test_abi.test_binding_table_matches_header()


def test_bad_arguments_are_refused_before_the_device():
    lib = _lib.load()
    res, args = _lib.SIGNATURES['ffk_sequence_frequency_shifts']
    assert lib.ffk_sequence_frequency_shifts(*[None if a is ctypes.c_void_p else 0 for a in args]) == _lib.FFK_EINVAL
    assert 'NULL' in lib.ffk_last_error().decode()


def test_workspace_query_needs_no_gpu():
    query = _lib.load().ffk_sequence_frequency_shifts_workspace_bytes
    # (T, P, n_index, n_host, d, A, N, W, n_idx, s_ndim, n_spectra)
    base = query(24, 2, 218, 0, 4, 2, 16, 301, 1, 1, 1)
    assert base > 2*16*301
    assert query(24, 200, 218, 0, 4, 2, 16, 301, 1, 1, 1) > base                  # grows with P
    assert query(24, 2, 218, 0, 4, 2, 16, 602, 1, 1, 1) > base                    # W
    assert query(24, 2, 218, 0, 4, 2, 16, 301, 1, 1, 5) > base                    # n_spectra
    assert query(24, 2, 218, 0, 4, 2, 16, 301, 2, 1, 1) > base                    # n_idx
    assert query(24, 2, 218, 3, 4, 2, 16, 301, 1, 1, 1) >= base + 3*16*2*16*301   # host rows
    d2 = query(24, 2, 218, 0, 2, 1, 4, 301, 1, 2, 3)
    assert 0 < d2 < base
    assert query(24, 200, 218, 0, 2, 1, 4, 301, 1, 2, 3) > d2
    for bad in ((24, 2, 218, 0, 3, 1, 9, 301, 1, 1, 1),         # d = 3
                (24, 2, 218, 0, 4, 5, 16, 301, 1, 1, 1),        # A = 5
                (24, 2, 218, 0, 4, 1, 4, 301, 1, 1, 1),         # N != d^2
                (24, 2, 218, 0, 4, 1, 16, 301, 2, 1, 1),        # more selected operators than there are
                (24, 2, 1, 0, 4, 1, 16, 301, 1, 1, 1),          # fewer positions than sequences
                (24, 2, 218, 0, 4, 1, 16, 301, 1, 3, 1),        # a cross-spectrum
                (24, 2, 218, 0, 4, 1, 16, 301, 1, 1, 0),        # no spectrum
                (24, 2, 218, 0, 4, 1, 16, 1, 1, 1, 1),          # one frequency: no integral
                (24, 2, 218, 25, 4, 1, 16, 301, 1, 1, 1),       # more host rows than gates
                (0, 2, 218, 0, 4, 1, 16, 301, 1, 1, 1), (24, 0, 218, 0, 4, 1, 16, 301, 1, 1, 1)):
        assert query(*bad) == 0, bad


def test_pass_bytes_are_pinned_and_cover_the_workspace():
    assert so.block_width(2, 4) == 64 and so.block_width(4, 2) == 64 and so.block_width(4, 3) == 32
    assert so.SPECTRA_PER_WALK == 2
    # the study's shape: 24 Cliffords, 301 frequencies, one operator, three spectra ...
    assert so.pass_bytes(152, 2, 1, 301, 1, 3) == 12 + 4*152 + 64 + 8*16*3*(1 + 5)
    assert so.table_bytes(24, 2, 1, 301, 1, 3, 1) == 24*(16*4*301 + 16*301 + 128 + 64 + 16 + 8*16*3) + 256 + 8*301 \
        + 32*3*301 + 4 + 5120
    # ... and two-qubit gates with four operators, two of them selected, one spectrum row each: blocks of 32
    assert so.pass_bytes(1000, 4, 4, 70, 2, 5) == 12 + 4000 + 256 + 8*256*10*(1 + 3)
    assert so.table_bytes(40, 4, 4, 70, 2, 5, 2) == 40*(16*4*16*70 + 16*70 + 2048 + 256 + 16 + 8*256*10) + 4096 + 560 \
        + 32*10*70 + 8 + 5120
    query = _lib.load().ffk_sequence_frequency_shifts_workspace_bytes
    for d, A, W, T, P, G, n_idx, s_ndim, K in ((2, 1, 301, 24, 1050, 152, 1, 1, 3), (4, 2, 301, 27, 1050, 152, 2, 2, 3),
                                               (4, 4, 70, 40, 7, 1000, 4, 2, 5), (4, 3, 7, 3, 2, 1, 1, 1, 1),
                                               (2, 4, 65, 24, 3, 2, 4, 2, 1)):
        bound = P*so.pass_bytes(G, d, A, W, n_idx, K) + so.table_bytes(T, d, A, W, n_idx, K, s_ndim)
        assert 0 < query(T, P, P*G, T, d, A, d*d, W, n_idx, s_ndim, K) <= bound


def test_new_kernels_resources(kernels):  # noqa: F811
    d2 = {name: k for name, k in kernels.items() if 'seq2o_walk2_kernel' in name}
    d4 = {name: k for name, k in kernels.items() if 'seq2o_walk4_kernel' in name}
    assert len(d2) == 8 and len(d4) == 8, (sorted(d2), sorted(d4))                  # A = 1..4, staged and not
    assert sum('seq2o_reduce_kernel' in name for name in kernels) == 1
    for a in range(1, 5):
        assert sum(f'ILi{a}E' in name for name in d2) == 2 and sum(f'ILi{a}E' in name for name in d4) == 2
    for name, k in {**d2, **d4}.items():
        assert k['.private_segment_fixed_size'] == 0, name
        assert k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, name
        assert k['.group_segment_fixed_size'] == 0, name        # (tables and weights are sized at the launch)
        # 256 threads are four wavefronts, one per SIMD: the whole file of 512 registers, accumulators included
        assert k['.max_flat_workgroup_size'] == 256, name
        assert k['.vgpr_count'] <= 512, (name, k['.vgpr_count'], k.get('.agpr_count'))
    for name, k in d4.items():
        assert k.get('.agpr_count', 0) > 0, name
    # the kernels of the first-order passes keep their names apart from the new ones
    assert sum('sequences4_rule_kernel' in name for name in kernels) == 8
    assert sum('sequences_rule_kernel' in name for name in kernels) == 8
    assert sum('sequences4_gamma_kernel' in name for name in kernels) == 8
    assert sum('sequences_gamma_kernel' in name for name in kernels) == 8
    assert sum('sequence_processes_reduce_kernel' in name for name in kernels) == 1


# ---- stand-ins for the device, the gates' own shifts and the loop ----------------------------------------------------
@pytest.fixture
def gates():
    omega = np.linspace(0.1, 1.0, 5)
    return [cached(gate(noise=('X', 'Z')), omega) for _ in range(3)], omega


class Passes:
    """Replaces the module's pass, the gates' own shifts and the loop: records what they were asked for and returns
    recognisable values."""

    def __init__(self, monkeypatch, not_finite=()):
        self.passes, self.loops, self.own, self.not_finite = [], [], [], set(not_finite)
        monkeypatch.setattr(so, '_run_pass', self.run_pass)
        monkeypatch.setattr(so, '_loop', self.loop)
        monkeypatch.setattr(so, '_gate_shifts', self.gate_shifts)

    def gate_shifts(self, gates, spectrum, omega, n_oper_identifiers):
        self.own.append(float(np.real(np.asarray(spectrum).flat[0])))
        n_idx = len(ff.util.get_indices_from_identifiers(gates[0].n_oper_identifiers, n_oper_identifiers))
        N = len(gates[0].basis)
        return np.full((len(gates), n_idx, N, N), self.own[-1])

    def run_pass(self, gates, indices, plan, omega, S, idx, shifts, want_U):
        self.passes.append(dict(indices=[i.tolist() for i in indices], S=S.copy(), idx=list(idx),
                                shifts=np.array(shifts)))
        N, K, P = plan['N'], len(S), len(indices)
        out = np.empty((K, P, len(idx), N, N))
        bad = np.zeros((K, P), dtype=bool)
        for k in range(K):
            for j, i in enumerate(indices):
                out[k, j] = S[k].sum() + 1000*len(i) + i[0]
                bad[k, j] = (int(round(S[k].flat[0])), len(i)) in self.not_finite
        return out, bad, np.zeros((P, plan['d'], plan['d']), dtype=complex) if want_U else None

    def loop(self, gates, indices, spectra, omega, n_oper_identifiers, want_U):
        self.loops.append(dict(spectra=spectra))
        return np.full((len(spectra), len(indices), 1), -1.0), np.ones((len(indices), 2, 2)) if want_U else None


def test_stacked_shapes_and_the_gates_own_shifts(gates, monkeypatch):
    gates, omega = gates
    seqs = [[0, 1], [2], [1, 1, 0]]
    stand_in = Passes(monkeypatch)
    W = len(omega)
    one = ff.sequence_frequency_shifts(gates, seqs, np.ones(W), omega)
    assert one.shape == (3, 2, 4, 4) and stand_in.own == [1.0]
    for S in (np.ones((4, W)), np.ones((4, 2, W)), np.ones((4, 1, W))):
        got = ff.sequence_frequency_shifts(gates, seqs, S, omega, stacked=True)
        assert got.shape == (4, 3, 2, 4, 4)
        assert stand_in.passes[-1]['S'].shape == (4,) + ((W,) if S.ndim == 2 else (2, W))
        assert stand_in.passes[-1]['shifts'].shape == (4, 3, 2, 4, 4)
    got, U = ff.sequence_frequency_shifts(gates, seqs, np.ones((1, W)), omega, stacked=True, return_propagators=True)
    assert got.shape == (1, 3, 2, 4, 4) and U.shape == (3, 2, 2)
    assert np.array_equal(got[0], one)
    assert not stand_in.loops
    # the gates' own shifts: one request per spectrum, in order, whatever the number of sequences
    stand_in.own.clear()
    S = np.arange(1.0, 4.0)[:, None]*np.ones(W)
    ff.sequence_frequency_shifts(gates, seqs*5, S, omega, stacked=True)
    assert stand_in.own == [1.0, 2.0, 3.0]
    assert [float(stand_in.passes[-1]['shifts'][k].flat[0]) for k in range(3)] == [1.0, 2.0, 3.0]
    # a subset of the operators, not in sorted order: their indices reach the pass, each spectrum row stays with its
    # operator
    S = np.arange(2*2*W, dtype=float).reshape(2, 2, W)
    ff.sequence_frequency_shifts(gates, seqs, S, omega, n_oper_identifiers=['Z', 'X'], stacked=True)
    assert stand_in.passes[-1]['idx'] == [1, 0] and np.array_equal(stand_in.passes[-1]['S'], S)
    # (K, n_idx, n_idx, W): cross-spectra, the loop
    C = np.ones((3, 2, 2, W))
    assert ff.sequence_frequency_shifts(gates, seqs, C, omega, stacked=True).shape == (3, 3, 1)
    assert len(stand_in.loops) == 1 and len(stand_in.loops[0]['spectra']) == 3
    # without stacked a two-dimensional spectrum is one spectrum
    assert ff.sequence_frequency_shifts(gates, seqs, np.ones((2, W)), omega).shape == (3, 2, 4, 4)
    assert stand_in.passes[-1]['S'].shape == (1, 2, W)


def test_refusals(gates, monkeypatch):
    gates, omega = gates
    Passes(monkeypatch)
    W = len(omega)
    function = ff.sequence_frequency_shifts
    with pytest.raises(ValueError, match='at least one spectrum'):
        function(gates, [[0]], np.ones((0, W)), omega, stacked=True)
    with pytest.raises(ValueError, match='leading axis'):
        function(gates, [[0]], np.ones(W), omega, stacked=True)
    with pytest.raises(ValueError, match='leading axis'):
        function(gates, [[0]], np.ones((1, 1, 1, 1, W)), omega, stacked=True)
    with pytest.raises(IndexError):
        function(gates, [[3]], np.ones(W), omega)
    with pytest.raises(ValueError):
        function(gates, [[0], []], np.ones(W), omega)
    with pytest.raises(ValueError):
        function(gates, [], np.ones(W), omega)
    with pytest.raises(TypeError):
        function(gates, [[0.0]], np.ones(W), omega)
    with pytest.raises(TypeError):
        function(gates + [3], [[0]], np.ones(W), omega)


def test_the_first_bad_spectrum_raises_what_the_loop_raises(gates, monkeypatch):
    gates, omega = gates
    stand_in = Passes(monkeypatch)
    W = len(omega)
    idx = np.arange(2)
    S = np.ones((3, 3, W))
    with pytest.raises(ValueError) as loop_error:
        ff.util.parse_spectrum(S[0], omega, idx)
    with pytest.raises(ValueError) as error:
        ff.sequence_frequency_shifts(gates, [[0, 1]], S, omega, stacked=True)
    assert str(error.value) == str(loop_error.value) and 'Spectrum should be of shape' in str(error.value)
    with pytest.raises(ValueError) as loop_error:
        ff.util.get_indices_from_identifiers(gates[0].n_oper_identifiers, ['Q'])
    with pytest.raises(ValueError) as error:
        ff.sequence_frequency_shifts(gates, [[0, 1]], np.ones(W), omega, n_oper_identifiers=['Q'])
    assert str(error.value) == str(loop_error.value)
    assert not stand_in.passes and not stand_in.loops and not stand_in.own

    # in order: the parser is asked for spectrum 0 first and nothing after the one that fails
    seen = []
    real = ff.util.parse_spectrum

    def parse(spectrum, omega, idx):
        seen.append(float(np.asarray(spectrum).flat[0]))
        if seen[-1] == 2.0:
            raise ValueError('spectrum two')
        return real(spectrum, omega, idx)
    monkeypatch.setattr(so.util, 'parse_spectrum', parse)
    with pytest.raises(ValueError, match='spectrum two'):
        ff.sequence_frequency_shifts(gates, [[0]], np.arange(1.0, 5.0)[:, None]*np.ones(W), omega, stacked=True)
    assert seen == [1.0, 2.0] and not stand_in.passes and not stand_in.own


def test_routing(gates, monkeypatch):
    gates, omega = gates
    W = len(omega)
    stand_in = Passes(monkeypatch)

    def refuse(*args, **kwargs):
        raise AssertionError('a pass ran')
    monkeypatch.setattr(so, '_run_pass', refuse)
    three = [ff.PulseSequence([[np.diag([1.0, 0.0, -1.0]), [0.3], 'Z']], [[np.diag([1.0, -1.0, 0.0]), [1.0], 'N']],
                              [1.0]) for _ in range(2)]
    for g in three:
        g.cache_control_matrix(omega, np.zeros((1, 9, W), dtype=complex))
    mismatched = [gates[0], cached(gate(noise=('X',)), omega)]
    no_total = [gates[0], cached(gate(noise=('X', 'Z')), omega)]
    del no_total[1]._data['total_propagator']
    five = ('IX', 'IZ', 'XI', 'ZI', 'ZZ')
    cases = [(gates, np.ones((2, 2, W))),                      # a cross-spectrum
             (gates, np.ones(W)*(1 + 1j)),                     # weights with an imaginary part
             (three, np.ones(W)),                              # d = 3
             (mismatched, np.ones(W)),                         # other noise operators on one gate
             (no_total, np.ones(W)),                           # a gate that does not know its total propagator
             ([cached(two_qubit(five), omega)]*2, np.ones(W))]  # five noise operators
    for n, (gate_set, S) in enumerate(cases):
        assert ff.sequence_frequency_shifts(gate_set, [[0, 1], [1]], S, omega).shape == (2, 1), n
        assert len(stand_in.loops) == n + 1
    # no selected operator, one frequency
    ff.sequence_frequency_shifts(gates, [[0]], np.ones(W), omega, n_oper_identifiers=[])
    one = [cached(gate(noise=('X', 'Z')), omega[:1])]
    ff.sequence_frequency_shifts(one, [[0]], np.ones(1), omega[:1])
    assert len(stand_in.loops) == len(cases) + 2
    assert not stand_in.own                                  # the loop route asks for no gate's shifts
    # the same gate set under real weights takes the pass (complex dtype, no imaginary part: still the pass)
    for S in (np.ones(W), np.ones((2, W)), np.ones(W) + 0j):
        with pytest.raises(AssertionError, match='a pass ran'):
            ff.sequence_frequency_shifts(gates, [[0, 1]], S, omega)
    # two-qubit gates, Pauli and default basis
    pauli2 = ff.Basis.pauli(2)
    for q in ([cached(two_qubit(('IX', 'XI'), basis=pauli2), omega) for _ in range(2)],
              [cached(two_qubit(('IX', 'XI')), omega) for _ in range(2)]):
        with pytest.raises(AssertionError, match='a pass ran'):
            ff.sequence_frequency_shifts(q, [[0, 1]], np.ones((3, W)), omega, stacked=True)


def test_passes_are_split_under_the_budget_and_results_keep_their_place(gates, monkeypatch):
    gates, omega = gates
    W = len(omega)
    stand_in = Passes(monkeypatch)
    seqs = [[k % 3]*(1 + k) for k in range(11)]
    S = np.arange(1.0, 4.0)[:, None]*np.ones(W)
    whole = ff.sequence_frequency_shifts(gates, seqs, S, omega, stacked=True)
    assert len(stand_in.passes) == 1
    per_sequence = so.pass_bytes(11, 2, 2, W, 2, 3)
    monkeypatch.setattr(so, 'PASS_BYTES', so.table_bytes(3, 2, 2, W, 2, 3, 1) + 4*per_sequence)
    stand_in.passes.clear()
    stand_in.own.clear()
    split = ff.sequence_frequency_shifts(gates, seqs, S, omega, stacked=True)
    assert [len(p['indices']) for p in stand_in.passes] == [3, 4, 4]
    assert sum((p['indices'] for p in stand_in.passes), []) == seqs
    assert stand_in.own == [1.0, 2.0, 3.0]                    # once per spectrum, not once per pass
    assert np.array_equal(split, whole)
    assert [whole[k, j, 0, 0, 0] for k in range(3) for j in (0, 10)] == [
        (k + 1)*W + 1000*(j + 1) + j % 3 for k in range(3) for j in (0, 10)]


def test_not_finite_members_run_the_loops_expression(gates, monkeypatch):
    gates, omega = gates
    W = len(omega)
    # spectrum 2 of the sequence of two positions, spectra 1 and 3 of the one of three
    stand_in = Passes(monkeypatch, not_finite={(2, 2), (1, 3), (3, 3)})
    calls = []

    def single(pulse, spectrum, omega, identifiers):
        calls.append((pulse, float(np.asarray(spectrum).flat[0]), identifiers))
        return np.full((1, 4, 4), -7.0)
    monkeypatch.setattr(so, '_single', single)
    monkeypatch.setattr(so, '_concatenated', lambda gates, sequence, omega: ('pulse', sequence.tolist()))
    S = np.arange(1.0, 4.0)[:, None]*np.ones(W)
    got = ff.sequence_frequency_shifts(gates, [[0], [1, 2], [2, 2, 0]], S, omega, n_oper_identifiers=['Z'],
                                       stacked=True)
    assert calls == [(('pulse', [1, 2]), 2.0, ['Z']), (('pulse', [2, 2, 0]), 1.0, ['Z']),
                     (('pulse', [2, 2, 0]), 3.0, ['Z'])]
    replaced = np.zeros((3, 3), dtype=bool)
    replaced[1, 1] = replaced[0, 2] = replaced[2, 2] = True
    assert (got[replaced] == -7.0).all() and (got[~replaced] > 0).all()
    assert not stand_in.loops


def test_the_loops_concatenation_asks_for_the_second_order_filter_function(gates, monkeypatch):
    gates, omega = gates
    seen = []
    monkeypatch.setattr(ff, 'concatenate', lambda pulses, **kwargs: seen.append((list(pulses), kwargs)) or 'pulse')
    assert so._concatenated(gates, np.array([2, 0]), omega) == 'pulse'
    assert seen[0][0] == [gates[2], gates[0]]
    assert seen[0][1]['calc_second_order_FF'] is True and seen[0][1]['omega'] is omega


# ---- second_order=True on the existing functions ---------------------------------------------------------------------
def test_second_order_keyword(gates, monkeypatch):
    gates, omega = gates
    W = len(omega)
    seqs = [[0, 1], [2], [1, 1, 0]]
    first_order, shifts, added = [], [], []

    def results(stage, gates, sequences, spectrum, omega, identifiers, stacked, return_propagators):
        first_order.append((stage, sequences, identifiers, stacked, return_propagators))
        K = len(spectrum) if stacked else 1
        shape = (4, 4) if stage == 'error_transfer_matrix' else (2, 4, 4)
        values = np.ones((K, len(sequences)) + shape)
        values = values if stacked else values[0]
        return (values, np.zeros((len(sequences), 2, 2), dtype=complex)) if return_propagators else values

    def frequency_shifts(gates, sequences, spectrum, omega, identifiers=None, stacked=False):
        shifts.append((sequences, identifiers, stacked))
        K = len(spectrum) if stacked else 1
        values = np.full((K, len(sequences), 2, 4, 4), 2.0)
        return values if stacked else values[0]

    class Library:
        @staticmethod
        def ffk_cumulant_function_second_order(delta, n, N, d, basis, K):
            added.append((n, N, d))
            tiles = np.ctypeslib.as_array(ctypes.cast(K, ctypes.POINTER(ctypes.c_double)), (n, N, N))
            tiles += 10.0
            return 0
    monkeypatch.setattr(sp, '_results', results)
    monkeypatch.setattr(so, 'sequence_frequency_shifts', frequency_shifts)
    # second_order=False: nothing new is called, the first-order route exactly as without the keyword
    for function, stage in ((ff.sequence_cumulant_functions, 'cumulant_function'),
                            (ff.sequence_error_transfer_matrices, 'error_transfer_matrix')):
        function(gates, seqs, np.ones(W), omega, ['Z'], False, True)
        function(gates, seqs, np.ones(W), omega, ['Z'], False, True, second_order=False)
        assert first_order == [(stage, seqs, ['Z'], False, True)]*2 and not shifts and not added
        first_order.clear()
    monkeypatch.setattr(_lib, 'load', lambda: Library)
    K, U = ff.sequence_cumulant_functions(gates, seqs, np.ones((3, W)), omega, ['Z', 'X'], stacked=True,
                                          return_propagators=True, second_order=True)
    assert first_order == [('cumulant_function', seqs, ['Z', 'X'], True, True)]
    assert shifts == [(seqs, ['Z', 'X'], True)]
    assert added == [(3*3*2, 4, 2)]                               # every tile of the call, one call
    assert K.shape == (3, 3, 2, 4, 4) and (K == 11.0).all() and U.shape == (3, 2, 2)
    first_order.clear(), shifts.clear(), added.clear()
    exponentials = []
    from filter_functions_amd import numeric
    monkeypatch.setattr(numeric, 'error_transfer_matrix',
                        lambda cumulant_function: exponentials.append(cumulant_function.shape) or np.eye(4))
    E = ff.sequence_error_transfer_matrices(gates, seqs, np.ones(W), omega, second_order=True)
    # the cumulant functions of the first order, not the first-order exponentials
    assert first_order == [('cumulant_function', seqs, None, False, False)] and shifts == [(seqs, None, False)]
    assert added == [(3*2, 4, 2)] and exponentials == [(2, 4, 4)]*3 and E.shape == (3, 4, 4)

"""CPU side of ff.sequence_prefix_infidelities, ff.sequence_prefix_decay_amplitudes and ff.sequence_prefix_propagators:
the ABI in header, exports and binding, the refusals of the C entry before the device, the workspace query without a
GPU and the Python byte counts that bound it, the new kernels' resources, routing, shapes, the closing gates' checks,
the not-finite fallback and the pass split (the pass and the loop replaced by stand-ins: no GPU), and the propagators
of the truncations against explicit products."""
import ctypes

import numpy as np
import pytest

import filter_functions_amd as ff
from filter_functions_amd import _gate_table, _lib
from filter_functions_amd import sequence_prefixes as sx
from test_kernel_resources import kernels  # noqa: F401  (the module's fixture)
from test_sequence_infidelities_host import two_qubit
from test_sequences_host import cached, gate

NAMES = ('sequence_prefix_infidelities', 'sequence_prefix_decay_amplitudes', 'sequence_prefix_propagators')


def test_public_names():
    for name in NAMES:
        assert name in ff.__all__ and name in sx.__all__ and getattr(ff, name) is getattr(sx, name)
    assert ff.sequence_prefixes is sx and 'sequence_prefixes' in ff.__all__


def test_binding_header_and_exports_agree():
    import test_abi
    names = test_abi.header_symbols()
    for name in ('ffk_sequence_prefix_processes', 'ffk_sequence_prefix_processes_workspace_bytes'):
        assert name in names and name in _lib.SIGNATURES
    test_abi.test_library_exports_every_declared_symbol()
    test_abi.test_binding_table_matches_header()


def _arguments(T=3, d=2, A=2, W=5, lengths=(2, 3), closing=None, s_ndim=1, n_spectra=1, idx=(0, 1), mode=0):
    """Valid host arguments of ffk_sequence_prefix_processes (gates without handles), as a dict in argument order,
    and the arrays that keep them alive."""
    N = d*d
    n_index = sum(lengths)
    keep = dict(handles=(ctypes.c_void_p*T)(), slots=np.full(T, -1, dtype=np.int32),
                table=np.zeros((T, A, N, W), dtype=complex), U=np.tile(np.eye(d, dtype=complex), (T, 1, 1)),
                tau=np.ones(T), offsets=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32),
                index=(np.arange(n_index) % T).astype(np.int32), omega=np.linspace(0.1, 1.0, W),
                basis=np.zeros((N, d, d), dtype=complex),
                closing=None if closing is None else np.asarray(closing, dtype=np.int32),
                S=np.ones((n_spectra,) + ((W,) if s_ndim == 1 else (len(idx), W))), idx=np.asarray(idx, dtype=np.int32),
                out=np.zeros((n_spectra, n_index, len(idx), N, N)))
    p = {k: (v.ctypes.data if isinstance(v, np.ndarray) else v) for k, v in keep.items()}
    args = [p['handles'], p['slots'], p['table'], p['U'], p['tau'], T, p['offsets'], p['index'], len(lengths),
            p['omega'], W, p['basis'], 1, d, A, N, p['closing'], p['S'], s_ndim, n_spectra, p['idx'], len(idx), mode,
            p['out']]
    return args, keep


def test_bad_arguments_are_refused_before_the_device():
    lib = _lib.load()
    res, args = _lib.SIGNATURES['ffk_sequence_prefix_processes']
    assert lib.ffk_sequence_prefix_processes(*[None if a is ctypes.c_void_p else 0 for a in args]) == _lib.FFK_EINVAL
    assert 'NULL' in lib.ffk_last_error().decode()
    for change, message in ((dict(closing=[0, 1, 2, 3, 0]), 'closing[3] = 3 outside [0, 3)'),
                            (dict(closing=[0, -1, 2, 0, 0]), 'closing[1] = -1 outside'),
                            (dict(mode=3), 'mode = 3'), (dict(mode=-1), 'mode = -1'),
                            (dict(s_ndim=3), 'cross-spectra'),
                            (dict(n_spectra=0), 'n_spectra = 0'),
                            (dict(idx=(1, 1)), 'distinct'),
                            (dict(idx=(0, 2)), 'idx[1] = 2 outside [0, 2)'),
                            (dict(W=1), 'W >= 2'),
                            (dict(d=3), 'unsupported shape'),
                            (dict(A=5, idx=(0,)), 'unsupported shape')):
        args, keep = _arguments(**change)
        assert lib.ffk_sequence_prefix_processes(*args) == _lib.FFK_EINVAL, change
        assert message in lib.ffk_last_error().decode(), (change, lib.ffk_last_error().decode())
    # an index of the sequences out of range, offsets that do not increase
    args, keep = _arguments()
    keep['index'][2] = 3
    assert lib.ffk_sequence_prefix_processes(*args) == _lib.FFK_EINVAL and 'index[2]' in lib.ffk_last_error().decode()
    args, keep = _arguments()
    keep['offsets'][1] = 0
    assert lib.ffk_sequence_prefix_processes(*args) == _lib.FFK_EINVAL and 'offsets' in lib.ffk_last_error().decode()


def test_workspace_query_needs_no_gpu():
    query = _lib.load().ffk_sequence_prefix_processes_workspace_bytes
    # (T, P, n_index, n_host, d, A, N, W, n_idx, s_ndim, n_spectra, mode, has_closing)
    base = query(24, 2, 218, 0, 4, 2, 16, 301, 1, 1, 1, 2, 0)
    assert base > 218*5*8*256
    assert query(24, 2, 436, 0, 4, 2, 16, 301, 1, 1, 1, 2, 0) > base                 # grows with the positions
    assert query(24, 200, 218, 0, 4, 2, 16, 301, 1, 1, 1, 2, 0) > base               # P
    assert query(24, 2, 218, 0, 4, 2, 16, 602, 1, 1, 1, 2, 0) > base                 # W
    assert query(24, 2, 218, 0, 4, 2, 16, 301, 1, 1, 5, 2, 0) > base                 # n_spectra
    assert query(24, 2, 218, 0, 4, 2, 16, 301, 2, 1, 1, 2, 0) > base                 # n_idx
    assert query(24, 2, 218, 3, 4, 2, 16, 301, 1, 1, 1, 2, 0) >= base + 3*16*2*16*301   # host rows
    assert query(24, 2, 218, 0, 4, 2, 16, 301, 1, 1, 1, 2, 1) >= base + 4*218        # closing gates
    assert query(24, 2, 218, 0, 4, 2, 16, 301, 1, 1, 1, 1, 0) < base                 # the diagonal only
    assert query(24, 2, 218, 0, 4, 2, 16, 301, 1, 1, 1, 0, 0) < query(24, 2, 218, 0, 4, 2, 16, 301, 1, 1, 1, 1, 0)
    d2 = query(24, 2, 218, 0, 2, 1, 4, 301, 1, 2, 3, 2, 0)
    assert 0 < d2 < base
    for bad in ((24, 2, 218, 0, 3, 1, 9, 301, 1, 1, 1, 0, 0),         # d = 3
                (24, 2, 218, 0, 4, 5, 16, 301, 1, 1, 1, 0, 0),        # A = 5
                (24, 2, 218, 0, 4, 1, 4, 301, 1, 1, 1, 0, 0),         # N != d^2
                (24, 2, 218, 0, 4, 1, 16, 301, 2, 1, 1, 0, 0),        # more selected operators than there are
                (24, 2, 1, 0, 4, 1, 16, 301, 1, 1, 1, 0, 0),          # fewer positions than sequences
                (24, 2, 218, 0, 4, 1, 16, 301, 1, 3, 1, 0, 0),        # a cross-spectrum
                (24, 2, 218, 0, 4, 1, 16, 301, 1, 1, 0, 0, 0),        # no spectrum
                (24, 2, 218, 0, 4, 1, 16, 301, 1, 1, 1, 3, 0),        # no such mode
                (24, 2, 218, 0, 4, 1, 16, 301, 1, 1, 1, -1, 0),
                (24, 2, 218, 0, 4, 1, 16, 1, 1, 1, 1, 0, 0),          # one frequency: no integral
                (24, 2, 218, 25, 4, 1, 16, 301, 1, 1, 1, 0, 0),       # more host rows than gates
                (0, 2, 218, 0, 4, 1, 16, 301, 1, 1, 1, 0, 0), (24, 0, 218, 0, 4, 1, 16, 301, 1, 1, 1, 0, 0)):
        assert query(*bad) == 0, bad


def test_pass_bytes_are_pinned_and_cover_the_workspace():
    assert sx.block_width(2, 4) == 64 and sx.block_width(4, 2) == 64 and sx.block_width(4, 3) == 32
    assert sx.SPECTRA_PER_WALK == 2
    # the study's shape: 24 Cliffords, 301 frequencies (five blocks), one operator, two spectra, per POSITION
    assert sx.pass_bytes(2, 1, 301, 1, 2, 'infidelities', False) == 4 + 8*2*(1 + 5*4)
    assert sx.pass_bytes(2, 1, 301, 1, 2, 'diagonal', True) == 8 + 8*2*(4 + 5*4)
    assert sx.pass_bytes(2, 1, 301, 1, 2, 'decay_amplitudes', True) == 8 + 8*2*(16 + 5*16)
    # two-qubit gates with four operators, two of them selected: blocks of 32, three of them
    assert sx.pass_bytes(4, 4, 70, 2, 5, 'infidelities', False) == 4 + 8*10*(1 + 3*16)
    assert sx.pass_bytes(4, 4, 70, 2, 5, 'decay_amplitudes', False) == 4 + 8*10*(256 + 3*256)
    assert sx.sequence_bytes(2) == 8 + 64 and sx.sequence_bytes(4) == 8 + 256
    assert sx.table_bytes(24, 2, 1, 301, 1, 3, 1) == 24*(16*4*301 + 16*301 + 128 + 64 + 16) + 256 + 8*301 \
        + 32*3*301 + 4 + 4 + 5120
    assert sx.table_bytes(40, 4, 4, 70, 2, 5, 2) == 40*(16*4*16*70 + 16*70 + 2048 + 256 + 16) + 4096 + 560 \
        + 32*10*70 + 8 + 4 + 5120
    query = _lib.load().ffk_sequence_prefix_processes_workspace_bytes
    for d, A, W, T, P, G, n_idx, s_ndim, K in ((2, 1, 301, 24, 1050, 152, 1, 1, 3), (4, 2, 301, 27, 1050, 152, 2, 2, 3),
                                               (4, 4, 70, 40, 7, 1000, 4, 2, 5), (4, 3, 7, 3, 2, 1, 1, 1, 1),
                                               (2, 4, 65, 24, 3, 2, 4, 2, 1)):
        for mode, number in sx._MODES.items():
            for closing in (False, True):
                bound = P*(sx.sequence_bytes(d) + G*sx.pass_bytes(d, A, W, n_idx, K, mode, closing)) \
                    + sx.table_bytes(T, d, A, W, n_idx, K, s_ndim)
                assert 0 < query(T, P, P*G, T, d, A, d*d, W, n_idx, s_ndim, K, number, int(closing)) <= bound


def test_new_kernels_resources(kernels):  # noqa: F811
    d2 = {name: k for name, k in kernels.items() if 'seqpre_walk2_kernel' in name}
    d4 = {name: k for name, k in kernels.items() if 'seqpre_walk4_kernel' in name}
    assert len(d2) == 8 and len(d4) == 8, (sorted(d2), sorted(d4))                  # A = 1..4, staged and not
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
        assert k.get('.agpr_count', 0) > 0, name                # (the count above includes the accumulators)
    assert sum('seqpre_reduce_kernel' in name for name in kernels) == 1
    # the kernels of the siblings keep their names apart from the new ones
    for sibling in ('sequences4_rule_kernel', 'sequences_rule_kernel', 'sequences4_gamma_kernel',
                    'sequences_gamma_kernel', 'seq2o_walk2_kernel', 'seq2o_walk4_kernel'):
        assert sum(sibling in name for name in kernels) == 8, sibling


# ---- the gate table with closing gates ------------------------------------------------------------------------------
def test_pass_table_holds_the_closing_gates():
    omega = np.linspace(0.1, 1.0, 5)
    gates = [cached(gate(noise=('X', 'Z')), omega) for _ in range(6)]
    plan = _gate_table.batched_plan(gates, omega)
    indices = [np.array([4, 1], dtype=np.int32), np.array([1], dtype=np.int32)]
    plain = _gate_table.PassTable(gates, indices, plan, omega)
    assert plain.used.tolist() == [1, 4] and plain.index.tolist() == [1, 0, 0] and plain.extra is None
    closing = [np.array([5, 1], dtype=np.int32), np.array([0], dtype=np.int32)]
    table = _gate_table.PassTable(gates, indices, plan, omega, extra=closing)
    assert table.used.tolist() == [0, 1, 4, 5] and [g is gates[k] for g, k in zip(table.gates, table.used)]
    assert table.index.tolist() == [2, 1, 1] and table.offsets.tolist() == [0, 2, 3]
    assert table.extra.tolist() == [3, 1, 0] and table.extra.dtype == np.int32
    assert len(table.c_arguments()) == 16 and table.c_arguments()[5] == 4


# ---- stand-ins for the device and the loop --------------------------------------------------------------------------
@pytest.fixture
def gates():
    omega = np.linspace(0.1, 1.0, 5)
    return [cached(gate(noise=('X', 'Z')), omega) for _ in range(3)], omega


_SHAPES = {'infidelities': (), 'diagonal': (4,), 'decay_amplitudes': (4, 4)}


class Passes:
    """Replaces the module's pass and loop: records what they were asked for and returns recognisable values."""

    def __init__(self, monkeypatch, not_finite=()):
        self.passes, self.loops, self.not_finite = [], [], set(not_finite)
        monkeypatch.setattr(sx, '_run_pass', self.run_pass)
        monkeypatch.setattr(sx, '_loop', self.loop)

    def run_pass(self, gates, indices, close, plan, omega, S, idx, mode):
        self.passes.append(dict(indices=[i.tolist() for i in indices], S=S.copy(), idx=list(idx), mode=mode,
                                close=None if close is None else [c.tolist() for c in close]))
        K, n_index = len(S), sum(len(i) for i in indices)
        out = np.empty((K, n_index, len(idx)) + _SHAPES[mode])
        at = 0
        for i in indices:
            for g in range(len(i)):
                for k in range(K):
                    out[k, at] = S[k].sum() + 1000*len(i) + 10*g + i[0]
                    if (int(round(S[k].flat[0])), len(i)) in self.not_finite and g == len(i) - 1:
                        out[k, at] = np.nan
                at += 1
        return out

    def loop(self, mode, gates, indices, close, spectra, omega, n_oper_identifiers, want_U):
        self.loops.append(dict(spectra=spectra, mode=mode, close=close))
        values = [np.full((len(spectra), len(i), 1), -1.0) for i in indices]
        return values, [np.ones((len(i), 2, 2)) for i in indices] if want_U else None


def test_shapes_stacked_and_not(gates, monkeypatch):
    gates, omega = gates
    seqs = [[0, 1], [2], [1, 1, 0]]
    stand_in = Passes(monkeypatch)
    W = len(omega)
    calls = ((ff.sequence_prefix_infidelities, {}, (2,), 'infidelities'),
             (ff.sequence_prefix_decay_amplitudes, {}, (2, 4, 4), 'decay_amplitudes'),
             (ff.sequence_prefix_decay_amplitudes, dict(diagonal=True), (2, 4), 'diagonal'))
    for function, kwargs, shape, mode in calls:
        one = function(gates, seqs, np.ones(W), omega, **kwargs)
        assert isinstance(one, list) and [a.shape for a in one] == [(len(s),) + shape for s in seqs]
        assert stand_in.passes[-1]['mode'] == mode and stand_in.passes[-1]['close'] is None
        for S in (np.ones((4, W)), np.ones((4, 2, W)), np.ones((4, 1, W))):
            got = function(gates, seqs, S, omega, stacked=True, **kwargs)
            assert [a.shape for a in got] == [(4, len(s)) + shape for s in seqs]
            assert stand_in.passes[-1]['S'].shape == (4,) + ((W,) if S.ndim == 2 else (2, W))
        got, U = function(gates, seqs, np.ones((1, W)), omega, stacked=True, return_propagators=True, **kwargs)
        assert [a.shape for a in got] == [(1, len(s)) + shape for s in seqs]
        assert [u.shape for u in U] == [(len(s), 2, 2) for s in seqs]
        assert all(np.array_equal(a[0], b) for a, b in zip(got, one))
    assert not stand_in.loops
    # every position keeps its place: sequence 2 has three positions, first gate 1
    one = ff.sequence_prefix_infidelities(gates, seqs, np.ones(W), omega)
    assert one[2][:, 0].tolist() == [W + 3000 + 10*g + 1 for g in range(3)] and one[1][0, 0] == W + 1000 + 2
    # a subset of the operators, not in sorted order: their indices reach the pass
    S = np.arange(2*2*W, dtype=float).reshape(2, 2, W)
    ff.sequence_prefix_decay_amplitudes(gates, seqs, S, omega, n_oper_identifiers=['Z', 'X'], stacked=True)
    assert stand_in.passes[-1]['idx'] == [1, 0] and np.array_equal(stand_in.passes[-1]['S'], S)
    # closing gates reach the pass as index arrays, negative ones wrapped
    ff.sequence_prefix_infidelities(gates, seqs, np.ones(W), omega, closing=[[0, -1], [1], [2, 2, -3]])
    assert stand_in.passes[-1]['close'] == [[0, 2], [1], [2, 2, 0]]
    # (K, n_idx, n_idx, W): cross-spectra, the loop
    C = np.ones((3, 2, 2, W))
    got = ff.sequence_prefix_decay_amplitudes(gates, seqs, C, omega, stacked=True)
    assert [a.shape for a in got] == [(3, len(s), 1) for s in seqs]
    assert len(stand_in.loops) == 1 and len(stand_in.loops[0]['spectra']) == 3
    # without stacked a two-dimensional spectrum is one spectrum
    assert ff.sequence_prefix_decay_amplitudes(gates, seqs, np.ones((2, W)), omega)[0].shape == (2, 2, 4, 4)
    assert stand_in.passes[-1]['S'].shape == (1, 2, W)


def test_refusals(gates, monkeypatch):
    gates, omega = gates
    stand_in = Passes(monkeypatch)
    W = len(omega)
    for function in (ff.sequence_prefix_infidelities, ff.sequence_prefix_decay_amplitudes):
        with pytest.raises(ValueError, match='at least one spectrum'):
            function(gates, [[0]], np.ones((0, W)), omega, stacked=True)
        with pytest.raises(ValueError, match='leading axis'):
            function(gates, [[0]], np.ones(W), omega, stacked=True)
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
        # the closing gates: one array per sequence, as long as it, read by the rules of the index arrays
        with pytest.raises(ValueError, match='closing holds 1 arrays for 2 sequences'):
            function(gates, [[0, 1], [1]], np.ones(W), omega, closing=[[0, 1]])
        with pytest.raises(ValueError, match=r'closing\[1\]: expected 1 gate indices'):
            function(gates, [[0, 1], [1]], np.ones(W), omega, closing=[[0, 1], [1, 2]])
        with pytest.raises(ValueError, match=r'closing\[0\]'):
            function(gates, [[0, 1]], np.ones(W), omega, closing=[[[0, 1]]])
        with pytest.raises(IndexError, match=r'^closing\[1\]: index 3 is out of bounds for 3 gates'):
            function(gates, [[1], [0, 1]], np.ones(W), omega, closing=[[0], [0, 3]])
        with pytest.raises(IndexError, match=r'^closing\[0\]: index -4'):
            function(gates, [[0, 1]], np.ones(W), omega, closing=[[-4, 0]])
        with pytest.raises(TypeError, match=r'^closing\[0\]: gate indices must be integers'):
            function(gates, [[0, 1]], np.ones(W), omega, closing=[[0.0, 1.0]])
        # unknown identifiers: the message of the single functions
        with pytest.raises(ValueError) as loop_error:
            ff.util.get_indices_from_identifiers(gates[0].n_oper_identifiers, ['Q'])
        with pytest.raises(ValueError) as error:
            function(gates, [[0, 1]], np.ones(W), omega, n_oper_identifiers=['Q'])
        assert str(error.value) == str(loop_error.value)
    with pytest.raises(ValueError, match='closing holds'):
        ff.sequence_prefix_propagators(gates, [[0, 1]], closing=[])
    with pytest.raises(IndexError):
        ff.sequence_prefix_propagators(gates, [[0, 3]])
    assert not stand_in.passes and not stand_in.loops


def test_routing(gates, monkeypatch):
    gates, omega = gates
    W = len(omega)
    stand_in = Passes(monkeypatch)

    def refuse(*args, **kwargs):
        raise AssertionError('a pass ran')
    monkeypatch.setattr(sx, '_run_pass', refuse)
    three = [ff.PulseSequence([[np.diag([1.0, 0.0, -1.0]), [0.3], 'Z']], [[np.diag([1.0, -1.0, 0.0]), [1.0], 'N']],
                              [1.0]) for _ in range(2)]
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
    for function in (ff.sequence_prefix_infidelities, ff.sequence_prefix_decay_amplitudes):
        for n, (gate_set, S) in enumerate(cases):
            if n == 2:
                for g in gate_set:
                    g.cache_control_matrix(omega, np.zeros((1, 9, W), dtype=complex))
            got = function(gate_set, [[0, 1], [1]], S, omega, closing=[[1, 0], [0]])
            assert [a.shape for a in got] == [(2, 1), (1, 1)], n
            assert len(stand_in.loops) == n + 1
            assert [c.tolist() for c in stand_in.loops[-1]['close']] == [[1, 0], [0]]
        # no selected operator, an operator selected twice, one frequency
        function(gates, [[0]], np.ones(W), omega, n_oper_identifiers=[])
        function(gates, [[0]], np.ones(W), omega, n_oper_identifiers=['X', 'X'])
        one = [cached(gate(noise=('X', 'Z')), omega[:1])]
        function(one, [[0]], np.ones(1), omega[:1])
        assert len(stand_in.loops) == len(cases) + 3
        stand_in.loops.clear()
    # the same gate set under real weights takes the pass (complex dtype, no imaginary part: still the pass)
    for S in (np.ones(W), np.ones((2, W)), np.ones(W) + 0j):
        with pytest.raises(AssertionError, match='a pass ran'):
            ff.sequence_prefix_infidelities(gates, [[0, 1]], S, omega)
    # two-qubit gates, Pauli and default basis
    pauli2 = ff.Basis.pauli(2)
    for q in ([cached(two_qubit(('IX', 'XI'), basis=pauli2), omega) for _ in range(2)],
              [cached(two_qubit(('IX', 'XI')), omega) for _ in range(2)]):
        with pytest.raises(AssertionError, match='a pass ran'):
            ff.sequence_prefix_decay_amplitudes(q, [[0, 1]], np.ones((3, W)), omega, stacked=True, diagonal=True)


def test_passes_are_split_under_the_budget_and_results_keep_their_place(gates, monkeypatch):
    gates, omega = gates
    W = len(omega)
    stand_in = Passes(monkeypatch)
    seqs = [[k % 3]*(1 + k) for k in range(11)]
    closing = [[(k + g) % 3 for g in range(1 + k)] for k in range(11)]
    S = np.arange(1.0, 4.0)[:, None]*np.ones(W)
    whole = ff.sequence_prefix_decay_amplitudes(gates, seqs, S, omega, closing=closing, stacked=True)
    assert len(stand_in.passes) == 1
    # passes are filled by their positions: a budget of the tables, 20 positions and their sequences takes the
    # sequences of 1 ... 5 gates (15 positions), then 6 + 7, 8 + 9, 10 and 11
    per_position = sx.pass_bytes(2, 2, W, 2, 3, 'decay_amplitudes', True)
    monkeypatch.setattr(sx, 'PASS_BYTES', sx.table_bytes(3, 2, 2, W, 2, 3, 1) + 20*per_position + 5*sx.sequence_bytes(2))
    stand_in.passes.clear()
    split = ff.sequence_prefix_decay_amplitudes(gates, seqs, S, omega, closing=closing, stacked=True)
    assert [len(p['indices']) for p in stand_in.passes] == [5, 2, 2, 1, 1]
    assert sum((p['indices'] for p in stand_in.passes), []) == seqs
    assert sum((p['close'] for p in stand_in.passes), []) == closing
    assert all(np.array_equal(a, b) for a, b in zip(split, whole))
    assert [whole[j][k, g, 0, 0, 0] for k in range(3) for j in (0, 10) for g in (0, j)] == [
        (k + 1)*W + 1000*(j + 1) + 10*g + j % 3 for k in range(3) for j in (0, 10) for g in (0, j)]


def test_split_sequences_and_the_staged_criterion():
    assert sx.split_sequences([3, 3, 3, 3], 10, 5, 70) == [[0, 1], [2, 3]]
    assert sx.split_sequences([3, 3, 3, 3], 10, 5, 10**6) == [[0, 1, 2, 3]]
    assert sx.split_sequences([3, 3, 3, 3], 10, 5, 10**6, max_sequences=3) == [[0, 1, 2], [3]]
    assert sx.split_sequences([9, 1, 1, 9], 10, 0, 20) == [[0], [1, 2], [3]]       # a sequence over the budget: alone
    assert sx.split_sequences([5], 10, 5, -100) == [[0]] and sx.split_sequences([], 10, 5, 100) == []
    # the tables of a pass in LDS: 16 T (A d^2 + 1) width bytes, at d = 4 behind 8*2*A*width of weights, within 150 KiB
    assert sx.staged(2, 24, 1) and 24*5*64*16 == 122880 and not sx.staged(2, 31, 1) and sx.staged(2, 30, 1)
    assert sx.staged(2, 8, 4) and not sx.staged(2, 24, 4)
    assert sx.staged(4, 3, 2) and 3*33*64*16 + 2048 == 103424 and not sx.staged(4, 5, 2) and not sx.staged(4, 40, 2)
    assert sx.staged(4, 4, 4) and not sx.staged(4, 5, 4) and sx.staged(4, 8, 1) and not sx.staged(4, 9, 1)


def test_not_finite_curves_run_the_loops_expression(gates, monkeypatch):
    gates, omega = gates
    W = len(omega)
    # spectrum 2 of the sequence of two positions, spectra 1 and 3 of the one of three
    stand_in = Passes(monkeypatch, not_finite={(2, 2), (1, 3), (3, 3)})
    calls = []

    def single(mode, pulse, spectrum, omega, identifiers):
        calls.append((mode, pulse, float(np.asarray(spectrum).flat[0]), identifiers))
        return np.full((1, 4), -7.0)
    monkeypatch.setattr(sx, '_single', single)
    monkeypatch.setattr(sx, '_concatenated', lambda gates, sequence, closer, omega: (sequence.tolist(), closer))
    S = np.arange(1.0, 4.0)[:, None]*np.ones(W)
    got = ff.sequence_prefix_decay_amplitudes(gates, [[0], [1, 2], [2, 2, 0]], S, omega, n_oper_identifiers=['Z'],
                                              closing=[[1], [0, 0], [1, 2, 0]], diagonal=True, stacked=True)
    # the whole curve of the (spectrum, sequence) is recomputed, every truncation with its closing gate
    assert calls == [('diagonal', ([1], 0), 2.0, ['Z']), ('diagonal', ([1, 2], 0), 2.0, ['Z']),
                     ('diagonal', ([2], 1), 1.0, ['Z']), ('diagonal', ([2, 2], 2), 1.0, ['Z']),
                     ('diagonal', ([2, 2, 0], 0), 1.0, ['Z']),
                     ('diagonal', ([2], 1), 3.0, ['Z']), ('diagonal', ([2, 2], 2), 3.0, ['Z']),
                     ('diagonal', ([2, 2, 0], 0), 3.0, ['Z'])]
    assert (got[0] > 0).all()
    assert (got[1][1] == -7.0).all() and (got[1][[0, 2]] > 0).all()
    assert (got[2][[0, 2]] == -7.0).all() and (got[2][1] > 0).all()
    assert not stand_in.loops


# ---- the propagators of the truncations -----------------------------------------------------------------------------
def _unitaries(rng, n, d):
    out = []
    for _ in range(n):
        q, r = np.linalg.qr(rng.standard_normal((d, d)) + 1j*rng.standard_normal((d, d)))
        out.append(q*(np.diagonal(r)/abs(np.diagonal(r))))
    return out


@pytest.mark.parametrize('d', [2, 4])
def test_prefix_propagators_against_explicit_products(d):
    rng = np.random.default_rng(40 + d)
    omega = np.linspace(0.1, 1.0, 5)
    gates = []
    for U in _unitaries(rng, 5, d):
        pulse = cached(gate(d=d) if d == 4 else gate(), omega)
        pulse._data['total_propagator'] = U
        gates.append(pulse)
    U = [g.total_propagator for g in gates]
    seqs = [[0, 1, 2, 3, 4, 4, 0], [3], [-1, -5, 2], rng.integers(0, 5, 70)]
    closing = [[4, 3, 2, 1, 0, -1, -2], [0], [1, 1, 1], rng.integers(-5, 5, 70)]
    for close in (None, closing):
        got = ff.sequence_prefix_propagators(gates, seqs, closing=close)
        assert [g.shape for g in got] == [(len(s), d, d) for s in seqs] and all(g.dtype == complex for g in got)
        for p, s in enumerate(seqs):
            current = np.eye(d, dtype=complex)
            for m, k in enumerate(s):
                current = U[k] @ current
                want = current if close is None else U[close[p][m]] @ current
                assert np.allclose(got[p][m], want, rtol=0, atol=1e-13), (p, m)
                assert np.allclose(got[p][m].conj().T @ got[p][m], np.eye(d), rtol=0, atol=1e-12)
    # the same sequences in another order and alone: the same bits (a position sees its own sequence only)
    alone = ff.sequence_prefix_propagators(gates, [seqs[3]], closing=[closing[3]])[0]
    assert np.array_equal(alone, ff.sequence_prefix_propagators(gates, seqs, closing=closing)[3])
    assert np.array_equal(alone[:7], ff.sequence_prefix_propagators(gates, [seqs[3][:7]], closing=[closing[3][:7]])[0])

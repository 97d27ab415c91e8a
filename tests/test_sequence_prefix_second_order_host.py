"""CPU side of ff.sequence_prefix_frequency_shifts and ff.sequence_prefix_cumulant_functions: the ABI in header, exports
and binding, the refusals of the C entry before the device, the workspace query without a GPU and the Python byte counts
that bound it, the new kernels' resources, routing, shapes, the not-finite fallback and the pass split (the pass and the
loop replaced by stand-ins: no GPU), and the host composition of the cumulant functions against the documented formula."""
import ctypes

import numpy as np
import pytest

import ff_oracle as orc
import filter_functions_amd as ff
from filter_functions_amd import _lib
from filter_functions_amd import sequence_prefix_second_order as sp2
from test_kernel_resources import kernels  # noqa: F401  (the module's fixture)
from test_sequence_infidelities_host import two_qubit
from test_sequences_host import cached, gate

NAMES = ('sequence_prefix_frequency_shifts', 'sequence_prefix_cumulant_functions')
ENTRY = 'ffk_sequence_prefix_frequency_shifts'


def test_public_names():
    for name in NAMES:
        assert name in ff.__all__ and name in sp2.__all__ and getattr(ff, name) is getattr(sp2, name)
    assert ff.sequence_prefix_second_order is sp2 and 'sequence_prefix_second_order' in ff.__all__
    # what is read as sequence_prefixes reads it is imported, not copied
    from filter_functions_amd import sequence_prefixes as sx, sequence_processes
    assert sp2._closing_arrays is sx._closing_arrays and sp2._products is sx._products
    assert sp2.split_sequences is sx.split_sequences and sp2.stacked_spectra is sequence_processes.stacked_spectra
    for function in (ff.sequence_prefix_frequency_shifts, ff.sequence_prefix_cumulant_functions):
        assert 'SHARED' not in function.__doc__ and 'closing' in function.__doc__
    assert 'ff.frequency_shifts' in ff.sequence_prefix_frequency_shifts.__doc__
    assert 'WITHOUT ``filter_function_2``' in ff.sequence_prefix_frequency_shifts.__doc__


def test_binding_header_and_exports_agree():
    import test_abi
    names = test_abi.header_symbols()
    for name in (ENTRY, ENTRY + '_workspace_bytes'):
        assert name in names and name in _lib.SIGNATURES
    test_abi.test_library_exports_every_declared_symbol()
    test_abi.test_binding_table_matches_header()


def _arguments(T=3, d=2, A=2, W=5, lengths=(2, 3), closing=None, s_ndim=1, n_spectra=1, idx=(0, 1)):
    """Valid host arguments of the entry (gates without handles), in argument order, and the arrays that keep them
    alive."""
    N = d*d
    n_index = sum(lengths)
    keep = dict(handles=(ctypes.c_void_p*T)(), slots=np.full(T, -1, dtype=np.int32),
                table=np.zeros((T, A, N, W), dtype=complex), U=np.tile(np.eye(d, dtype=complex), (T, 1, 1)),
                tau=np.ones(T), offsets=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32),
                index=(np.arange(n_index) % T).astype(np.int32), omega=np.linspace(0.1, 1.0, W),
                basis=np.zeros((N, d, d), dtype=complex),
                closing=None if closing is None else np.asarray(closing, dtype=np.int32),
                S=np.ones((max(n_spectra, 1),) + ((W,) if s_ndim == 1 else (len(idx), W))),
                idx=np.asarray(idx, dtype=np.int32), shifts=np.zeros((max(n_spectra, 1), T, len(idx), N, N)),
                out=np.zeros((max(n_spectra, 1), n_index, len(idx), N, N)))
    p = {k: (v.ctypes.data if isinstance(v, np.ndarray) else v) for k, v in keep.items()}
    args = [p['handles'], p['slots'], p['table'], p['U'], p['tau'], T, p['offsets'], p['index'], len(lengths),
            p['omega'], W, p['basis'], 1, d, A, N, p['closing'], p['S'], s_ndim, n_spectra, p['idx'], len(idx),
            p['shifts'], p['out']]
    return args, keep


def test_bad_arguments_are_refused_before_the_device():
    lib = _lib.load()
    entry = getattr(lib, ENTRY)
    res, args = _lib.SIGNATURES[ENTRY]
    assert len(args) == 24
    assert entry(*[None if a is ctypes.c_void_p else 0 for a in args]) == _lib.FFK_EINVAL
    assert 'NULL' in lib.ffk_last_error().decode()
    # every pointer that must be there, one at a time (closing, argument 16, and the host table, 2, may be NULL)
    for position in (0, 1, 3, 4, 6, 7, 9, 11, 17, 20, 22, 23):
        args, keep = _arguments()
        args[position] = None
        assert entry(*args) == _lib.FFK_EINVAL and 'NULL' in lib.ffk_last_error().decode(), position
    for change, message in ((dict(closing=[0, 1, 2, 3, 0]), 'closing[3] = 3 outside [0, 3)'),
                            (dict(closing=[0, -1, 2, 0, 0]), 'closing[1] = -1 outside'),
                            (dict(s_ndim=3), 'cross-spectra'),
                            (dict(n_spectra=0), 'n_spectra = 0'),
                            (dict(idx=(1, 1)), 'distinct'),
                            (dict(idx=(0, 2)), 'idx[1] = 2 outside [0, 2)'),
                            (dict(W=1), 'W >= 2'),
                            (dict(d=3), 'unsupported shape'),
                            (dict(A=5, idx=(0,)), 'unsupported shape')):
        args, keep = _arguments(**change)
        assert entry(*args) == _lib.FFK_EINVAL, change
        assert message in lib.ffk_last_error().decode(), (change, lib.ffk_last_error().decode())
    # an index of the sequences out of range, offsets that do not start at 0 or do not increase
    args, keep = _arguments()
    keep['index'][2] = 3
    assert entry(*args) == _lib.FFK_EINVAL and 'index[2]' in lib.ffk_last_error().decode()
    args, keep = _arguments()
    keep['offsets'][1] = 0
    assert entry(*args) == _lib.FFK_EINVAL and 'offsets' in lib.ffk_last_error().decode()
    args, keep = _arguments()
    keep['offsets'][0] = 1
    assert entry(*args) == _lib.FFK_EINVAL and 'offsets[0]' in lib.ffk_last_error().decode()


def test_workspace_query_needs_no_gpu():
    query = getattr(_lib.load(), ENTRY + '_workspace_bytes')
    # (T, P, n_index, n_host, d, A, N, W, n_idx, s_ndim, n_spectra, has_closing)
    base = query(24, 2, 218, 0, 4, 2, 16, 301, 1, 1, 1, 0)
    assert base > 218*(1 + 5)*8*256
    assert query(24, 2, 436, 0, 4, 2, 16, 301, 1, 1, 1, 0) > base                 # grows with the positions
    assert query(24, 200, 218, 0, 4, 2, 16, 301, 1, 1, 1, 0) > base               # P
    assert query(24, 2, 218, 0, 4, 2, 16, 602, 1, 1, 1, 0) > base                 # W
    assert query(24, 2, 218, 0, 4, 2, 16, 301, 1, 1, 5, 0) > base                 # n_spectra
    assert query(24, 2, 218, 0, 4, 2, 16, 301, 2, 1, 1, 0) > base                 # n_idx
    assert query(24, 2, 218, 3, 4, 2, 16, 301, 1, 1, 1, 0) >= base + 3*16*2*16*301   # host rows
    assert query(24, 2, 218, 0, 4, 2, 16, 301, 1, 1, 1, 1) >= base + 4*218        # closing gates
    # the gates' own shifts are part of it: more than the decay amplitudes of the same shape need
    prefix = _lib.load().ffk_sequence_prefix_processes_workspace_bytes
    assert base >= prefix(24, 2, 218, 0, 4, 2, 16, 301, 1, 1, 1, 2, 0) + 8*24*256
    assert 0 < query(24, 2, 218, 0, 2, 1, 4, 301, 1, 2, 3, 0) < base
    for bad in ((24, 2, 218, 0, 3, 1, 9, 301, 1, 1, 1, 0),         # d = 3
                (24, 2, 218, 0, 4, 5, 16, 301, 1, 1, 1, 0),        # A = 5
                (24, 2, 218, 0, 4, 1, 16, 301, 1, 3, 1, 0),        # s_ndim 3: a cross-spectrum
                (24, 2, 218, 0, 4, 1, 4, 301, 1, 1, 1, 0),         # N != d^2
                (24, 2, 218, 0, 4, 1, 16, 301, 2, 1, 1, 0),        # more selected operators than there are
                (24, 2, 1, 0, 4, 1, 16, 301, 1, 1, 1, 0),          # fewer positions than sequences
                (24, 2, 218, 0, 4, 1, 16, 301, 1, 1, 0, 0),        # no spectrum
                (24, 2, 218, 0, 4, 1, 16, 1, 1, 1, 1, 0),          # one frequency: no integral
                (24, 2, 218, 25, 4, 1, 16, 301, 1, 1, 1, 0),       # more host rows than gates
                (0, 2, 218, 0, 4, 1, 16, 301, 1, 1, 1, 0), (24, 0, 218, 0, 4, 1, 16, 301, 1, 1, 1, 0)):
        assert query(*bad) == 0, bad


def test_pass_bytes_are_pinned_and_cover_the_workspace():
    assert sp2.block_width(2, 4) == 64 and sp2.block_width(4, 2) == 64 and sp2.block_width(4, 3) == 32
    # spectra of one walk: what the registers hold, a function of (d, A, closing) alone
    assert [sp2.spectra_per_walk(2, A, c) for A in (1, 2, 3, 4) for c in (False, True)] == [2, 2, 2, 2, 2, 2, 1, 1]
    assert [sp2.spectra_per_walk(4, A, c) for A in (1, 2, 3, 4) for c in (False, True)] == [2, 2, 2, 2, 2, 1, 1, 1]
    # the study's shape: 24 Cliffords, 301 frequencies (five blocks), one operator, two spectra, per POSITION
    assert sp2.pass_bytes(2, 1, 301, 1, 2, False) == 4 + 8*2*16*(1 + 5)
    assert sp2.pass_bytes(2, 1, 301, 1, 2, True) == 8 + 8*2*16*(1 + 5)
    # two-qubit gates with four operators, two of them selected: blocks of 32, three of them
    assert sp2.pass_bytes(4, 4, 70, 2, 5, False) == 4 + 8*10*256*(1 + 3)
    assert sp2.sequence_bytes(2) == 8 + 64 and sp2.sequence_bytes(4) == 8 + 256
    assert sp2.table_bytes(24, 2, 1, 301, 1, 3, 1) == 24*(16*4*301 + 16*301 + 128 + 64 + 16 + 8*16*3) + 256 + 8*301 \
        + 32*3*301 + 4 + 4 + 5120
    assert sp2.table_bytes(40, 4, 4, 70, 2, 5, 2) == 40*(16*4*16*70 + 16*70 + 2048 + 256 + 16 + 8*256*10) + 4096 \
        + 560 + 32*10*70 + 8 + 4 + 5120
    query = getattr(_lib.load(), ENTRY + '_workspace_bytes')
    for d, A, W, T, P, G, n_idx, s_ndim, K in ((2, 1, 301, 24, 1050, 152, 1, 1, 3), (4, 2, 301, 27, 1050, 152, 2, 2, 3),
                                               (4, 2, 301, 24, 1050, 152, 2, 1, 3),
                                               (4, 4, 70, 40, 7, 1000, 4, 2, 5), (4, 3, 7, 3, 2, 1, 1, 1, 1),
                                               (2, 4, 65, 24, 3, 2, 4, 2, 1)):
        for closing in (False, True):
            bound = P*(sp2.sequence_bytes(d) + G*sp2.pass_bytes(d, A, W, n_idx, K, closing)) \
                + sp2.table_bytes(T, d, A, W, n_idx, K, s_ndim)
            assert 0 < query(T, P, P*G, T, d, A, d*d, W, n_idx, s_ndim, K, int(closing)) <= bound, (d, A, closing)
    # the tables of a pass in LDS: 16 T (A d^2 + 1) width bytes, at d = 4 behind the weights, within 150 KiB
    assert sp2.staged(2, 24, 1, True) and not sp2.staged(2, 31, 1, False) and sp2.staged(2, 30, 1, True)
    assert sp2.staged(4, 3, 2, True) and not sp2.staged(4, 5, 2, False) and not sp2.staged(4, 40, 2, True)
    assert sp2.staged(4, 4, 4, True) and not sp2.staged(4, 5, 4, False)


def test_new_kernels_resources(kernels):  # noqa: F811
    d2 = {name: k for name, k in kernels.items() if 'seqpre2o_walk2_kernel' in name}
    d4 = {name: k for name, k in kernels.items() if 'seqpre2o_walk4_kernel' in name}
    # A = 1..4, staged and not, with and without closing gates
    assert len(d2) == 16 and len(d4) == 16, (sorted(d2), sorted(d4))
    for a in range(1, 5):
        assert sum(f'ILi{a}E' in name for name in d2) == 4 and sum(f'ILi{a}E' in name for name in d4) == 4
    for name, k in {**d2, **d4}.items():
        assert k['.private_segment_fixed_size'] == 0, name
        assert k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, name
        assert k['.group_segment_fixed_size'] == 0, name        # (tables and weights are sized at the launch)
        # 256 threads are four wavefronts, one per SIMD: the whole file of 512 registers, accumulators included
        assert k['.max_flat_workgroup_size'] == 256, name
        assert k['.vgpr_count'] <= 512, (name, k['.vgpr_count'], k.get('.agpr_count'))
        assert k['.sgpr_count'] <= 108, (name, k['.sgpr_count'])
    # the registers as ranges (vector registers and accumulators together): lane = frequency at d = 2, the matrix
    # instruction's tiles at d = 4; the largest are the walks of two spectra read from L2
    for name, k in d2.items():
        assert 200 <= k['.vgpr_count'] <= 448, (name, k['.vgpr_count'])
    for name, k in d4.items():
        assert 224 <= k['.vgpr_count'] <= 512, (name, k['.vgpr_count'])
        assert k.get('.agpr_count', 0) > 0, name                # (the count above includes the accumulators)
    assert sum('seqpre2o_reduce_kernel' in name for name in kernels) == 1
    reduce = [k for name, k in kernels.items() if 'seqpre2o_reduce_kernel' in name][0]
    assert reduce['.vgpr_count'] <= 32 and reduce['.private_segment_fixed_size'] == 0
    # the LDS of the staged criterion, sized at the launch: within the 160 KiB of a compute unit
    for d, T, A in ((2, 30, 1), (2, 24, 1), (4, 3, 2), (4, 4, 4), (4, 8, 1)):
        for closing in (False, True):
            assert sp2.staged(d, T, A, closing)
            width = sp2.block_width(d, A)
            weights = 0 if d == 2 else 8*sp2.spectra_per_walk(d, A, closing)*A*width
            assert 100*1024 <= 16*T*(A*d*d + 1)*width + weights <= 150*1024
    # the kernels of the siblings keep their names apart from the new ones
    for sibling in ('seq2o_walk2_kernel', 'seq2o_walk4_kernel', 'seqpre_walk2_kernel', 'seqpre_walk4_kernel'):
        assert sum(sibling in name for name in kernels) == 8, sibling


# ---- stand-ins for the device and the loop --------------------------------------------------------------------------
@pytest.fixture
def gates():
    omega = np.linspace(0.1, 1.0, 5)
    return [cached(gate(noise=('X', 'Z')), omega) for _ in range(3)], omega


class Passes:
    """Replaces the module's pass, loop and the gates' own shifts: records what they were asked for and returns
    recognisable values."""

    def __init__(self, monkeypatch, not_finite=()):
        self.passes, self.loops, self.own, self.not_finite = [], [], [], set(not_finite)
        monkeypatch.setattr(sp2, '_run_pass', self.run_pass)
        monkeypatch.setattr(sp2, '_loop', self.loop)
        monkeypatch.setattr(sp2, '_gate_shifts', self.gate_shifts)

    def gate_shifts(self, gates, spectrum, omega, names):
        self.own.append(np.asarray(spectrum))
        n_idx = len(ff.util.get_indices_from_identifiers(gates[0].n_oper_identifiers, names))
        return np.full((len(gates), n_idx, 4, 4), float(np.real(np.asarray(spectrum).flat[0])))

    def run_pass(self, gates, indices, close, plan, omega, S, idx, shifts):
        self.passes.append(dict(indices=[i.tolist() for i in indices], S=S.copy(), idx=list(idx),
                                shifts=np.array(shifts), close=None if close is None else [c.tolist() for c in close]))
        K, n_index = len(S), sum(len(i) for i in indices)
        out = np.empty((K, n_index, len(idx), 4, 4))
        at = 0
        for i in indices:
            for g in range(len(i)):
                for k in range(K):
                    out[k, at] = S[k].sum() + 1000*len(i) + 10*g + i[0]
                    if (int(round(S[k].flat[0])), len(i)) in self.not_finite and g == len(i) - 1:
                        out[k, at, 0, 1, 2] = np.inf
                at += 1
        return out

    def loop(self, gates, indices, close, spectra, omega, n_oper_identifiers, want_U, single=None):
        self.loops.append(dict(spectra=spectra, close=close))
        values = [np.full((len(spectra), len(i), 1), -1.0) for i in indices]
        return values, [np.ones((len(i), 2, 2)) for i in indices] if want_U else None


def test_shapes_stacked_and_not(gates, monkeypatch):
    gates, omega = gates
    seqs = [[0, 1], [2], [1, 1, 0]]
    stand_in = Passes(monkeypatch)
    W = len(omega)
    function, shape = ff.sequence_prefix_frequency_shifts, (2, 4, 4)
    one = function(gates, seqs, np.ones(W), omega)
    assert isinstance(one, list) and [a.shape for a in one] == [(len(s),) + shape for s in seqs]
    assert stand_in.passes[-1]['close'] is None and stand_in.passes[-1]['shifts'].shape == (1, 3, 2, 4, 4)
    for S in (np.ones((4, W)), np.ones((4, 2, W)), np.ones((4, 1, W))):
        stand_in.own.clear()
        got = function(gates, seqs, S, omega, stacked=True)
        assert [a.shape for a in got] == [(4, len(s)) + shape for s in seqs]
        assert stand_in.passes[-1]['S'].shape == (4,) + ((W,) if S.ndim == 2 else (2, W))
        # the gates' own shifts: one call per spectrum, with the spectrum as the caller gave it
        assert len(stand_in.own) == 4 and all(np.array_equal(a, b) for a, b in zip(stand_in.own, S))
        assert stand_in.passes[-1]['shifts'].shape == (4, 3, 2, 4, 4)
    got, U = function(gates, seqs, np.ones((1, W)), omega, stacked=True, return_propagators=True)
    assert [a.shape for a in got] == [(1, len(s)) + shape for s in seqs]
    assert [u.shape for u in U] == [(len(s), 2, 2) for s in seqs]
    assert all(np.array_equal(a[0], b) for a, b in zip(got, one))
    helper = ff.sequence_prefix_propagators(gates, seqs)
    assert all(np.array_equal(a, b) for a, b in zip(U, helper))
    assert not stand_in.loops
    # every position keeps its place: sequence 2 has three positions, first gate 1
    assert one[2][:, 0, 0, 0].tolist() == [W + 3000 + 10*g + 1 for g in range(3)] and one[1][0, 0, 0, 0] == W + 1000 + 2
    # a subset of the operators, not in sorted order: their indices reach the pass
    S = np.arange(2*2*W, dtype=float).reshape(2, 2, W)
    function(gates, seqs, S, omega, n_oper_identifiers=['Z', 'X'], stacked=True)
    assert stand_in.passes[-1]['idx'] == [1, 0] and np.array_equal(stand_in.passes[-1]['S'], S)
    # closing gates reach the pass as index arrays, negative ones wrapped; the propagators hold them
    got, U = function(gates, seqs, np.ones(W), omega, closing=[[0, -1], [1], [2, 2, -3]], return_propagators=True)
    assert stand_in.passes[-1]['close'] == [[0, 2], [1], [2, 2, 0]]
    helper = ff.sequence_prefix_propagators(gates, seqs, closing=[[0, -1], [1], [2, 2, -3]])
    assert all(np.array_equal(a, b) for a, b in zip(U, helper))
    # (K, n_idx, n_idx, W): cross-spectra, the loop
    got = function(gates, seqs, np.ones((3, 2, 2, W)), omega, stacked=True)
    assert [a.shape for a in got] == [(3, len(s), 1) for s in seqs]
    assert len(stand_in.loops) == 1 and len(stand_in.loops[0]['spectra']) == 3
    # without stacked a two-dimensional spectrum is one spectrum
    assert function(gates, seqs, np.ones((2, W)), omega)[0].shape == (2, 2, 4, 4)
    assert stand_in.passes[-1]['S'].shape == (1, 2, W)


def test_refusals(gates, monkeypatch):
    gates, omega = gates
    stand_in = Passes(monkeypatch)
    W = len(omega)
    for function in (ff.sequence_prefix_frequency_shifts, ff.sequence_prefix_cumulant_functions):
        with pytest.raises(ValueError, match='at least one spectrum'):
            function(gates, [[0]], np.ones((0, W)), omega, stacked=True)                 # K = 0
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
        with pytest.raises(ValueError, match='closing holds 1 arrays for 2 sequences'):
            function(gates, [[0, 1], [1]], np.ones(W), omega, closing=[[0, 1]])
        with pytest.raises(ValueError, match=r'closing\[1\]: expected 1 gate indices'):
            function(gates, [[0, 1], [1]], np.ones(W), omega, closing=[[0, 1], [1, 2]])
        with pytest.raises(IndexError, match=r'^closing\[1\]: index 3 is out of bounds for 3 gates'):
            function(gates, [[1], [0, 1]], np.ones(W), omega, closing=[[0], [0, 3]])
        with pytest.raises(TypeError, match=r'^closing\[0\]: gate indices must be integers'):
            function(gates, [[0, 1]], np.ones(W), omega, closing=[[0.0, 1.0]])
    with pytest.raises(ValueError) as loop_error:
        ff.util.get_indices_from_identifiers(gates[0].n_oper_identifiers, ['Q'])
    with pytest.raises(ValueError) as error:
        ff.sequence_prefix_frequency_shifts(gates, [[0, 1]], np.ones(W), omega, n_oper_identifiers=['Q'])
    assert str(error.value) == str(loop_error.value)
    assert not stand_in.passes and not stand_in.loops


def test_routing(gates, monkeypatch):
    gates, omega = gates
    W = len(omega)
    stand_in = Passes(monkeypatch)

    def refuse(*args, **kwargs):
        raise AssertionError('a pass ran')
    monkeypatch.setattr(sp2, '_run_pass', refuse)
    three = [ff.PulseSequence([[np.diag([1.0, 0.0, -1.0]), [0.3], 'Z']], [[np.diag([1.0, -1.0, 0.0]), [1.0], 'N']],
                              [1.0]) for _ in range(2)]
    for g in three:
        g.cache_control_matrix(omega, np.zeros((1, 9, W), dtype=complex))
    other_basis = cached(gate(noise=('X', 'Z')), omega)
    other_basis.basis = ff.Basis(np.asarray(gates[0].basis)[[0, 2, 1, 3]])
    mismatched = [gates[0], cached(gate(noise=('X',)), omega)]
    no_total = [gates[0], cached(gate(noise=('X', 'Z')), omega)]
    del no_total[1]._data['total_propagator']
    five = ('IX', 'IZ', 'XI', 'ZI', 'ZZ')
    cases = [(gates, np.ones((2, 2, W))),                      # a cross-spectrum
             (gates, np.ones(W)*(1 + 1j)),                     # weights with an imaginary part
             (three, np.ones(W)),                              # d = 3
             ([gates[0], other_basis], np.ones(W)),            # gates of two bases
             (mismatched, np.ones(W)),                         # other noise operators on one gate
             (no_total, np.ones(W)),                           # a gate that does not know its total propagator
             ([cached(two_qubit(five), omega)]*2, np.ones(W))]  # five noise operators
    function = ff.sequence_prefix_frequency_shifts
    for n, (gate_set, S) in enumerate(cases):
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
    assert not stand_in.own                                    # the loop's route asks for no gate's own shifts
    # the same gate set under real weights takes the pass (complex dtype, no imaginary part: still the pass)
    for S in (np.ones(W), np.ones((2, W)), np.ones(W) + 0j):
        with pytest.raises(AssertionError, match='a pass ran'):
            function(gates, [[0, 1]], S, omega)
    # two-qubit gates, Pauli and default basis
    pauli2 = ff.Basis.pauli(2)
    for q in ([cached(two_qubit(('IX', 'XI'), basis=pauli2), omega) for _ in range(2)],
              [cached(two_qubit(('IX', 'XI')), omega) for _ in range(2)]):
        with pytest.raises(AssertionError, match='a pass ran'):
            function(q, [[0, 1]], np.ones((3, W)), omega, stacked=True)


def test_passes_are_split_under_the_budget_and_results_keep_their_place(gates, monkeypatch):
    gates, omega = gates
    W = len(omega)
    stand_in = Passes(monkeypatch)
    seqs = [[k % 3]*(1 + k) for k in range(11)]
    closing = [[(k + g) % 3 for g in range(1 + k)] for k in range(11)]
    S = np.arange(1.0, 4.0)[:, None]*np.ones(W)
    whole = ff.sequence_prefix_frequency_shifts(gates, seqs, S, omega, closing=closing, stacked=True)
    assert len(stand_in.passes) == 1
    # a budget of the tables, 20 positions and their sequences takes the sequences of 1 ... 5 gates (15 positions),
    # then 6 + 7, 8 + 9, 10 and 11
    per_position = sp2.pass_bytes(2, 2, W, 2, 3, True)
    monkeypatch.setattr(sp2, 'PASS_BYTES', sp2.table_bytes(3, 2, 2, W, 2, 3, 1) + 20*per_position + 5*sp2.sequence_bytes(2))
    stand_in.passes.clear()
    split = ff.sequence_prefix_frequency_shifts(gates, seqs, S, omega, closing=closing, stacked=True)
    assert [len(p['indices']) for p in stand_in.passes] == [5, 2, 2, 1, 1]
    assert sum((p['indices'] for p in stand_in.passes), []) == seqs
    assert sum((p['close'] for p in stand_in.passes), []) == closing
    assert all(p['shifts'].shape == (3, 3, 2, 4, 4) for p in stand_in.passes)
    assert all(np.array_equal(a, b) for a, b in zip(split, whole))
    assert [whole[j][k, g, 0, 0, 0] for k in range(3) for j in (0, 10) for g in (0, j)] == [
        (k + 1)*W + 1000*(j + 1) + 10*g + j % 3 for k in range(3) for j in (0, 10) for g in (0, j)]


def test_not_finite_curves_run_the_loops_expression(gates, monkeypatch):
    gates, omega = gates
    W = len(omega)
    # spectrum 2 of the sequence of two positions, spectra 1 and 3 of the one of three
    stand_in = Passes(monkeypatch, not_finite={(2, 2), (1, 3), (3, 3)})
    calls = []

    def single(pulse, spectrum, omega, identifiers):
        calls.append((pulse, float(np.asarray(spectrum).flat[0]), identifiers))
        return np.full((1, 4, 4), -7.0)
    monkeypatch.setattr(sp2, '_single', single)
    monkeypatch.setattr(sp2, '_concatenated', lambda gates, sequence, closer, omega: (sequence.tolist(), closer))
    S = np.arange(1.0, 4.0)[:, None]*np.ones(W)
    got = ff.sequence_prefix_frequency_shifts(gates, [[0], [1, 2], [2, 2, 0]], S, omega, n_oper_identifiers=['Z'],
                                              closing=[[1], [0, 0], [1, 2, 0]], stacked=True)
    # the whole curve of the (spectrum, sequence) is recomputed, every truncation with its closing gate
    assert calls == [(([1], 0), 2.0, ['Z']), (([1, 2], 0), 2.0, ['Z']),
                     (([2], 1), 1.0, ['Z']), (([2, 2], 2), 1.0, ['Z']), (([2, 2, 0], 0), 1.0, ['Z']),
                     (([2], 1), 3.0, ['Z']), (([2, 2], 2), 3.0, ['Z']), (([2, 2, 0], 0), 3.0, ['Z'])]
    assert (got[0] > 0).all()
    assert (got[1][1] == -7.0).all() and (got[1][[0, 2]] > 0).all()
    assert (got[2][[0, 2]] == -7.0).all() and (got[2][1] > 0).all()
    assert not stand_in.loops


# ---- the cumulant functions: a host composition -------------------------------------------------------------------------
class HostCumulants:
    """Stands in for the two batched cumulant entries of the library (which run on the device): the documented formulas
    on the host (oracle/ff_oracle.py), through the entries' own signatures."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _array(address, shape, dtype=np.float64):
        n = int(np.prod(shape))*np.dtype(dtype).itemsize
        return np.frombuffer((ctypes.c_char*n).from_address(address), dtype=dtype).reshape(shape)

    def ffk_cumulant_function(self, gamma, batch, N, d, basis, single_qubit, out):
        self.calls.append(('first', batch, single_qubit))
        C = self._array(basis, (N, d, d), complex)
        self._array(out, (batch, N, N))[:] = orc.cumulant_function_dense(self._array(gamma, (batch, N, N)), C,
                                                                         bool(single_qubit))
        return 0

    def ffk_cumulant_function_second_order(self, delta, batch, N, d, basis, inout):
        self.calls.append(('second', batch))
        C = self._array(basis, (N, d, d), complex)
        self._array(inout, (batch, N, N))[:] += orc.cumulant_second_order_dense(self._array(delta, (batch, N, N)), C)
        return 0


@pytest.mark.parametrize('d', [2, 4])
def test_cumulant_functions_compose_the_two_prefix_calls(d, monkeypatch):
    omega = np.linspace(0.1, 1.0, 5)
    if d == 2:
        gates = [cached(gate(noise=('X', 'Z')), omega) for _ in range(3)]
    else:
        gates = [cached(two_qubit(('IX', 'XI'), basis=ff.Basis.pauli(2)), omega) for _ in range(3)]
    N = d*d
    seqs = [[0, 1], [2], [1, 1, 0]]
    closing = [[1, 1], [0], [2, 0, 1]]
    asked = []

    def stand_in(kind):
        def call(gates_, sequences, spectrum, omega_, n_oper_identifiers=None, closing=None, diagonal=False,
                 stacked=False, return_propagators=False):
            asked.append((kind, [list(s) for s in sequences], closing, stacked, return_propagators))
            lead = (len(spectrum),) if stacked else ()
            local = np.random.default_rng(len(kind))
            values = [local.standard_normal(lead + (len(s), 2, N, N)) for s in sequences]
            if kind == 'gamma':
                values = [v + v.swapaxes(-1, -2) for v in values]
            if return_propagators:
                return values, [np.ones((len(s), d, d)) for s in sequences]
            return values
        return call
    library = HostCumulants()
    monkeypatch.setattr(sp2, 'sequence_prefix_decay_amplitudes', stand_in('gamma'))
    monkeypatch.setattr(sp2, 'sequence_prefix_frequency_shifts', stand_in('delta'))
    monkeypatch.setattr(sp2._lib, 'load', lambda: library)
    # (a launch that takes five tiles: the chunks cut through the sequences)
    monkeypatch.setattr(sp2, 'MAX_CUMULANTS', 5)
    basis = np.asarray(gates[0].basis)
    single_qubit = int(d == 2)                     # the Pauli basis of one qubit: the flag sequence_processes sets
    S = np.random.default_rng(d).random((3, len(omega)))
    for stacked, spectrum in ((False, S[0]), (True, S)):
        gamma = stand_in('gamma')(gates, seqs, spectrum, omega, stacked=stacked)
        delta = stand_in('delta')(gates, seqs, spectrum, omega, stacked=stacked)
        tiles = sum(g.size for g in gamma)//(N*N)
        chunks = [5]*(tiles//5) + ([tiles % 5] if tiles % 5 else [])
        asked.clear()
        library.calls.clear()
        # first order: no second-order code runs, with the keyword and without it
        first = ff.sequence_prefix_cumulant_functions(gates, seqs, spectrum, omega, closing=closing, stacked=stacked)
        assert [a[0] for a in asked] == ['gamma'] and asked[0][1:] == (seqs, closing, stacked, False)
        assert library.calls == [('first', n, single_qubit) for n in chunks]
        again = ff.sequence_prefix_cumulant_functions(gates, seqs, spectrum, omega, closing=closing, stacked=stacked,
                                                      second_order=False)
        assert [a[0] for a in asked] == ['gamma', 'gamma'] and all(c[0] == 'first' for c in library.calls)
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
        library.calls.clear()
        second, U = ff.sequence_prefix_cumulant_functions(gates, seqs, spectrum, omega, closing=closing,
                                                          stacked=stacked, second_order=True, return_propagators=True)
        assert [a[0] for a in asked[2:]] == ['gamma', 'delta'] and asked[2][4] is True and asked[3][4] is False
        assert asked[3][1:4] == (seqs, closing, stacked)
        # one second-order call per chunk, behind the chunk's first-order call
        assert library.calls == sum(([('first', n, single_qubit), ('second', n)] for n in chunks), [])
        assert [u.shape for u in U] == [(len(s), d, d) for s in seqs]
        for p, s in enumerate(seqs):
            assert first[p].shape == second[p].shape == gamma[p].shape and first[p].dtype == np.float64
            want = orc.cumulant_function_dense(gamma[p], basis, bool(single_qubit))
            assert np.array_equal(first[p], want)
            assert np.array_equal(second[p], want + orc.cumulant_second_order_dense(delta[p], basis))
            assert not np.array_equal(first[p], second[p])
    # frequency shifts of another shape than the decay amplitudes: the loop's message
    monkeypatch.setattr(sp2, 'sequence_prefix_frequency_shifts',
                        lambda *args, **kwargs: [np.zeros((len(s), 1, N, N)) for s in seqs])
    with pytest.raises(ValueError, match='Frequency shifts not same shape as decay amplitudes'):
        ff.sequence_prefix_cumulant_functions(gates, seqs, S[0], omega, second_order=True)


def test_cumulant_functions_of_gates_of_several_bases_run_the_loops_expression(gates, monkeypatch):
    gates, omega = gates
    other = cached(gate(noise=('X', 'Z')), omega)
    other.basis = ff.Basis(np.asarray(gates[0].basis)[[0, 2, 1, 3]])
    calls = []

    def refuse(*args, **kwargs):
        raise AssertionError('a batched call ran')
    monkeypatch.setattr(sp2, 'sequence_prefix_decay_amplitudes', refuse)
    monkeypatch.setattr(sp2, 'sequence_prefix_frequency_shifts', refuse)
    monkeypatch.setattr(sp2, '_concatenated', lambda gates, sequence, closer, omega: (sequence.tolist(), closer))
    monkeypatch.setattr(sp2, '_single_cumulant',
                        lambda pulse, S, omega, names, second_order: calls.append((pulse, second_order)) or np.ones((2, 4, 4)))
    got = ff.sequence_prefix_cumulant_functions([gates[0], other], [[0, 1], [1]], np.ones(len(omega)), omega,
                                                closing=[[1, 0], [0]], second_order=True)
    assert [a.shape for a in got] == [(2, 2, 4, 4), (1, 2, 4, 4)]
    assert calls == [(([0], 1), True), (([0, 1], 0), True), (([1], 0), True)]

"""ff.concatenate_sequences: many gate sequences from one gate set in one pass, against the loop of
ff.concatenate (fresh results, same gates), the golden config-3 fixture, and itself in other batches."""
import copy
import ctypes
import gc
import weakref

import numpy as np
import pytest

import filter_functions_amd as ff
import workloads as wl
from conftest import load_golden, rel_err
from filter_functions_amd import _lib, sequences

pytestmark = pytest.mark.gpu

TIGHT = 2e-13
LONG = 1e-12          # total propagators, and sequences of 500 positions or more (products associated differently)


def loop(seqs, **kw):
    return [ff.concatenate(s, **kw) for s in seqs]


def caches(pulse):
    return sorted(pulse._data), sorted(pulse._frequency_data)


def assert_like_loop(got, ref, omega, n_positions):
    """The batched result equals the loop's: ``==``, cached attributes, control matrix, F, total propagator, tau."""
    bar = LONG if n_positions >= 500 else TIGHT
    assert caches(got) == caches(ref)
    assert got == ref
    assert got.tau == ref.tau
    assert rel_err(got.total_propagator, ref.total_propagator) < LONG
    assert rel_err(got.get_filter_function(omega), ref.get_filter_function(omega)) < bar
    assert rel_err(got.get_control_matrix(omega), ref.get_control_matrix(omega)) < bar
    assert np.array_equal(got.omega, ref.omega)


def draws(lengths, seed, n_gates=24):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, n_gates, m) for m in lengths]


def inverse_of(U, gates):
    """The gate whose total propagator undoes U up to a phase (the example's find_inverse, on the host)."""
    overlaps = [abs(np.trace(g.total_propagator @ U)) for g in gates]
    return gates[int(np.argmax(overlaps))]


@pytest.fixture(scope='module')
def cfg3():
    omega = wl.rb_omega(wl.CONFIG3['W'], wl.CONFIG3['T'])
    _, cliffords = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])
    return omega, np.array(cliffords, dtype=object)


def test_config3_gate_set_against_loop_and_reference(cfg3):
    omega, cliffords = cfg3
    lengths = [1, 2, 3, 5, 63, 64, 65, 151, 152, 500, 1000]
    indices = draws(lengths, 11) + [wl.rb_draw(wl.CONFIG3['n_gates'], wl.CONFIG3['seed'])]
    seqs = [cliffords[i] for i in indices]
    got = ff.concatenate_sequences(seqs)
    ref = loop(seqs)
    assert len(got) == len(seqs)
    for g, r, i in zip(got, ref, indices):
        if len(i) == 1:
            assert isinstance(g, ff.PulseSequence) and g == r and g is not cliffords[i[0]]
            continue
        assert isinstance(g._resident, sequences._SequenceMember)
        assert_like_loop(g, r, omega, len(i))
    gold = load_golden('cfg3_subgrid')
    thousand = got[-1]
    at = gold['omega_index']
    assert rel_err(thousand.total_propagator, gold['total_propagator']) < 1e-11
    assert rel_err(thousand.get_control_matrix(omega)[..., at], gold['control_matrix']) < 1e-10
    assert rel_err(thousand.get_filter_function(omega)[..., at], gold['filter_function']) < 1e-10


def test_study_shape_infidelities_and_inverse():
    omega = wl.rb_omega(301, wl.CONFIG3['T'])
    _, cliffords = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])
    cliffords = np.array(cliffords, dtype=object)
    lengths = np.linspace(1, 151, 21).astype(int)
    seqs = []
    for k, m in enumerate(np.repeat(lengths, 3)):
        draw = np.random.default_rng(100 + k).integers(0, 24, m)
        U = ff.concatenate_without_filter_function(cliffords[draw]).total_propagator
        seqs.append(list(cliffords[draw]) + [inverse_of(U, cliffords)])
    spectra = [wl.rb_spectrum(omega, 0.0), wl.rb_spectrum(omega, 0.7)]
    got = ff.concatenate_sequences(seqs)
    ref = loop(seqs)
    for g, r, s in zip(got, ref, seqs):
        assert_like_loop(g, r, omega, len(s))
        assert abs(abs(np.trace(g.total_propagator)) - 2) < 1e-12          # the inverse closes the sequence
    for S in spectra:
        batched = ff.infidelities(got, S, omega)
        one_by_one = np.array([ff.infidelity(g, S, omega) for g in got])
        looped = np.array([ff.infidelity(r, S, omega) for r in ref])
        assert rel_err(batched, looped) < 1e-13
        assert rel_err(batched, one_by_one) < 1e-14
    # the example's U @ U_inv step: the gates of the second call are results of the first
    firsts = ff.concatenate_sequences([cliffords[np.random.default_rng(500 + k).integers(0, 24, m)]
                                       for k, m in enumerate(lengths)])
    firsts_ref = [ff.concatenate(cliffords[np.random.default_rng(500 + k).integers(0, 24, m)])
                  for k, m in enumerate(lengths)]
    inverses = [inverse_of(U.total_propagator, cliffords) for U in firsts_ref]
    second = ff.concatenate_sequences([[U, V] for U, V in zip(firsts, inverses)])
    second_ref = [U @ V for U, V in zip(firsts_ref, inverses)]
    for g, r, m in zip(second, second_ref, lengths):
        assert isinstance(g._resident, sequences._SequenceMember)
        assert_like_loop(g, r, omega, 2)
    for S in spectra:
        assert rel_err(ff.infidelities(second, S, omega), [ff.infidelity(r, S, omega) for r in second_ref]) < 1e-13


def test_optimized_gate_set():
    g = load_golden('rb_optimized_gates')
    omega = wl.rb_omega(301, wl.CONFIG3['T'])
    gates = {name: (g[f'{name}_eps'], g[f'{name}_t'], g[f'{name}_B']) for name in ('X2', 'Y2')}
    _, cliffords = wl.rb_cliffords_optimized(ff, omega, gates)
    cliffords = np.array(cliffords, dtype=object)
    lengths = [2, 7, 20, 40, 64, 65, 100, 151]
    seqs = [cliffords[i] for i in draws(lengths, 3)]
    for got, ref, m in zip(ff.concatenate_sequences(seqs), loop(seqs), lengths):
        assert_like_loop(got, ref, omega, m)


def random_gate_set(T, noise, omega, seed):
    """T distinct single-segment gates (control on X and Y), every one carrying the noise operators *noise*, control
    matrices cached at omega."""
    rng = np.random.default_rng(seed)
    X, Y = ff.util.paulis[1], ff.util.paulis[2]
    gates = []
    for _ in range(T):
        gate = ff.PulseSequence([[X/2, [rng.normal()], 'X'], [Y/2, [rng.normal()], 'Y']],
                                [[op/2, [1.0], name] for name, op in noise], [1.0 + rng.random()])
        gate.cache_control_matrix(omega)
        gates.append(gate)
    return np.array(gates, dtype=object)


@pytest.mark.parametrize('T, noise', [(24, 'XZ'), (70, 'X')])
def test_tables_that_do_not_fit_lds(T, noise):
    from filter_functions_amd.util import paulis
    ops = {'X': paulis[1], 'Z': paulis[3]}
    omega = wl.rb_omega(300, wl.CONFIG3['T'])
    gates = random_gate_set(T, [(n, ops[n]) for n in noise], omega, seed=T)
    lengths = [2, 9, 64, 130, 200]
    seqs = [gates[i] for i in draws(lengths, T, n_gates=T)]
    for got, ref, m in zip(ff.concatenate_sequences(seqs), loop(seqs), lengths):
        assert_like_loop(got, ref, omega, m)


def test_a_sequence_does_not_depend_on_its_batch():
    omega = wl.rb_omega(301, wl.CONFIG3['T'])
    _, cliffords = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])
    cliffords = np.array(cliffords, dtype=object)
    probe = cliffords[wl.rb_draw(300, 7)]
    others = [cliffords[i] for i in draws(np.random.default_rng(1).integers(2, 400, 199), 9)]
    runs = [ff.concatenate_sequences([probe, others[0]])[0],
            ff.concatenate_sequences([probe] + others)[0],
            ff.concatenate_sequences(others + [probe])[-1]]
    for other in runs[1:]:
        assert np.array_equal(other.get_filter_function(omega), runs[0].get_filter_function(omega))
        assert np.array_equal(other.get_control_matrix(omega), runs[0].get_control_matrix(omega))
        assert np.array_equal(other.total_propagator, runs[0].total_propagator)


def test_mixed_lists_follow_the_loop():
    omega = wl.rb_omega(301, wl.CONFIG3['T'])
    _, cliffords = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])
    cliffords = np.array(cliffords, dtype=object)
    other_grid = wl.rb_omega(200, wl.CONFIG3['T'])
    cliffords_other = np.array(wl.rb_cliffords(ff, other_grid, wl.CONFIG3['T'])[1], dtype=object)
    X, Z = ff.util.paulis[1], ff.util.paulis[3]
    # d = 4 gates (two qubits), control matrices cached
    P4 = [ff.PulseSequence([[np.kron(X, X)/2, [0.3, 0.7]], [np.kron(Z, X)/2, [0.1, -0.2]]],
                           [[np.kron(X, ff.util.paulis[0])/2, [1.0, 1.0]]], [1.0, 2.0]) for _ in range(3)]
    for p in P4:
        p.cache_control_matrix(omega)
    # a gate without the noise operator of the others
    bare = ff.PulseSequence([[X/2, [0.4], 'X']], [[Z/2, [1.0], 'Z']], [1.0])
    bare.cache_control_matrix(omega)
    seqs = [cliffords[[0, 3, 5]], [P4[0], P4[1], P4[2], P4[0]], cliffords_other[[1, 2, 2]], [cliffords[4]],
            list(cliffords[[1, 2]]) + [bare], cliffords[draws([40], 2)[0]], [cliffords_other[6]]]
    got = ff.concatenate_sequences(seqs)
    ref = loop(seqs)
    for k, (g, r) in enumerate(zip(got, ref)):
        w = r.omega
        assert caches(g) == caches(r), k
        assert g == r
        assert rel_err(g.get_filter_function(w), r.get_filter_function(w)) < TIGHT, k
        assert rel_err(g.total_propagator, r.total_propagator) < LONG, k
    assert isinstance(got[0]._resident, sequences._SequenceMember)
    assert isinstance(got[5]._resident, sequences._SequenceMember)
    assert not isinstance(got[1]._resident, sequences._SequenceMember)      # d = 4: the loop
    # the same exception as the loop, raised by the same sequence
    bad = [cliffords[[0, 1]], [cliffords[2], cliffords_other[3]]]
    with pytest.raises(ValueError) as loop_error:
        loop(bad, calc_filter_function=True)
    with pytest.raises(ValueError) as error:
        ff.concatenate_sequences(bad, calc_filter_function=True)
    assert str(error.value) == str(loop_error.value)
    with pytest.raises(TypeError):
        ff.concatenate_sequences([cliffords[[0, 1]], [cliffords[0], 3]])
    # no filter function asked for: the loop's answer
    for g, r in zip(ff.concatenate_sequences(seqs[:1], calc_filter_function=False), loop(seqs[:1],
                                                                                         calc_filter_function=False)):
        assert caches(g) == caches(r) and g == r


def test_caches_copies_and_bad_arguments():
    omega = wl.rb_omega(301, wl.CONFIG3['T'])
    _, cliffords = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])
    cliffords = np.array(cliffords, dtype=object)
    before = [(caches(c), {k: id(c._frequency_data.peek(k)) for k in c._frequency_data}) for c in cliffords]
    results = ff.concatenate_sequences([cliffords[i] for i in draws([30, 31], 5)])
    assert [(caches(c), {k: id(c._frequency_data.peek(k)) for k in c._frequency_data}) for c in cliffords] == before
    result = results[0]
    passed = weakref.ref(result._resident.batch)
    twin = copy.deepcopy(result)
    F = np.array(result.get_filter_function(omega))
    del result, results
    gc.collect()
    assert passed() is None
    assert np.array_equal(twin.get_filter_function(omega), F)
    # a bad index / offsets array through the C entry: FFK_EINVAL (ValueError), the stream stays usable
    lib = _lib.load()
    handle = ctypes.c_void_p()
    assert lib.ffk_resident_create(ctypes.byref(handle)) == 0
    gate = cliffords[0]
    U = np.ascontiguousarray(gate.total_propagator[None], dtype=np.complex128)
    table = np.ascontiguousarray(gate.get_control_matrix(omega)[None])
    tau = np.array([gate.tau])
    basis = np.ascontiguousarray(np.asarray(gate.basis), dtype=np.complex128)
    om = np.ascontiguousarray(omega)
    gates = (ctypes.c_void_p*1)(None)
    slots = np.array([-1], dtype=np.int32)
    total = np.empty((2, 2, 2), dtype=np.complex128)
    F_ptr = ctypes.c_void_p()

    def call(offsets, index):
        offsets = np.asarray(offsets, dtype=np.int32)
        index = np.asarray(index, dtype=np.int32)
        return lib.ffk_concatenate_sequences_resident(
            handle, gates, slots.ctypes.data, table.ctypes.data, U.ctypes.data, tau.ctypes.data, 1,
            offsets.ctypes.data, index.ctypes.data, len(offsets) - 1, om.ctypes.data, len(om), basis.ctypes.data, 1, 2,
            1, 4, None, 0, 0, None, 0, 0, total.ctypes.data, ctypes.byref(F_ptr), None)
    try:
        assert call([0, 2, 3], [0, 1, 0]) == _lib.FFK_EINVAL
        assert 'index' in lib.ffk_last_error().decode()
        assert call([0, 2, 1], [0, 0, 0]) == _lib.FFK_EINVAL
        assert call([1, 2, 3], [0, 0, 0]) == _lib.FFK_EINVAL
        assert call([0, 2, 3], [0, 0, 0]) == 0
        assert rel_err(total[1], gate.total_propagator) < 1e-15
    finally:
        lib.ffk_resident_destroy(handle)
    again = ff.concatenate_sequences([cliffords[[0, 1, 2]]])[0]
    assert rel_err(again.get_filter_function(omega), ff.concatenate(cliffords[[0, 1, 2]]).get_filter_function(omega)) \
        < TIGHT

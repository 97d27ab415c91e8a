"""ff.correlation_infidelities: the pulse-correlation infidelities I[g, h, a] of many gate sequences in one pass,
against the existing path -- ff.concatenate(..., calc_pulse_correlation_FF=True)'s summands, contracted and integrated
here in extended precision --, against the literal loop over ff.infidelity(..., which='correlations'), and against
itself in other batches.

The bar: by Cauchy-Schwarz every entry's rounding error is bounded by a multiple of eps times the largest diagonal
entry, which is the max-norm of the reference when the weights are non-negative; the summands of the two paths differ
by the association of at most 256 phase and propagator products.  TIGHT is test_sequences_gpu.py's value for
sequences under 500 positions."""
import copy
import ctypes

import numpy as np
import pytest

import filter_functions_amd as ff
import workloads as wl
from conftest import rel_err
from filter_functions_amd import _lib, correlations

pytestmark = pytest.mark.gpu

TIGHT = 2e-13
LENGTHS = [2, 3, 15, 16, 17, 31, 33, 64, 65, 151, 255, 256]
T = wl.CONFIG3['T']


def trapezoid_weights(omega):
    """The weights of util.integrate, in extended precision."""
    steps = np.diff(np.asarray(omega, dtype=np.longdouble))
    w = np.zeros(len(omega), dtype=np.longdouble)
    w[:-1] += steps/2
    w[1:] += steps/2
    return w


def yardstick(seq, S, omega, names=None, absolute=False):
    """(G, G, n_idx) from the existing path's summands, in np.longdouble:
    einsum('gako,ao,hako->gha', conj(R_pc)[:, idx], S w, R_pc[:, idx]).real / (2 pi d), as one real product per operator;
    *absolute*: with |S w| (the scale of a spectrum that changes sign)."""
    pulse = ff.concatenate(seq, calc_pulse_correlation_FF=True, omega=omega)
    R = pulse.get_pulse_correlation_control_matrix()
    R = R[:, ff.util.get_indices_from_identifiers(pulse.n_oper_identifiers, names)]
    G, n_idx = R.shape[:2]
    weights = np.broadcast_to(np.asarray(S, dtype=np.longdouble), (n_idx, len(omega)))*trapezoid_weights(omega)
    if absolute:
        weights = np.abs(weights)
    out = np.empty((G, G, n_idx), dtype=np.longdouble)
    for a in range(n_idx):
        Z = np.concatenate([R[:, a].real, R[:, a].imag], axis=1).astype(np.longdouble)      # (G, 2 N, W)
        out[:, :, a] = (Z*weights[a]).reshape(G, -1) @ Z.reshape(G, -1).T
    return out/(2*np.pi*np.longdouble(pulse.d))


def draws(lengths, seed, n_gates):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, n_gates, m) for m in lengths]


NOISE = {'X': ff.util.paulis[1]/2, 'Y': ff.util.paulis[2]/2, 'Z': ff.util.paulis[3]/2,
         'D': (ff.util.paulis[1] + ff.util.paulis[3])/np.sqrt(8)}


def random_gates(n, noise, omega, seed):
    """One-segment gates (control on X and Y, random amplitudes and durations) carrying the noise operators *noise*
    (as test_sequences_host.py's gate(noise=...)), control matrices cached at *omega*."""
    rng = np.random.default_rng(seed)
    X, Y = ff.util.paulis[1], ff.util.paulis[2]
    gates = []
    for _ in range(n):
        g = ff.PulseSequence([[X/2, [rng.normal()], 'X'], [Y/2, [rng.normal()], 'Y']],
                             [[NOISE[name], [0.5 + rng.random()], name] for name in noise], [1.0 + rng.random()])
        g.cache_control_matrix(omega)
        gates.append(g)
    return np.array(gates, dtype=object)


@pytest.fixture(scope='module')
def study():
    """The study's gate set at W = 301 and one batch of every length (and one gate 40 times), evaluated once."""
    omega = wl.rb_omega(301, T)
    cliffords = np.array(wl.rb_cliffords(ff, omega, T)[1], dtype=object)
    seqs = [cliffords[i] for i in draws(LENGTHS, 21, 24)] + [[cliffords[7]]*40]
    S = wl.rb_spectrum(omega)
    return omega, cliffords, seqs, S, ff.correlation_infidelities(seqs, S, omega)


@pytest.mark.parametrize('k', range(len(LENGTHS) + 1))
def test_lengths_at_the_study_grid(study, k):
    omega, _, seqs, S, got = study
    G = len(seqs[k])
    assert got[k].shape == (G, G, 1) and got[k].dtype == np.float64
    err = rel_err(got[k], yardstick(seqs[k], S, omega))
    print(f'G = {G}: rel_err {err:.2e}')
    assert err < TIGHT


@pytest.mark.parametrize('noise, names, two_dim, extra', [('X', None, False, [257]), ('XZ', ['Z', 'X'], True, []),
                                                           ('XYZ', ['Z', 'X'], False, []),
                                                           ('XYZD', ['Z', 'D', 'X'], True, []),
                                                           ('XYZD', None, True, [])])
def test_lengths_operators_and_spectra_at_seven_frequencies(noise, names, two_dim, extra):
    """Every length, A = 1 ... 4, a subset of the operators in non-sorted order, spectra of one and two dimensions; the
    batch also holds a sequence of one gate and (once: its loop makes 257^2 library calls) one of 257 gates, which
    follow the loop."""
    omega = np.geomspace(1e-2, 30.0, 7)
    gates = random_gates(9, noise, omega, seed=len(noise))
    single = ff.concatenate(gates[[0, 1]], calc_pulse_correlation_FF=True, omega=omega)      # (the loop's answer: its own)
    seqs = [gates[i] for i in draws(LENGTHS + extra, 5, 9)] + [[single]]
    n_idx = len(noise) if names is None else len(names)
    rng = np.random.default_rng(3)
    S = rng.random((n_idx, 7)) + 0.1 if two_dim else 1/omega
    got = ff.correlation_infidelities(seqs, S, omega, n_oper_identifiers=names)
    assert len(got) == len(seqs)
    worst = 0.0
    for seq, result in zip(seqs[:-1], got):
        assert result.shape == (len(seq), len(seq), n_idx)
        worst = max(worst, rel_err(result, yardstick(seq, S, omega, names)))
    print(f'A = {len(noise)}: worst rel_err {worst:.2e}')
    assert worst < TIGHT
    assert np.array_equal(got[-1], ff.infidelity(single, S, omega, n_oper_identifiers=names, which='correlations'))


def test_two_frequencies_and_fewer():
    omega = np.array([0.3, 1.1])
    gates = random_gates(5, 'XZ', omega, seed=8)
    seqs = [gates[i] for i in draws(LENGTHS, 6, 5)]
    S = np.array([[2.0, 0.5], [0.25, 3.0]])
    got = ff.correlation_infidelities(seqs, S, omega)
    assert max(rel_err(g, yardstick(s, S, omega)) for g, s in zip(got, seqs)) < TIGHT
    one = np.array([0.7])
    lonely = random_gates(2, 'X', one, seed=9)
    zeros = ff.correlation_infidelities([lonely[[0, 1, 0]]], [1.0], one)[0]
    assert zeros.shape == (3, 3, 1) and not zeros.any()                 # W < 2 gives zeros, as elsewhere


def test_a_spectrum_that_changes_sign(study):
    omega, cliffords, seqs, _, _ = study
    S = wl.rb_spectrum(omega)*np.cos(np.arange(len(omega)))
    picks = [seqs[1], seqs[6], seqs[9]]
    got = ff.correlation_infidelities(picks, S, omega)
    for seq, result in zip(picks, got):
        scale = np.max(np.abs(yardstick(seq, S, omega, absolute=True)))
        err = float(np.max(np.abs(result - yardstick(seq, S, omega)))/scale)
        print(f'G = {len(seq)}: error over the absolute scale {err:.2e}')
        assert err < TIGHT


def test_the_batched_route_is_really_taken(study, monkeypatch):
    omega, cliffords, seqs, S, got = study
    d4 = ff.PulseSequence([[np.kron(NOISE['X'], NOISE['X'])*2, [0.3]]], [[np.kron(NOISE['X'], np.eye(2)), [1.0]]], [1.0])
    d4.cache_control_matrix(omega)
    long = cliffords[draws([257], 1, 24)[0]]

    def refuse(*args, **kwargs):
        raise AssertionError('the loop ran')
    monkeypatch.setattr(ff, 'concatenate', refuse)
    again = ff.correlation_infidelities(seqs, S, omega)
    assert all(np.array_equal(a, b) for a, b in zip(again, got))
    for ineligible in ([d4, d4], long, [cliffords[3]]):
        with pytest.raises(AssertionError, match='the loop ran'):
            ff.correlation_infidelities([seqs[0], ineligible], S, omega)
    with pytest.raises(AssertionError, match='the loop ran'):
        ff.correlation_infidelities(seqs[:2], np.ones((1, 1, len(omega))), omega)      # cross-spectra


def loop(seqs, S, omega=None, names=None):
    out = []
    for s in seqs:
        pulse = ff.concatenate(s, calc_pulse_correlation_FF=True, omega=omega)
        out.append(ff.infidelity(pulse, S, pulse.omega, n_oper_identifiers=names, which='correlations'))
    return out


def test_literal_loop_equality():
    omega = wl.rb_omega(40, T)
    gates = random_gates(6, 'XZ', omega, seed=2)
    seqs = [gates[i] for i in draws([2, 3, 4, 5], 4, 6)]
    rng = np.random.default_rng(12)
    C = rng.random((2, 2, 40)) + 1j*rng.random((2, 2, 40))
    cross = C + C.conj().swapaxes(0, 1)
    for S, names in ((1/omega, None), (rng.random((2, 40)), None), (1/omega, ['Z']), (cross, None),
                     (cross[:1, :1], ['X'])):
        got = ff.correlation_infidelities(seqs, S, names and omega, n_oper_identifiers=names)
        for g, r in zip(got, loop(seqs, S, names and omega, names)):
            assert g.shape == r.shape
            assert rel_err(g, r) < 1e-13
    # a gate lacking an operator, gates on different grids: still the loop's numbers
    bare = ff.PulseSequence([[NOISE['X'], [0.4], 'X']], [[NOISE['Z'], [1.0], 'Z']], [1.0])
    bare.cache_control_matrix(omega)
    X, Y = ff.util.paulis[1], ff.util.paulis[2]
    unit = [ff.PulseSequence([[X/2, [0.2 + 0.3*k], 'X'], [Y/2, [0.1*k], 'Y']],
                             [[NOISE['X'], [1.0], 'X'], [NOISE['Z'], [1.0], 'Z']], [1.0 + 0.1*k]) for k in range(3)]
    for g in unit:
        g.cache_control_matrix(omega)
    mixed = [[unit[1], unit[2], bare], gates[[0, 5, 3]], [unit[0], bare, unit[0], unit[2]]]
    for g, r in zip(ff.correlation_infidelities(mixed, 1/omega, omega), loop(mixed, 1/omega, omega)):
        assert g.shape == r.shape and rel_err(g, r) < 1e-13
    other = random_gates(2, 'XZ', wl.rb_omega(30, T), seed=5)
    bad = [gates[[0, 1]], [gates[2], other[0]]]
    for kwargs in (dict(), dict(n_oper_identifiers=['Q'])):
        with pytest.raises(ValueError) as loop_error:
            loop(bad if not kwargs else seqs, 1/omega, None, kwargs.get('n_oper_identifiers'))
        with pytest.raises(ValueError) as error:
            ff.correlation_infidelities(bad if not kwargs else seqs, 1/omega, **kwargs)
        assert str(error.value) == str(loop_error.value)
    # a wrong omega: gates recomputed on it by the loop, and a spectrum that does not fit the grid
    wrong = wl.rb_omega(12, T)
    for g, r in zip(ff.correlation_infidelities(seqs[:2], 1/wrong, wrong), loop(seqs[:2], 1/wrong, wrong)):
        assert rel_err(g, r) < 1e-13
    for g in gates:
        g.cache_control_matrix(omega)
    with pytest.raises(ValueError) as loop_error:
        loop(seqs, np.ones(7), omega)
    with pytest.raises(ValueError) as error:
        ff.correlation_infidelities(seqs, np.ones(7), omega)
    assert str(error.value) == str(loop_error.value)
    assert ff.correlation_infidelities([], 1/omega) == []


def test_invariants(study):
    omega, cliffords, seqs, S, got = study
    totals = ff.infidelities(ff.concatenate_sequences(seqs), S, omega)
    for result, total in zip(got, totals):
        assert rel_err(result.sum(axis=(0, 1)), total) < 1e-12
        assert np.array_equal(result, result.swapaxes(0, 1))
    probe = seqs[9]
    others = [cliffords[i] for i in draws(np.random.default_rng(1).integers(2, 60, 39), 9, 24)]
    alone = ff.correlation_infidelities([probe], S, omega)[0]
    assert np.array_equal(alone, got[9])
    assert np.array_equal(ff.correlation_infidelities([probe] + others, S, omega)[0], alone)
    assert np.array_equal(ff.correlation_infidelities(others + [probe], S, omega)[-1], alone)


def test_resident_gates_and_host_gates_agree():
    omega = wl.rb_omega(301, T)
    rng = np.random.default_rng(17)
    X, Y = ff.util.paulis[1], ff.util.paulis[2]

    def fresh():
        r = np.random.default_rng(4)
        return [ff.PulseSequence([[X/2, r.normal(size=3), 'X'], [Y/2, r.normal(size=3), 'Y']],
                                 [[NOISE['X'], [1.0]*3, 'X'], [NOISE['Z'], [0.7]*3, 'Z']], 1.0 + r.random(3))
                for _ in range(6)]
    resident, host = fresh(), fresh()
    ff.get_filter_functions(resident, omega)                     # members of a batched pass: read in HBM
    for g in host:
        g.cache_control_matrix(omega)
    host = [copy.deepcopy(g) for g in host]                      # (a copy keeps the arrays and drops the HBM result)
    from filter_functions_amd.sequences import _gate_source
    assert all(_gate_source(g, 301, 2) is not None for g in resident)
    assert all(_gate_source(g, 301, 2) is None for g in host)
    index = [rng.integers(0, 6, m) for m in (2, 17, 70)]
    S = wl.rb_spectrum(omega)
    a = ff.correlation_infidelities([[resident[i] for i in ix] for ix in index], S, omega)
    b = ff.correlation_infidelities([[host[i] for i in ix] for ix in index], S, omega)
    mixed = ff.correlation_infidelities([[(resident if n % 2 else host)[i] for n, i in enumerate(ix)] for ix in index],
                                        S, omega)
    for x, y, z, ix in zip(a, b, mixed, index):
        assert rel_err(x, y) < TIGHT and rel_err(z, y) < TIGHT
        assert rel_err(y, yardstick([host[i] for i in ix], S, omega)) < TIGHT


def test_c_entry_refuses_bad_arguments():
    omega = wl.rb_omega(301, T)
    gate = wl.rb_cliffords(ff, omega, T)[1][0]
    lib = _lib.load()
    U = np.ascontiguousarray(gate.total_propagator[None], dtype=np.complex128)
    table = np.ascontiguousarray(gate.get_control_matrix(omega)[None])
    tau = np.array([gate.tau])
    basis = np.ascontiguousarray(np.asarray(gate.basis), dtype=np.complex128)
    om = np.ascontiguousarray(omega)
    S = np.ascontiguousarray(wl.rb_spectrum(omega))
    gates = (ctypes.c_void_p*1)(None)
    slots = np.array([-1], dtype=np.int32)
    idx = np.zeros(1, dtype=np.int32)

    def call(offsets, index, s_ndim=1, out_offsets=None):
        offsets = np.asarray(offsets, dtype=np.int32)
        index = np.asarray(index, dtype=np.int32)
        if out_offsets is None:
            out_offsets = correlations.output_offsets(np.abs(np.diff(offsets)))
        out_offsets = np.asarray(out_offsets, dtype=np.int64)
        out = np.full((max(int(out_offsets[-1]), 1), 1), np.nan)
        rc = lib.ffk_sequence_correlation_infidelities(
            gates, slots.ctypes.data, table.ctypes.data, U.ctypes.data, tau.ctypes.data, 1, offsets.ctypes.data,
            index.ctypes.data, len(offsets) - 1, om.ctypes.data, len(om), basis.ctypes.data, 1, 2, 1, 4, S.ctypes.data,
            s_ndim, 1, idx.ctypes.data, 1, 2, out_offsets.ctypes.data, out.ctypes.data)
        return rc, out
    assert call([0, 2, 3], [0, 1, 0])[0] == _lib.FFK_EINVAL
    assert 'index' in lib.ffk_last_error().decode()
    assert call([0, 2, 1], [0, 0, 0])[0] == _lib.FFK_EINVAL
    assert call([1, 2, 3], [0, 0, 0])[0] == _lib.FFK_EINVAL
    assert call([0, 257], [0]*257)[0] == _lib.FFK_EINVAL
    assert call([0, 2, 3], [0, 0, 0], s_ndim=3)[0] == _lib.FFK_EINVAL
    assert call([0, 2, 3], [0, 0, 0], out_offsets=[0, 4, 6])[0] == _lib.FFK_EINVAL
    rc, out = call([0, 2, 3], [0, 0, 0])
    assert rc == 0
    want = ff.correlation_infidelities([[gate, gate], [gate]*2], S, omega)[0]
    assert np.array_equal(out[:4].reshape(2, 2, 1), want)
    assert rel_err(out[4, 0], yardstick([gate, gate], S, omega)[0, 0, 0]) < TIGHT       # a sequence of one gate

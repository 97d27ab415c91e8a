"""ff.periodic_frequency_shifts / periodic_cumulant_functions / periodic_error_transfer_matrices on the GPU against the
loop over ff.concatenate([p]*n, calc_second_order_FF=True), against the sequential yardstick of
periodic_shift_yardstick.py (n - 1 steps of one period, in the operator basis, in extended precision where NumPy has
it) and against the walk of ff.sequence_frequency_shifts.

Pulses and grid are those of test_periodic_gpu.py (copied): d = 2 (a generic rotation, an exact 2 pi rotation, a pi
rotation; 4 segments, two noise operators), d = 4 in the Pauli basis (a generic pulse and one with a two-fold
degenerate eigenphase; 3 segments, three noise operators), d = 3 in the GGM basis; W = 33 frequencies with 0, 1e-10
and the two resonances of the first qubit pulse on the grid.

Same bits.  The pass is a function of a pulse's control matrix, eigensystem, its own frequency shifts Delta_1 and the
steps of the count alone.  Delta_1 comes from ff.frequency_shifts, which routes a group of one and a pulse with a
cached second-order filter function through the single function and everything else through its batched pass -- two
routes whose bits may differ.  The comparisons of a pulse alone and among others, and of resident against uploaded
control matrices, therefore hold Delta_1 fixed (ff.frequency_shifts replaced by a table of its own earlier rows);
without that the two agree within the parity bar, which is asserted as well.

Measured on MI355X, max |got - ref| / max |ref| per pulse and count:
    against the loop, n in {1, 2, 3, 7}:   d = 2: 7.4e-17 .. 2.0e-15;  d = 4: 1.3e-16 .. 4.9e-15;  d = 3: 0 .. 2.0e-15
    n = 1000 against the yardstick in np.longdouble:   d = 2: 1.4e-13, 2.9e-13, 1.7e-13;  d = 4: 4.3e-13, 5.0e-13;
        d = 3: 2.5e-13   (the loop itself: 1.5e-13, 1.8e-13, 2.9e-13;  2.4e-14, 6.4e-14;  1.3e-13)
    n = 1000 against the walk of ff.sequence_frequency_shifts:   d = 2: 1.6e-13, 3.4e-13, 2.3e-13;  d = 4: 4.6e-13,
        4.9e-13
    error transfer matrices, second order: max |got - loop| = 2.2e-16, the second-order term moves them by 0.115
(DESIGN.md section 7.16).
"""
import ctypes

import numpy as np
import pytest

import filter_functions_amd as ff
import periodic_shift_yardstick as shift_yard
from conftest import rel_err
from filter_functions_amd import _lib, batch, batch_second_order, numeric, periodic
from filter_functions_amd import periodic_second_order as pso
from filter_functions_amd._resident import Deferred
from filter_functions_amd.sequence_prefix_second_order import _cumulants

pytestmark = pytest.mark.gpu

REPEATS = [1, 2, 3, 7]
PAULI = np.array([[[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]], dtype=complex)
BAR = 1e-10          # the project's parity contract


def herm(rng, d):
    m = rng.normal(size=(d, d)) + 1j*rng.normal(size=(d, d))
    return m + m.conj().T


def qubit_pulses():
    """[generic, 2 pi about x, pi about x]: 4 segments, noise on z and y."""
    rng = np.random.default_rng(100)
    dt = np.array([0.3, 0.2, 0.4, 0.1])
    noise = [[PAULI[2], rng.uniform(0.5, 1.5, 4)], [PAULI[1], rng.uniform(0.5, 1.5, 4)]]
    basis = ff.Basis.pauli(1)
    generic = ff.PulseSequence([[PAULI[0], rng.normal(size=4)], [PAULI[1], rng.normal(size=4)]], noise, dt, basis)
    shape = np.array([1.0, 2.0, 0.5, 1.5])
    made = [generic]
    for angle in (2*np.pi, np.pi):
        amplitude = shape*angle/(shape*dt).sum()          # sum a_g dt_g = angle, H = a sigma_x / 2
        made.append(ff.PulseSequence([[PAULI[0]/2, amplitude]], noise, dt, basis))
    return made


def two_qubit_pulses():
    rng = np.random.default_rng(101)
    dt = np.array([0.5, 0.25, 0.75])
    basis = ff.Basis.pauli(2)
    noise = [[herm(rng, 4), rng.uniform(0.5, 1.5, 3)] for _ in range(3)]
    generic = ff.PulseSequence([[herm(rng, 4), rng.normal(size=3)], [herm(rng, 4), rng.normal(size=3)]], noise, dt,
                               basis)
    q, r = np.linalg.qr(rng.normal(size=(4, 4)) + 1j*rng.normal(size=(4, 4)))
    frame = q*(np.diag(r)/np.abs(np.diag(r)))
    H = (frame*(-np.array([0.3, 0.3, 1.1, -2.0])/dt.sum())) @ frame.conj().T
    degenerate = ff.PulseSequence([[(H + H.conj().T)/2, np.ones(3)]], noise, dt, basis)
    return [generic, degenerate]


def qutrit_pulses():
    rng = np.random.default_rng(102)
    noise = [[herm(rng, 3), rng.uniform(0.5, 1.5, 3)] for _ in range(2)]
    return [ff.PulseSequence([[herm(rng, 3), rng.normal(size=3)]], noise, np.array([0.4, 0.3, 0.6]), ff.Basis.ggm(3))]


MAKERS = {2: qubit_pulses, 4: two_qubit_pulses, 3: qutrit_pulses}


def grid():
    """33 frequencies: 0, 1e-10, the two resonances of the first qubit pulse (w T <= 2 pi), 29 more up to w T = 50."""
    first = qubit_pulses()[0]
    first.diagonalize()
    _, phi, _ = periodic.eigensystem(first.total_propagator)
    T = first.tau
    resonances = [np.mod(phi[0] - phi[1], 2*np.pi)/T, np.mod(phi[1] - phi[0], 2*np.pi)/T]
    rest = np.geomspace(1e-3, 50.0/T, 29)
    omega = np.sort(np.concatenate([[0.0, 1e-10], resonances, rest]))
    assert len(omega) == 33 and all(r in omega for r in resonances)
    return omega


def spectrum_of(omega):
    return 1.0/(1.0 + omega**2) + 0.1


def loop_shifts(pulses, repeats, S, omega, identifiers=None):
    """The loop of the documentation."""
    return np.stack([np.stack([numeric.calculate_frequency_shifts(
        ff.concatenate([p]*n, calc_second_order_FF=True, omega=omega), S, omega, identifiers) for n in repeats])
        for p in pulses])


@pytest.fixture(scope='module')
def study():
    omega = grid()
    S = spectrum_of(omega)
    ref = {d: loop_shifts(make(), REPEATS, S, omega) for d, make in MAKERS.items()}
    for values in ref.values():
        values.flags.writeable = False
    return omega, S, ref


def hold_first_order(monkeypatch, rows):
    """ff.frequency_shifts as the pass reads it, replaced by the table *rows* {id(pulse): Delta_1}."""
    def held(pulses, spectrum, omega, n_oper_identifiers=None):
        return np.stack([rows[id(p)] for p in pulses])
    monkeypatch.setattr(batch_second_order, 'frequency_shifts', held)


@pytest.mark.parametrize('d', [2, 4, 3])
def test_against_the_loop(study, d):
    omega, S, ref = study
    pulses = MAKERS[d]()
    got = ff.periodic_frequency_shifts(pulses, REPEATS, S, omega)
    assert got.shape == ref[d].shape and got.dtype == np.float64
    for p in range(len(pulses)):
        for k, n in enumerate(REPEATS):
            print(d, p, n, rel_err(got[p, k], ref[d][p, k]))
            assert rel_err(got[p, k], ref[d][p, k]) < BAR, (p, n)
    # the frequency shifts are not symmetric, and not n times those of one period
    assert not np.array_equal(got, got.swapaxes(-1, -2))
    assert rel_err(7*got[:, 0], got[:, 3]) > 1e-3
    # row n = 1 is the pulses' row of ff.frequency_shifts, bit for bit
    assert np.array_equal(got[:, 0], ff.frequency_shifts(MAKERS[d](), S, omega))
    # deferred cache entries stay deferred, and batched members of ff.frequency_shifts end without filter_function_2
    if len(pulses) > 1:
        assert all(type(p._frequency_data.peek('control_matrix')) is Deferred for p in pulses)
        assert not any(p.is_cached('filter_function_2') for p in pulses)


def yardstick_rows(pulses, omega, S, delta1, n):
    rows = []
    for pulse, first in zip(pulses, delta1):
        R1 = np.array(pulse.get_control_matrix(omega))
        rows.append(shift_yard.sequential_frequency_shifts(R1, np.asarray(pulse.basis), pulse.total_propagator,
                                                           pulse.tau, omega, S, first, [n],
                                                           extended=shift_yard.EXTENDED)[n])
    return np.stack(rows)


@pytest.mark.parametrize('d', [2, 4, 3])
def test_against_the_sequential_yardstick_at_1000_periods(study, d):
    """999 steps of one period against ten of the doubling, from the same control matrix, propagator and Delta_1."""
    omega, S, _ = study
    pulses = MAKERS[d]()
    got = ff.periodic_frequency_shifts(pulses, [1, 1000], S, omega)
    want = yardstick_rows(pulses, omega, S, got[:, 0], 1000)
    for p in range(len(pulses)):
        print(f'd = {d} pulse {p} n = 1000: {rel_err(got[p, 1], want[p]):.3e} (extended: {shift_yard.EXTENDED})')
        assert rel_err(got[p, 1], want[p]) < BAR, p


@pytest.mark.parametrize('d', [2, 4])
def test_against_the_walk_of_sequence_frequency_shifts_at_1000_periods(study, d):
    omega, S, _ = study
    pulses = MAKERS[d]()
    got = ff.periodic_frequency_shifts(pulses, [1000], S, omega)
    for p, twin in enumerate(MAKERS[d]()):
        want = ff.sequence_frequency_shifts([twin], [np.zeros(1000, dtype=int)], S, omega)[0]
        print(f'd = {d} pulse {p} n = 1000 against the walk: {rel_err(got[p, 0], want):.3e}')
        assert rel_err(got[p, 0], want) < BAR, p


def ragged_pulses(d, A, count=2):
    rng = np.random.default_rng(200 + 10*d + A)
    G = 3
    basis = ff.Basis.pauli(d//2)
    made = []
    for _ in range(count):
        noise = [[herm(rng, d), rng.uniform(0.5, 1.5, G), f'N{a}'] for a in range(A)]
        made.append(ff.PulseSequence([[herm(rng, d), rng.normal(size=G)]], noise, rng.uniform(0.2, 0.6, G), basis))
    return made


@pytest.mark.parametrize('W', [7, 64, 65])
@pytest.mark.parametrize('d', [2, 4])
def test_ragged_shapes(d, W):
    """The 64-frequency step boundary, one to four noise operators, a subset of them in non-sorted order, a spectrum
    of two dimensions."""
    repeats = [1, 2, 5, 12]
    omega = np.concatenate([[0.0], np.geomspace(1e-2, 30.0, W - 1)])
    for A in (1, 2, 3, 4):
        identifiers = [f'N{a}' for a in range(A)][::-1][:max(1, A - 1)]          # e.g. A = 4: N3, N2, N1
        n_idx = len(identifiers)
        S = np.stack([(1.0 + 0.5*a)/(1.0 + omega**2) + 0.1 for a in range(n_idx)])
        got = ff.periodic_frequency_shifts(ragged_pulses(d, A), repeats, S, omega, identifiers)
        want = loop_shifts(ragged_pulses(d, A), repeats, S, omega, identifiers)
        assert got.shape == want.shape == (2, 4, n_idx, d*d, d*d)
        for p in range(2):
            for k, n in enumerate(repeats):
                assert rel_err(got[p, k], want[p, k]) < BAR, (A, p, n, rel_err(got[p, k], want[p, k]))


@pytest.mark.parametrize('d', [2, 4])
def test_same_bits_alone_among_others_anywhere_resident_or_uploaded(study, d, monkeypatch):
    omega, S, _ = study
    pulses = MAKERS[d]()
    repeats = REPEATS + [1000]
    whole = ff.periodic_frequency_shifts(pulses, repeats, S, omega)
    assert all(type(p._frequency_data.peek('control_matrix')) is Deferred for p in pulses)
    # among others in another order, at any place in repeats and whatever else is in it
    assert np.array_equal(ff.periodic_frequency_shifts(pulses[::-1], repeats, S, omega), whole[::-1])
    order = [4, 0, 3, 1, 2, 4]
    assert np.array_equal(ff.periodic_frequency_shifts(pulses, [repeats[k] for k in order], S, omega), whole[:, order])
    other = ff.periodic_frequency_shifts(pulses, [999, 7, 13, 1000], S, omega)
    assert np.array_equal(other[:, 1], whole[:, 3]) and np.array_equal(other[:, 3], whole[:, 4])
    # alone, on ff.frequency_shifts' own route for a group of one: within the bar
    for i in range(len(pulses)):
        assert rel_err(ff.periodic_frequency_shifts([MAKERS[d]()[i]], repeats, S, omega)[0], whole[i]) < BAR
    # from here on Delta_1 is held fixed
    rows = {id(p): whole[i, 0] for i, p in enumerate(pulses)}
    hold_first_order(monkeypatch, rows)
    for i in range(len(pulses)):
        assert np.array_equal(ff.periodic_frequency_shifts([pulses[i]], repeats, S, omega)[0], whole[i])
    # uploaded: twins that hold the same control matrices as host arrays
    twins = MAKERS[d]()
    for i, (twin, pulse) in enumerate(zip(twins, pulses)):
        twin.total_propagator = pulse.total_propagator
        twin.cache_control_matrix(omega, np.array(pulse.get_control_matrix(omega)))
        rows[id(twin)] = whole[i, 0]
    assert np.array_equal(ff.periodic_frequency_shifts([twins[0]] + pulses[1:], repeats, S, omega), whole)
    # in any pass split: a budget of one member and a bit
    monkeypatch.setattr(batch, 'PASS_BYTES', 4096)
    assert np.array_equal(ff.periodic_frequency_shifts(twins, repeats, S, omega), whole)


def test_an_ineligible_pulse_and_a_cross_spectrum(study):
    """d = 8 (more than 16 basis elements) and a cross-spectrum: the fallback's values, which are the loop's.  The
    output shape (n_idx, N, N) ties N = d^2 to the dimension, so a d = 8 pulse and a qubit pulse cannot share a call:
    that is the ValueError of every batched call here (the next test mixes within one dimension)."""
    omega, S, _ = study
    rng = np.random.default_rng(103)
    noise = [[herm(rng, 8), np.ones(2)], [herm(rng, 8), np.ones(2)]]
    big = lambda: ff.PulseSequence([[herm(np.random.default_rng(7), 8), np.array([0.3, -0.2])]], noise,   # noqa: E731
                                   np.array([0.5, 0.7]), ff.Basis.pauli(3))
    with pytest.raises(ValueError, match='same output shape'):
        ff.periodic_frequency_shifts(qubit_pulses() + [big()], [1, 3], S, omega)
    got = ff.periodic_frequency_shifts([big()], [1, 3], S, omega)
    assert got.shape == (1, 2, 2, 64, 64)
    assert rel_err(got[0], loop_shifts([big()], [1, 3], S, omega)[0]) < BAR
    cross = np.stack([[S, 0.1*S], [0.1*S, S]])
    got = ff.periodic_frequency_shifts(qubit_pulses()[:2], [2, 5], cross, omega)
    assert got.shape == (2, 2, 2, 2, 4, 4)
    want = loop_shifts(qubit_pulses()[:2], [2, 5], cross, omega)
    assert rel_err(got, want) < BAR


def test_an_ineligible_pulse_in_the_same_call(study):
    """One call that mixes eligible pulses with an ineligible one of the same output shape: a qubit pulse with five
    noise operators (the kernels take four) evaluates the fallback between two that take the pass."""
    omega, S, _ = study
    dt = np.array([0.3, 0.2, 0.4, 0.1])

    def five():
        r = np.random.default_rng(105)
        noise = [[herm(r, 2), r.uniform(0.5, 1.5, 4), f'N{a}'] for a in range(5)]
        return ff.PulseSequence([[PAULI[0], r.normal(size=4)]], noise, dt, ff.Basis.pauli(1))

    def two():
        r = np.random.default_rng(106)
        noise = [[herm(r, 2), r.uniform(0.5, 1.5, 4), f'N{a}'] for a in range(2)]
        return ff.PulseSequence([[PAULI[1], r.normal(size=4)]], noise, dt, ff.Basis.pauli(1))
    assert not periodic._eligible(five()) and periodic._eligible(two())
    identifiers = ['N1', 'N0']
    got = ff.periodic_frequency_shifts([two(), five(), two()], [1, 2, 5], S, omega, identifiers)
    want = loop_shifts([two(), five()], [1, 2, 5], S, omega, identifiers)
    assert got.shape == (3, 3, 2, 4, 4)
    assert rel_err(got[1], want[1]) < BAR and rel_err(got[0], want[0]) < BAR and np.array_equal(got[0], got[2])


def test_device_pointer_entry_gives_the_same_bits(study):
    """ffk_periodic_shifts_dev on device arrays (ffk_malloc / ffk_memcpy_*): launches only, the bits of the
    host-pointer entry."""
    lib = _lib.load()
    omega, S, _ = study
    pulses = qubit_pulses()
    repeats = [1, 7, 12, 2]
    want = ff.periodic_frequency_shifts(pulses, repeats, S, omega)
    steps, count_slots = pso.step_plan(repeats)
    P, K, W, d, A, n_steps = len(pulses), len(repeats), len(omega), 2, 2, len(steps)
    systems = [periodic.eigensystem(p.total_propagator) for p in pulses]
    owned, kept = [], []          # (the host arrays stay alive until the copies have run)

    def alloc(nbytes):
        ptr = ctypes.c_void_p()
        _lib.check(lib.ffk_malloc(ctypes.byref(ptr), nbytes))
        owned.append(ptr)
        return ptr

    def up(a, dtype=np.float64):
        a = np.ascontiguousarray(a, dtype=dtype)
        ptr = alloc(a.nbytes)
        kept.append(a)
        _lib.check(lib.ffk_memcpy_h2d(ptr, a.ctypes.data, a.nbytes, None))
        return ptr
    try:
        R = [up(np.array(p.get_control_matrix(omega)), np.complex128) for p in pulses]
        table = up([r.value for r in R], np.uint64)
        V = up(np.stack([s[0] for s in systems]), np.complex128)
        dphi = up(np.stack([periodic.phase_differences(p.total_propagator, s[0]) for p, s in zip(pulses, systems)]))
        T = up([p.tau for p in pulses])
        basis, grid_d, spectrum = up(np.asarray(pulses[0].basis), np.complex128), up(omega), up(S, np.complex128)
        plan, slots, idx = up(steps, np.int32), up(count_slots, np.int32), up(np.arange(A), np.int32)
        delta1 = up(want[:, 0])
        tile = 8*P*A*d**4
        need = 3*256 + 16*W + tile*(2*n_steps + 1)
        workspace, out = alloc(need), alloc(want.nbytes)
        _lib.check(lib.ffk_device_synchronize())
        _lib.check(lib.ffk_periodic_shifts_dev(table, P, A, W, d, grid_d, basis, V, dphi, T, plan, n_steps, slots, K,
                                               spectrum, 1, idx, A, delta1, out, workspace, need, None))
        got = np.empty_like(want)
        _lib.check(lib.ffk_memcpy_d2h(got.ctypes.data, out, got.nbytes, None))
        _lib.check(lib.ffk_device_synchronize())
    finally:
        for ptr in owned:
            lib.ffk_free(ptr)
    assert np.array_equal(got, want)


def test_cumulant_functions_and_error_transfer_matrices(study):
    omega, S, _ = study
    repeats = [1, 2, 7]
    for d in (2, 4):
        for second_order in (False, True):
            got = ff.periodic_cumulant_functions(MAKERS[d](), repeats, S, omega, second_order=second_order)
            want = np.stack([np.stack([numeric.calculate_cumulant_function(
                ff.concatenate([p]*n, calc_second_order_FF=second_order, omega=omega), S, omega,
                second_order=second_order) for n in repeats]) for p in MAKERS[d]()])
            assert got.shape == want.shape
            for p in range(len(want)):
                for k, n in enumerate(repeats):
                    assert rel_err(got[p, k], want[p, k]) < BAR, (d, second_order, p, n)
        # second_order=False: the bits of the cumulant entry on ff.periodic_decay_amplitudes
        pulses = MAKERS[d]()
        first = ff.periodic_cumulant_functions(pulses, repeats, S, omega)
        gamma = ff.periodic_decay_amplitudes(pulses, repeats, S, omega)
        N = d*d
        assert np.array_equal(first, _cumulants(gamma.reshape(-1, N, N), None, pulses[0].basis).reshape(gamma.shape))
    # error transfer matrices: entries of order one, 1e-10 absolute; the second-order term must matter
    S_weak = 0.05*S
    pulses = qubit_pulses()
    got = ff.periodic_error_transfer_matrices(pulses, repeats, S_weak, omega, second_order=True)
    without = ff.periodic_error_transfer_matrices(pulses, repeats, S_weak, omega)
    want = np.stack([np.stack([ff.error_transfer_matrix(
        ff.concatenate([p]*n, calc_second_order_FF=True, omega=omega), S_weak, omega, second_order=True)
        for n in repeats]) for p in qubit_pulses()])
    assert got.shape == want.shape == (3, 3, 4, 4)
    print('error transfer matrices: max |got - loop| =', np.abs(got - want).max(), ' second order moves them by',
          np.abs(got - without).max())
    assert np.abs(got - without).max() > 1e-4
    assert np.abs(got - want).max() < 1e-10

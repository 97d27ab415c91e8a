"""ff.periodic_filter_functions / periodic_infidelities / periodic_decay_amplitudes on the GPU against the double loop
over ff.concatenate_periodic, and both against the 60-digit series of periodic_yardstick.py.

Shapes: d = 2 (a generic rotation, an exact 2 pi rotation -- all phases degenerate --, a pi rotation; 4 segments, two
noise operators), d = 4 in the Pauli basis (a generic pulse and one whose propagator has the phases 0.3, 0.3, 1.1,
-2.0 in a random frame; 3 segments, three noise operators), d = 3 in the GGM basis.  W = 33 frequencies (a tail in
every tile width) with 0, 1e-10 and the two resonances ((phi_j - phi_k) mod 2 pi)/T of the first pulse on the grid.

Extended precision, d = 2, F of n periods against the series summed term by term (max |F - exact| / max |exact| per
pulse and repeat count; measured on MI355X, loop = the doubling route of ff.concatenate_periodic), new call / loop:
    generic rotation   n <= 7: 3.6e-16 .. 6.1e-16 / 1.2e-16 .. 7.2e-16     n = 1000: 4.0e-14 / 1.5e-13
    2 pi rotation      n <= 7: 2.5e-16 .. 1.3e-15 / 9.9e-17 .. 1.3e-15     n = 1000: 1.1e-13 / 2.2e-13
    pi rotation        n <= 7: 2.0e-16 .. 7.1e-16 / 2.4e-16 .. 8.0e-16     n = 1000: 2.5e-16 / 2.8e-13
(DESIGN.md section 7.15).
"""
import numpy as np
import pytest

import filter_functions_amd as ff
import periodic_yardstick as yard
from conftest import rel_err
from filter_functions_amd import batch, numeric, periodic
from filter_functions_amd._resident import Deferred

pytestmark = pytest.mark.gpu

REPEATS = [1, 2, 3, 7, 1000]
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


def loop_results(pulses, omega, S):
    """The double loop, on pulses with the control matrix cached (the doubling route)."""
    F, I, G = [], [], []
    for p in pulses:
        p.cache_control_matrix(omega)
        rows = [ff.concatenate_periodic(p, n) for n in REPEATS]
        F.append(np.stack([np.einsum('aaw->aw', r.get_filter_function(omega)).real for r in rows]))
        I.append(np.stack([ff.infidelity(r, S, omega) for r in rows]))
        G.append(np.stack([numeric.calculate_decay_amplitudes(r, S, omega) for r in rows]))
    return np.stack(F), np.stack(I), np.stack(G)


@pytest.fixture(scope='module')
def study():
    omega = grid()
    S = spectrum_of(omega)
    ref = {d: loop_results(make(), omega, S) for d, make in MAKERS.items()}
    for values in ref.values():
        for v in values:
            v.flags.writeable = False
    return omega, S, ref


def batched(pulses, omega, S, repeats=REPEATS):
    return (ff.periodic_filter_functions(pulses, repeats, omega), ff.periodic_infidelities(pulses, repeats, S, omega),
            ff.periodic_decay_amplitudes(pulses, repeats, S, omega))


@pytest.mark.parametrize('d', [2, 4, 3])
def test_against_the_loop(study, d):
    omega, S, ref = study
    pulses = MAKERS[d]()
    got = batched(pulses, omega, S)
    for name, g, r in zip(('F', 'infidelity', 'decay'), got, ref[d]):
        assert g.shape == r.shape and g.dtype == np.float64
        for p in range(len(pulses)):
            for k, n in enumerate(REPEATS):
                print(d, name, p, n, rel_err(g[p, k], r[p, k]))
                assert rel_err(g[p, k], r[p, k]) < BAR, (name, p, n)
    # decay amplitudes: symmetric bit for bit
    assert np.array_equal(got[2], got[2].swapaxes(-1, -2))
    # row n = 1 is the pulses themselves
    fresh = MAKERS[d]()
    assert rel_err(got[1][:, 0], ff.infidelities(fresh, S, omega)) < BAR
    assert rel_err(got[2][:, 0], ff.decay_amplitudes(fresh, S, omega)) < BAR
    # the pulses went through ONE ff.get_filter_functions call: their control matrices are still in HBM
    if len(pulses) > 1:
        assert all(type(p._frequency_data.peek('control_matrix')) is Deferred for p in pulses)


@pytest.mark.parametrize('d', [2, 4])
def test_same_bits_alone_among_others_anywhere_resident_or_uploaded(study, d, monkeypatch):
    omega, S, _ = study
    pulses = MAKERS[d]()
    whole = batched(pulses, omega, S)
    assert all(type(p._frequency_data.peek('control_matrix')) is Deferred for p in pulses)
    # alone, and in another order among others
    for i in range(len(pulses)):
        for a, b in zip(batched([pulses[i]], omega, S), whole):
            assert np.array_equal(a[0], b[i])
    for a, b in zip(batched(pulses[::-1], omega, S), whole):
        assert np.array_equal(a, b[::-1])
    # at any place in repeats
    order = [4, 0, 3, 1, 2, 4]
    for a, b in zip(batched(pulses, omega, S, [REPEATS[k] for k in order]), whole):
        assert np.array_equal(a, b[:, order])
    assert all(type(p._frequency_data.peek('control_matrix')) is Deferred for p in pulses)
    # uploaded: twins that hold the same control matrices as host arrays
    twins = MAKERS[d]()
    for twin, pulse in zip(twins, pulses):
        twin.total_propagator = pulse.total_propagator
        twin.cache_control_matrix(omega, np.array(pulse.get_control_matrix(omega)))
    mixed = [twins[0]] + pulses[1:]
    for a, b in zip(batched(mixed, omega, S), whole):
        assert np.array_equal(a, b)
    # in any pass split: a budget of one member and a bit
    monkeypatch.setattr(batch, 'PASS_BYTES', 4096)
    for a, b in zip(batched(twins, omega, S), whole):
        assert np.array_equal(a, b)


def test_an_ineligible_pulse_in_the_same_call(study):
    """d = 8 (more than 16 basis elements) among qubit pulses, and a cross-spectrum: the loop's values."""
    omega, S, ref = study
    rng = np.random.default_rng(103)
    noise = [[herm(rng, 8), np.ones(2)], [herm(rng, 8), np.ones(2)]]
    big = lambda: ff.PulseSequence([[herm(np.random.default_rng(7), 8), np.array([0.3, -0.2])]], noise,   # noqa: E731
                                   np.array([0.5, 0.7]), ff.Basis.pauli(3))
    repeats = [1, 3]
    got = ff.periodic_infidelities(qubit_pulses() + [big()], repeats, S, omega)
    assert got.shape == (4, 2, 2)
    twin = big()
    twin.cache_control_matrix(omega)
    loop = np.stack([ff.infidelity(ff.concatenate_periodic(twin, n), S, omega) for n in repeats])
    assert rel_err(got[3], loop) < BAR
    assert rel_err(got[:3, 1], ref[2][1][:, 2]) < BAR
    cross = np.stack([[S, 0.1*S], [0.1*S, S]])
    pulses = qubit_pulses()[:2]
    got = ff.periodic_decay_amplitudes(pulses, [2], cross, omega)
    assert got.shape == (2, 1, 2, 2, 4, 4)
    for p, twin in enumerate(qubit_pulses()[:2]):
        twin.cache_control_matrix(omega)
        want = numeric.calculate_decay_amplitudes(ff.concatenate_periodic(twin, 2), cross, omega)
        assert rel_err(got[p, 0], want) < BAR


def test_extended_precision(study):
    """d = 2, n <= 1000: F of the new call and of the loop against the series summed term by term at 60 digits from
    the same control matrix, the same fl(w T) and the exact matrix powers of the same propagator.  The new call's
    error must not exceed four times the loop's (the factor allows for the other order of the sums; both routes
    share the n eps w T sensitivity of the phase)."""
    omega, S, ref = study
    pulses = qubit_pulses()
    new = ff.periodic_filter_functions(pulses, REPEATS, omega)
    for p, pulse in enumerate(pulses):
        R1 = np.array(pulse.get_control_matrix(omega))
        exact = yard.series_control_matrices_mp(R1, np.asarray(pulse.basis), pulse.total_propagator, pulse.tau, omega,
                                                REPEATS)
        err_new, err_loop = [], []
        for k, n in enumerate(REPEATS):
            F = yard.filter_function_of(exact[n])
            err_new.append(rel_err(new[p, k], F))
            # (the loop on the very same control matrix, so that both errors are errors of the periodic sum alone)
            loop = np.einsum('aaw->aw', ff.concatenate_periodic(pulse, n).get_filter_function(omega)).real
            err_loop.append(rel_err(loop, F))
            print(f'pulse {p} n {n}: new {err_new[-1]:.3e} loop {err_loop[-1]:.3e}')
        assert max(err_new) <= 4*max(err_loop), (p, err_new, err_loop)


@pytest.mark.parametrize('stage', [1, 2, 3])
def test_device_pointer_entry_gives_the_same_bits(study, stage):
    """ffk_periodic_dev on device arrays (ffk_malloc / ffk_memcpy_*): launches only, the bits of the host-pointer
    entry."""
    import ctypes

    from filter_functions_amd import _lib
    lib = _lib.load()
    omega, S, _ = study
    pulses = qubit_pulses()
    want = batched(pulses, omega, S)[stage - 1]
    P, K, W, d, A = len(pulses), len(REPEATS), len(omega), 2, 2
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
        repeats, idx = up(REPEATS, np.int32), up(np.arange(A), np.int32)
        workspace, out = alloc(16*W + 256), alloc(want.nbytes)
        _lib.check(lib.ffk_device_synchronize())
        _lib.check(lib.ffk_periodic_dev(table, P, A, W, d, grid_d, basis, V, dphi, T, repeats, K, spectrum, 1, idx, A, d,
                                        stage, out, workspace, 16*W + 256, None))
        got = np.empty_like(want)
        _lib.check(lib.ffk_memcpy_d2h(got.ctypes.data, out, got.nbytes, None))
        _lib.check(lib.ffk_device_synchronize())
    finally:
        for ptr in owned:
            lib.ffk_free(ptr)
    assert np.array_equal(got, want)

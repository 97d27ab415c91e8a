"""ff.sequence_decay_amplitudes, ff.sequence_cumulant_functions, ff.sequence_error_transfer_matrices: the processes of
many gate sequences given as index arrays into one gate set, against the concatenation rule and the spectral integral
run on the host in extended precision from the same inputs (the Yardstick of test_sequence_infidelities_gpu.py,
extended by Gamma = sum_w trapezoid(w) Re(conj R_k S R_l) / 2 pi), against the loop over ff.concatenate and the single
functions, and against itself in other passes (bit for bit)."""
import numpy as np
import pytest

import filter_functions_amd as ff
import workloads as wl
from conftest import rel_err
from filter_functions_amd import numeric
from filter_functions_amd import sequence_processes as sp
from filter_functions_amd.sequences import resident_source
from test_sequence_infidelities_gpu import CLD, LD, LONG, NAMES, TIGHT, Yardstick, draws, two_qubit_gates

pytestmark = pytest.mark.gpu

BAR = 1e-12           # cumulant functions and error transfer matrices against the loop (tests/test_processes_gpu.py)
LENGTHS = [1, 2, 3, 63, 64, 65, 130]


def gamma_yardstick(yard, R, S, idx):
    """Gamma (n_idx, N, N) in long double from R (A, N, W) of Yardstick.sequence and real weights S (W,) or
    (n_idx, W)."""
    S = np.broadcast_to(np.asarray(S, dtype=np.float64), (len(idx), len(yard.omega))).astype(LD)
    picked = R[np.asarray(idx)]
    f = (picked[:, :, None, :].conj()*S[:, None, None, :]*picked[:, None, :, :]).real
    x = yard.omega.astype(LD)
    pi = 4*np.arctan(LD(1))
    return ((f[..., 1:] + f[..., :-1])*np.diff(x)).sum(axis=-1)/2/(2*pi)


def pulses_of(gates, seqs, omega):
    table = np.asarray(gates, dtype=object)
    return [ff.concatenate(table[s], omega=omega) for s in seqs]


def loop(function, pulses, S, omega, names=None):
    return np.stack([function(p, S, omega, names) for p in pulses])


def real_spectra(n_idx, omega, seed):
    """Spectra of one and of two dimensions."""
    return [wl.rb_spectrum(omega, 0.7), 0.5 + np.random.default_rng(seed).random((n_idx, len(omega)))]


WORST = {'new': 0.0, 'loop': 0.0}


def check_against_yardstick_and_loop(gates, seqs, omega, names, seed):
    """Every sequence, spectra of one and two dimensions, every (sequence, operator) tile: the new call against the
    yardstick under the project's bars and within twice the loop's own error; the total propagators; the symmetry."""
    yard = Yardstick(gates, omega)
    idx = ff.util.get_indices_from_identifiers(gates[0].n_oper_identifiers, names)
    N = len(gates[0].basis)
    refs = [yard.sequence([int(k) % len(gates) for k in s]) for s in seqs]
    bars = [LONG if len(s) >= 500 else TIGHT for s in seqs]
    pulses = pulses_of(gates, seqs, omega)
    for S in real_spectra(len(idx), omega, seed):
        got, U = ff.sequence_decay_amplitudes(gates, seqs, S, omega, n_oper_identifiers=names,
                                              return_propagators=True)
        looped = loop(numeric.calculate_decay_amplitudes, pulses, S, omega, names)
        assert got.shape == looped.shape == (len(seqs), len(idx), N, N) and got.dtype == np.float64
        assert np.array_equal(got, got.swapaxes(-1, -2))
        for j, (R_ref, _, U_ref) in enumerate(refs):
            ref = gamma_yardstick(yard, R_ref, S, idx)
            for a in range(len(idx)):
                new, old = rel_err(got[j, a], ref[a]), rel_err(looped[j, a], ref[a])
                print(f'd={yard.d} W={len(omega)} A={len(gates[0].n_opers)} T={len(gates)} G={len(seqs[j])} '
                      f'S.ndim={np.ndim(S)} operator {a}: Gamma new {new:.2e} loop {old:.2e}')
                WORST.update(new=max(WORST['new'], new), loop=max(WORST['loop'], old))
                assert new < bars[j], (j, a, new)
                assert new <= max(2e-13, 2*old), (j, a, new, old)
            assert rel_err(U[j], U_ref) < bars[j], j
    print(f'worst so far: new {WORST["new"]:.2e}, loop {WORST["loop"]:.2e}')


# ---- accuracy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W, A, T, pauli', [(7, 1, 3, True), (64, 2, 3, False), (65, 3, 3, True), (70, 4, 3, False),
                                            (33, 2, 3, True), (70, 1, 40, False), (65, 2, 40, True),
                                            (33, 3, 40, False), (7, 4, 40, True), (64, 4, 40, False)])
def test_two_qubit_gates_against_extended_precision(W, A, T, pauli):
    """T = 3: the tables staged in LDS; T = 40: read from L2.  W: a partial tile of 16 frequencies, a partial block of
    either width, a full block, one frequency past it, a partial second block."""
    omega = wl.rb_omega(W, 1.0, m_max=3)
    gates = two_qubit_gates(T, A, omega, seed=10*W + A, basis=ff.Basis.pauli(2) if pauli else ff.Basis.ggm(4))
    assert len(gates[0].basis) == 16 and gates[0].d == 4
    seqs = draws(LENGTHS, W + T, T)
    seqs[2] = np.array([-1, 0, -T])                       # negative indices wrap
    names = None if A == 1 else [NAMES[A - 1], NAMES[0]]    # a subset, not in sorted order
    check_against_yardstick_and_loop(gates, seqs, omega, names, seed=W)


def test_five_hundred_two_qubit_gates():
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(40, 1, omega, seed=5)
    check_against_yardstick_and_loop(gates, draws([500], 1, 40), omega, None, seed=2)


def single_qubit_gates(T, A, omega, seed):
    """T random single-qubit gates of one and two segments carrying A noise operators (identifiers in sorted order)."""
    rng = np.random.default_rng(seed)
    X, Y, Z = ff.util.paulis[1:]
    noise = [('A', X/2), ('B', Y/2), ('C', Z/2), ('D', (X + Z)/np.sqrt(8))][:A]
    gates = []
    for k in range(T):
        G = 1 + k % 2
        gate = ff.PulseSequence([[X/2, rng.normal(size=G), 'X'], [Y/2, rng.normal(size=G), 'Y']],
                                [[op, 0.5 + rng.random(G), name] for name, op in noise], 1.0 + rng.random(G))
        gate.cache_control_matrix(omega)
        gates.append(gate)
    return gates


@pytest.mark.parametrize('W, A, T', [(301, 1, 24), (7, 2, 8), (64, 3, 8), (65, 4, 8), (65, 4, 24)])
def test_single_qubit_gates_against_extended_precision(W, A, T):
    """A = 1: the Clifford gate set; tables staged in LDS (sixteen wavefronts, eight at A = 4) and, the last, in L2."""
    if A == 1:
        omega = wl.rb_omega(W, wl.CONFIG3['T'])
        gates = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])[1]
    else:
        omega = wl.rb_omega(W, 1.0, m_max=3)
        gates = single_qubit_gates(T, A, omega, seed=W + A)
    names = None if A == 1 else ['B', 'A']
    check_against_yardstick_and_loop(gates, draws([1, 2, 3, 64, 65, 152], W, T), omega, names, seed=A)


# ---- bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d, A, T', [(4, 1, 3), (4, 2, 40), (4, 4, 3), (2, 1, 24), (2, 4, 24)])
def test_a_sequence_does_not_depend_on_its_pass_or_the_split(d, A, T, monkeypatch):
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(T, A, omega, seed=A) if d == 4 else single_qubit_gates(T, A, omega, seed=A)
    S = real_spectra(A, omega, 4)[1]
    probe = draws([77], 8, T)[0]
    others = draws(np.random.default_rng(1).integers(1, 140, 39), 9, T)
    for function in (ff.sequence_decay_amplitudes, ff.sequence_error_transfer_matrices):
        alone = function(gates, [probe], S, omega, return_propagators=True)
        first = function(gates, [probe] + others, S, omega, return_propagators=True)
        last = function(gates, others + [probe], S, omega, return_propagators=True)
        for a, f, l in zip(alone, first, last):
            assert np.array_equal(a[0], f[0]) and np.array_equal(a[0], l[-1])
        # several passes: a budget of the tables and seven sequences
        with monkeypatch.context() as patch:
            longest = max(len(s) for s in [probe] + others)
            patch.setattr(sp, 'PASS_BYTES',
                          sp.table_bytes(T, d, A, 70, A, 1, 2) + 7*sp.pass_bytes(longest, d, A, 70, A, 1))
            calls = []
            run_pass = sp._run_pass
            patch.setattr(sp, '_run_pass', lambda *args: calls.append(len(args[1])) or run_pass(*args))
            split = function(gates, others + [probe], S, omega, return_propagators=True)
        assert len(calls) >= 6 and max(calls) <= 7, calls
        for whole, part in zip(last, split):
            assert np.array_equal(whole, part)


@pytest.mark.parametrize('d', [2, 4])
def test_stacked_spectra_give_the_bits_of_single_calls(d):
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(3, 3, omega, seed=3) if d == 4 else single_qubit_gates(5, 3, omega, seed=3)
    names = [gates[0].n_oper_identifiers[2], gates[0].n_oper_identifiers[0]]
    seqs = draws([1, 5, 64, 100], 7, len(gates))
    rng = np.random.default_rng(0)
    for S in (np.stack([wl.rb_spectrum(omega, alpha) for alpha in (0.0, 0.7, 1.5)]), rng.random((3, 2, 70))):
        for function in (ff.sequence_decay_amplitudes, ff.sequence_cumulant_functions,
                         ff.sequence_error_transfer_matrices):
            stacked, U = function(gates, seqs, S, omega, n_oper_identifiers=names, stacked=True,
                                  return_propagators=True)
            assert stacked.shape[:2] == (3, 4)
            for k in range(3):
                single, U_single = function(gates, seqs, S[k], omega, n_oper_identifiers=names,
                                            return_propagators=True)
                assert np.array_equal(stacked[k], single) and np.array_equal(U, U_single)


def test_resident_gates_and_host_arrays_give_the_same_bits():
    omega = wl.rb_omega(70, 1.0, m_max=3)
    S = real_spectra(2, omega, 1)[1]
    seqs = draws([1, 2, 17, 64, 100], 6, 4)
    single = two_qubit_gates(4, 2, omega, seed=3)                     # cache_control_matrix: single resident results
    assert all(resident_source(g, 4, 70, 16, 2)[1] == -1 for g in single)
    got = ff.sequence_decay_amplitudes(single, seqs, S, omega, return_propagators=True)
    host = [ff.PulseSequence(list(zip(g.c_opers, g.c_coeffs, g.c_oper_identifiers)),
                             list(zip(g.n_opers, g.n_coeffs, g.n_oper_identifiers)), g.dt) for g in single]
    for h, g in zip(host, single):
        h.cache_control_matrix(omega, np.array(g.get_control_matrix(omega)))
        h.total_propagator = np.array(g.total_propagator)
        assert resident_source(h, 4, 70, 16, 2) is None
    # every row uploaded, and a mixed table
    for table in (host, [single[0], host[1], single[2], host[3]]):
        for a, b in zip(got, ff.sequence_decay_amplitudes(table, seqs, S, omega, return_propagators=True)):
            assert np.array_equal(a, b)


def test_single_qubit_tables_in_lds_and_in_l2_give_the_same_bits():
    """The 24 Cliffords alone are staged in LDS; in a pass whose sequences use 70 gates the tables are read from L2."""
    omega = wl.rb_omega(70, wl.CONFIG3['T'])
    X, Y = ff.util.paulis[1], ff.util.paulis[2]
    rng = np.random.default_rng(2)
    gates = list(wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])[1])
    for _ in range(46):
        extra = ff.PulseSequence([[X/2, [rng.normal()], 'X'], [Y/2, [rng.normal()], 'Y']], [[X/2, [1], 'X']],
                                 [1.0 + rng.random()])
        extra.cache_control_matrix(omega)
        gates.append(extra)
    assert sp.eligibility(gates) is not None
    S = wl.rb_spectrum(omega, 0.7)
    probes = draws([1, 30, 152], 3, 24)
    staged = ff.sequence_decay_amplitudes(gates, probes, S, omega)
    among = ff.sequence_decay_amplitudes(gates, probes + [np.arange(70)], S, omega)
    assert np.array_equal(staged, among[:3])


# ---- later stages ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d, pauli', [(2, True), (4, True), (4, False)])
def test_cumulant_functions_and_error_transfer_matrices_against_the_loop(d, pauli):
    omega = wl.rb_omega(70, 1.0, m_max=3)
    if d == 4:
        gates = two_qubit_gates(5, 3, omega, seed=11, basis=ff.Basis.pauli(2) if pauli else ff.Basis.ggm(4))
    else:
        gates = single_qubit_gates(5, 3, omega, seed=11)
    names = [gates[0].n_oper_identifiers[2], gates[0].n_oper_identifiers[0]]
    seqs = draws([1, 2, 40, 130], 5, 5)
    pulses = pulses_of(gates, seqs, omega)
    eye = np.eye(d*d)
    for S in (wl.rb_spectrum(omega, 0.7), np.outer([1e-3, 2e-3], 1/omega)):
        K =ff.sequence_cumulant_functions(gates, seqs, S, omega, n_oper_identifiers=names)
        K_ref = loop(numeric.calculate_cumulant_function, pulses, S, omega, names)
        assert K.shape == K_ref.shape
        U = ff.sequence_error_transfer_matrices(gates, seqs, S, omega, n_oper_identifiers=names)
        U_ref = loop(ff.error_transfer_matrix, pulses, S, omega, names)
        assert U.shape == U_ref.shape == (4, d*d, d*d)
        for j in range(len(seqs)):
            print(f'd={d} G={len(seqs[j])}: K {rel_err(K[j], K_ref[j]):.2e}, U {np.abs(U[j] - U_ref[j]).max():.2e} '
                  f'of {np.abs(U_ref[j] - eye).max():.2e}')
            assert rel_err(K[j], K_ref[j]) < BAR, j
            assert np.abs(U[j] - U_ref[j]).max() < BAR*np.abs(U_ref[j] - eye).max() + 1e-15, j


def test_state_infidelity_of_the_benchmarking_study():
    """The study's state infidelity (input state an eigenstate of the third Pauli matrix): the diagonal of Gamma summed
    over the other basis elements, over d, against |R|^2 of the loop's control matrix integrated the same way."""
    omega = wl.rb_omega(301, wl.CONFIG3['T'])
    cliffords = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])[1]
    seqs = draws([2, 17, 64, 152], 4, 24)
    spectra = np.stack([wl.rb_spectrum(omega, alpha) for alpha in (0.0, 0.7)])
    gamma = ff.sequence_decay_amplitudes(cliffords, seqs, spectra, omega, stacked=True)
    assert gamma.shape == (2, 4, 1, 4, 4)
    got = gamma[:, :, 0, [0, 1, 2], [0, 1, 2]].sum(axis=-1)/2
    for j, pulse in enumerate(pulses_of(cliffords, seqs, omega)):
        R = pulse.get_control_matrix(omega)
        F = (np.abs(R[:, :3])**2).sum(axis=(0, 1))
        for k in range(2):
            ref = ff.util.integrate(F*spectra[k], omega)/(2*np.pi*2)
            assert abs(got[k, j] - ref) < 1e-12*abs(ref), (k, j, got[k, j], ref)


# ---- the loop route, exceptions, caches ------------------------------------------------------------------------------
def test_loop_route_returns_what_the_loop_returns():
    omega = wl.rb_omega(20, 1.0, m_max=3)
    rng = np.random.default_rng(3)
    d4 = two_qubit_gates(3, 2, omega, seed=1)
    C = rng.random((2, 2, 20)) + 1j*rng.random((2, 2, 20))
    cross = C + C.conj().swapaxes(0, 1)
    spin1 = [ff.PulseSequence([[np.diag([1.0, 0.0, -1.0]), [0.3 + 0.1*k], 'Z']],
                              [[np.diag([1.0, -1.0, 0.0]), [1.0], 'N']], [1.0]) for k in range(2)]
    X, Z = ff.util.paulis[1], ff.util.paulis[3]
    cliffords = wl.rb_cliffords(ff, omega, 1.0)[1]
    bare = ff.PulseSequence([[X/2, [0.4], 'X']], [[Z/2, [1.0], 'Z']], [1.0])
    for g in spin1 + [bare]:
        g.cache_control_matrix(omega)
    S = wl.rb_spectrum(omega, 0.7)
    cases = [(d4, [[0, 1, 2], [2, 2]], cross), (spin1, [[0, 1], [1, 1, 0]], S),
             (list(cliffords[:3]) + [bare], [[0, 3], [1, 2, 3]], S)]
    singles = (numeric.calculate_decay_amplitudes, numeric.calculate_cumulant_function, ff.error_transfer_matrix)
    functions = (ff.sequence_decay_amplitudes, ff.sequence_cumulant_functions, ff.sequence_error_transfer_matrices)
    for gates, seqs, spectrum in cases:
        pulses = pulses_of(gates, seqs, omega)
        for single, function in zip(singles, functions):
            got, U = function(gates, seqs, spectrum, omega, return_propagators=True)
            assert np.array_equal(got, loop(single, pulses, spectrum, omega))
            assert np.array_equal(U, np.stack([p.total_propagator for p in pulses]))
    stacked = ff.sequence_decay_amplitudes(d4, [[0, 1, 2], [2, 2]], np.stack([cross, 2*cross]), omega, stacked=True)
    assert stacked.shape == (2, 2, 2, 2, 16, 16)
    assert np.array_equal(stacked[1], ff.sequence_decay_amplitudes(d4, [[0, 1, 2], [2, 2]], 2*cross, omega))


def test_indices_exceptions_and_caches():
    omega = wl.rb_omega(20, 1.0, m_max=3)
    S = wl.rb_spectrum(omega, 0.7)
    gates = two_qubit_gates(4, 1, omega, seed=7)
    caches = lambda: [(sorted(g._data), sorted(g._frequency_data),                       # noqa: E731
                       {k: id(g._frequency_data.peek(k)) for k in g._frequency_data}) for g in gates]
    before = caches()
    got = ff.sequence_decay_amplitudes(gates, [[-1, 0, -4], [3, 0, 0]], S, omega)
    assert caches() == before
    assert np.array_equal(got[0], got[1])                                                # negative indices wrap
    for function in (ff.sequence_decay_amplitudes, ff.sequence_cumulant_functions,
                     ff.sequence_error_transfer_matrices):
        with pytest.raises(IndexError):
            function(gates, [[0, 4]], S, omega)
        with pytest.raises(ValueError):
            function(gates, [[0], []], S, omega)
        with pytest.raises(TypeError):
            function(gates, [[0.0, 1.0]], S, omega)
    # the loop's messages for a spectrum that does not fit the grid and for unknown identifiers
    pulse = pulses_of(gates, [[0, 1]], omega)[0]
    for kwargs in (dict(spectrum=np.ones(7)), dict(spectrum=S, n_oper_identifiers=['Q'])):
        with pytest.raises(ValueError) as loop_error:
            numeric.calculate_decay_amplitudes(pulse, kwargs['spectrum'], omega, kwargs.get('n_oper_identifiers'))
        with pytest.raises(ValueError) as error:
            ff.sequence_decay_amplitudes(gates, [[0, 1]], omega=omega, **kwargs)
        assert str(error.value) == str(loop_error.value)
    # gates without a control matrix on the grid are completed by one batched call, then read in place
    fresh = [ff.PulseSequence(list(zip(g.c_opers, g.c_coeffs, g.c_oper_identifiers)),
                              list(zip(g.n_opers, g.n_coeffs, g.n_oper_identifiers)), g.dt) for g in gates]
    assert rel_err(ff.sequence_decay_amplitudes(fresh, [[3, 0, 0], [1, 2]], S, omega),
                   ff.sequence_decay_amplitudes(gates, [[3, 0, 0], [1, 2]], S, omega)) < 1e-13
    assert all(resident_source(g, 4, 20, 16, 1) is not None for g in fresh)


def test_return_propagators_against_the_extended_product():
    omega = wl.rb_omega(20, 1.0, m_max=3)
    S = wl.rb_spectrum(omega, 0.7)
    for gates in (two_qubit_gates(4, 1, omega, seed=8), single_qubit_gates(4, 2, omega, seed=8)):
        seqs = draws([1, 3, 130, 500], 2, 4)
        yard = Yardstick(gates, omega)
        for function in (ff.sequence_cumulant_functions, ff.sequence_error_transfer_matrices):
            _, U = function(gates, seqs, S, omega, return_propagators=True)
            for j, s in enumerate(seqs):
                total = np.eye(yard.d, dtype=CLD)
                for k in s:
                    total = yard.U[k] @ total
                assert rel_err(U[j], total) < (LONG if len(s) >= 500 else TIGHT), j

"""ff.frequency_shifts (batch_second_order.py, csrc/second.hip: so_shift_kernel) and the second-order keyword of
ff.cumulant_functions / ff.error_transfer_matrices against the trapezoid of F2 from the definition in 60 digits
(tests/golden/second_order_exact.npz), and against the loop over the single functions on twin pulses.

Criterion for the frequency shifts (that of test_second_order_exact_gpu.py): per selected noise operator or operator
pair, max_kl |got - ref| <= 1e-10 max_kl |ref|.  Every test prints its worst value."""
import ctypes

import numpy as np
import pytest

import ff_oracle as orc
import filter_functions_amd as ff
import workloads as wl
from conftest import load_golden
from filter_functions_amd import _lib, batch_second_order, numeric
from filter_functions_amd._lib import as_c128, as_f64, ptr

pytestmark = pytest.mark.gpu

TOL = 1e-10
CASES = ['exact_d2', 'exact_d3', 'exact_d4',
         'near_idle_d2_1e-06', 'near_idle_d2_1e-09', 'near_idle_d2_1e-12', 'near_idle_d2_1e-15',
         'near_idle_d3_1e-09',
         'near_idle_d4_1e-06', 'near_idle_d4_1e-09', 'near_idle_d4_1e-12', 'near_idle_d4_1e-15',
         'crossing_d3_1e-09', 'crossing_d4_1e-06', 'crossing_d4_1e-09', 'crossing_d4_1e-12',
         'near_resonant_d2', 'near_resonant_d4', 'near_resonant_d5']


@pytest.fixture(scope='module')
def exact():
    return load_golden('second_order_exact')


def pair_error(got, ref):
    """worst selected operator (pair): max_kl |got - ref| / max_kl |ref|"""
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float64, (got.shape, ref.shape, got.dtype)
    return float((np.abs(got - ref).max(axis=(-2, -1))/np.abs(ref).max(axis=(-2, -1))).max())


def exact_pulse(g, name, scale=1.0):
    return ff.PulseSequence(
        [[op, scale*c, str(i)] for op, c, i in zip(g[f'{name}_c_opers'], g[f'{name}_c_coeffs'], g[f'{name}_c_ids'])],
        [[op, c, f'n{a}'] for a, (op, c) in enumerate(zip(g[f'{name}_n_opers'], g[f'{name}_n_coeffs']))],
        g[f'{name}_dt'], ff.Basis(g[f'{name}_basis'], btype='GGM'))


def spectra(omega, A):
    """the two spectra of test_second_order_exact_gpu.py and, for two operators, the Hermitian cross spectrum"""
    rows = np.stack([(a + 1.0)/(1.0 + (omega/(a + 2.0))**2) for a in range(A)])
    out = {'1-D': 1.0/(1.0 + omega**2), '(A, W)': rows}
    if A == 2:
        cross = np.zeros((2, 2, len(omega)), dtype=complex)
        cross[0, 0], cross[1, 1] = rows
        cross[0, 1] = 0.3*np.exp(0.7j*omega)/(1.0 + omega**2)
        cross[1, 0] = cross[0, 1].conj()
        out['(A, A, W)'] = cross
    return out


@pytest.mark.parametrize('case', range(len(CASES)), ids=CASES)
def test_batch_member_against_the_trapezoid_of_exact_second_order(exact, case):
    """The fixture's pulse is member s = case mod 3 of a batch of three; the other two are the same pulse with every
    control coefficient scaled by 0.5 and by 1.5 and are compared with numeric.calculate_frequency_shifts."""
    name, s = CASES[case], case % 3
    assert len(CASES) == 19 and f'{name}_F2' in exact
    omega, F2 = exact[f'{name}_omega'], exact[f'{name}_F2']
    A = F2.shape[0]
    scales = [0.5, 1.5]
    scales.insert(s, 1.0)
    runs = [(key, S, None, np.arange(A)) for key, S in spectra(omega, A).items()]
    if A == 2:
        runs.append(("(A, W), only 'n1'", spectra(omega, A)['(A, W)'][1:2], ['n1'], np.array([1])))
    worst_exact = worst_loop = 0.0
    for key, S, identifiers, idx in runs:
        pulses = [exact_pulse(exact, name, c) for c in scales]
        got = ff.frequency_shifts(pulses, S, omega, identifiers)
        assert not any(p.is_cached('filter_function_2') for p in pulses)       # the batched route ran
        ref = orc.frequency_shifts(F2, S, omega, idx)
        assert np.abs(ref).max(axis=(-2, -1)).min() >= 0.116                   # never a small divisor
        err = pair_error(got[s], ref)
        print(f'{name} slot {s}: {key} spectrum against the exact trapezoid, worst pair {err:.3e}')
        worst_exact = max(worst_exact, err)
        for j, c in enumerate(scales):
            if j != s:
                twin = numeric.calculate_frequency_shifts(exact_pulse(exact, name, c), S, omega, identifiers)
                err = pair_error(got[j], twin)
                print(f'{name} slot {j} (x{c}): {key} spectrum against the single function, worst pair {err:.3e}')
                worst_loop = max(worst_loop, err)
    print(f'{name}: worst against exact {worst_exact:.3e}, worst neighbour against the single function {worst_loop:.3e}')
    assert worst_exact <= TOL and worst_loop <= TOL


def random_pulse(seed, d, G, A, basis):
    c, cc, n, nc, dt = wl.random_pulse_inputs(seed, d, G, A, n_cops=2)
    return ff.PulseSequence(list(zip(c, cc)), list(zip(n, nc)), dt, basis)


def c_entry(pulses, S, omega, idx):
    """ffk_batch_frequency_shifts on diagonalised pulses, nothing in between"""
    for p in pulses:
        p.diagonalize()
    stack = lambda f, conv: conv(np.stack([f(p) for p in pulses]))      # noqa: E731
    D, V, Q = stack(lambda p: p.eigvals, as_f64), stack(lambda p: p.eigvecs, as_c128), \
        stack(lambda p: p.propagators, as_c128)
    B, s, dt = stack(lambda p: p.n_opers, as_c128), stack(lambda p: p.n_coeffs, as_f64), stack(lambda p: p.dt, as_f64)
    t = as_f64(np.concatenate((np.zeros((len(pulses), 1)), dt.cumsum(axis=1)), axis=1))
    C, omega, S = as_c128(np.asarray(pulses[0].basis)), as_f64(omega), as_c128(S)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    P, G, d = D.shape
    A, N, W, n_idx = B.shape[1], len(C), len(omega), len(idx)
    out = np.full((P, n_idx, n_idx, N, N) if S.ndim == 3 else (P, n_idx, N, N), np.nan)
    _lib.check(_lib.load().ffk_batch_frequency_shifts(
        P, ptr(D), ptr(V), ptr(Q), ptr(omega), W, ptr(C), N, ptr(B), A, ptr(s), ptr(dt), ptr(t), G, d, ptr(S), S.ndim,
        idx.ctypes.data_as(ctypes.c_void_p), n_idx, ptr(out)))
    return out


def test_a_pulse_has_the_same_bits_in_every_batch_and_slot():
    d, G, A, W = 3, 6, 2, 37                       # three frequency blocks of 16, the last ragged
    basis = ff.Basis.ggm(d)
    make = lambda k: random_pulse(8100 + k, d, G, A, basis)      # noqa: E731
    omega = wl.random_pulse_omega(make(0).dt, W)
    S = spectra(omega, A)['(A, A, W)']
    idx = np.arange(A)
    alone = c_entry([make(0)], S, omega, idx)[0]
    assert np.isfinite(alone).all()
    first_of_two = c_entry([make(0), make(1)], S, omega, idx)[0]
    last_of_five = c_entry([make(k) for k in (1, 2, 3, 4, 0)], S, omega, idx)[4]
    print('bits: P = 1 against slot 0 of 2:', np.abs(alone - first_of_two).max(),
          'against slot 4 of 5:', np.abs(alone - last_of_five).max())
    assert np.array_equal(alone, first_of_two) and np.array_equal(alone, last_of_five)


def general_spectra(omega, A):
    rows = np.stack([(a + 1.0)/(1.0 + (omega/(a + 2.0))**2) for a in range(A)])
    cross = np.zeros((A, A, len(omega)), dtype=complex)
    for a in range(A):
        cross[a, a] = rows[a]
        for b in range(a + 1, A):
            cross[a, b] = 0.3*np.exp(0.7j*(b - a)*omega)/(1.0 + omega**2)
            cross[b, a] = cross[a, b].conj()
    return {'1-D': 1.0/(1.0 + omega**2), '(A, W)': rows, '(A, A, W)': cross}


def against_the_loop(tag, d, A, G, W, P, basis, seed, subset=None):
    make = lambda: [random_pulse(seed + k, d, G, A, basis) for k in range(P)]      # noqa: E731
    omega = wl.random_pulse_omega(make()[0].dt, W)
    runs = [(key, S, None) for key, S in general_spectra(omega, A).items()]
    if subset is not None:
        runs.append((f'operators {subset}', general_spectra(omega, A)['(A, W)'][subset],
                     list(make()[0].n_oper_identifiers[subset])))
    worst = 0.0
    for key, S, identifiers in runs:
        pulses = make()
        got = ff.frequency_shifts(pulses, S, omega, identifiers)
        assert not any(p.is_cached('filter_function_2') for p in pulses)
        for j, twin in enumerate(make()):
            err = pair_error(got[j], numeric.calculate_frequency_shifts(twin, S, omega, identifiers))
            print(f'{tag}: {key} spectrum, member {j}, worst pair {err:.3e}')
            worst = max(worst, err)
    print(f'{tag}: worst pair {worst:.3e}')
    assert worst <= TOL


def test_tiles_and_frequency_blocks_two_qubits_four_operators():
    """A N = 64: more than one tile per side and off-diagonal tiles; three frequency blocks, the last ragged; every
    kind of spectrum, and operators 0 and 2 of 4 by a (2, W) spectrum"""
    d, A, G = 4, 4, 5
    query = _lib.load().ffk_batch_frequency_shifts_chunk
    chunk = query(35, d*d, A, G, d)
    W = 2*chunk + 3
    assert chunk > 0 and query(W, d*d, A, G, d) == chunk and -(-W//chunk) == 3
    against_the_loop('d=4 A=4', d, A, G, W, 3, ff.Basis.pauli(2), 8200, subset=[0, 2])


@pytest.mark.parametrize('d, A, G, W, P', [(5, 2, 4, 10, 2), (6, 2, 3, 9, 2), (2, 3, 7, 13, 5)],
                         ids=['d5 operator boundary inside a strip, padded k-step', 'd6 smaller tile',
                              'd2 three operators in one partial tile'])
def test_tiles_of_other_dimensions(d, A, G, W, P):
    basis = ff.Basis.pauli(1) if d == 2 else ff.Basis.ggm(d)
    against_the_loop(f'd={d} A={A}', d, A, G, W, P, basis, 8300 + 10*d)


def test_front_routes_a_mixed_list_like_the_loop():
    """Two batchable groups (G = 6 and G = 7), one pulse whose F2 is cached, in one list with the order kept; the
    shape the pass does not take (d = 9: no tile fits) has another output shape and therefore a list of its own."""
    from filter_functions_amd.pulse_sequence import _DIAGONALIZATION
    d, A, W = 3, 2, 21
    basis = ff.Basis.ggm(d)
    plan = [(6, 0), (7, 1), (6, 2), (5, 3), (7, 4), (6, 5)]              # (G, seed); index 3 is the cached one
    make = lambda: [random_pulse(8400 + k, d, G, A, basis) for G, k in plan]      # noqa: E731
    omega = wl.random_pulse_omega(make()[0].dt, W)
    S = general_spectra(omega, A)['(A, W)']
    pulses, twins = make(), make()
    cached = pulses[3].get_filter_function(omega, order=2)
    got = ff.frequency_shifts(pulses, S, omega)
    ref = np.stack([numeric.calculate_frequency_shifts(p, S, omega) for p in twins])
    err = max(pair_error(g, r) for g, r in zip(got, ref))
    print(f'front, mixed list: worst pair {err:.3e}')
    assert err <= TOL
    for i, p in enumerate(pulses):
        assert np.array_equal(p.omega, omega)
        assert all(key in p._data for key in _DIAGONALIZATION)
        assert p.is_cached('filter_function_2') == (i == 3)
    assert pulses[3].get_filter_function(omega, order=2) is cached or \
        np.array_equal(pulses[3].get_filter_function(omega, order=2), cached)
    # a batched member computes F2 later as before
    later = pulses[0].get_filter_function(omega, order=2)
    assert pair_error(numeric._frequency_shifts(later, S, omega, np.arange(A)), ref[0]) <= TOL

    d9 = ff.Basis.ggm(9)
    assert _lib.load().ffk_batch_frequency_shifts_chunk(5, 81, 1, 2, 9) == 0
    make9 = lambda: [random_pulse(8450 + k, 9, 2, 1, d9) for k in range(2)]       # noqa: E731
    omega9 = wl.random_pulse_omega(make9()[0].dt, 5)
    nine = make9()
    got9 = ff.frequency_shifts(nine, 1.0/(1.0 + omega9**2), omega9)
    ref9 = np.stack([numeric.calculate_frequency_shifts(p, 1.0/(1.0 + omega9**2), omega9) for p in make9()])
    assert np.array_equal(got9, ref9) and all(p.is_cached('filter_function_2') for p in nine)

    with pytest.raises(ValueError):
        ff.frequency_shifts(make()[:2] + make9()[:1], 1.0/(1.0 + omega**2), omega)
    empty = ff.frequency_shifts([], S, omega)
    assert empty.shape == (0,) and empty.dtype == np.float64


@pytest.mark.parametrize('d, A, G, W, P', [(2, 2, 6, 30, 3), (4, 2, 4, 9, 2)], ids=['one qubit', 'two qubits'])
def test_second_order_processes_against_the_loops(d, A, G, W, P):
    basis = ff.Basis.pauli(1 if d == 2 else 2)
    make = lambda: [random_pulse(8500 + 10*d + k, d, G, A, basis) for k in range(P)]      # noqa: E731
    omega = wl.random_pulse_omega(make()[0].dt, W)
    S = general_spectra(omega, A)['(A, W)']
    K = ff.cumulant_functions(make(), S, omega, second_order=True)
    K_ref = np.stack([numeric.calculate_cumulant_function(p, S, omega, second_order=True) for p in make()])
    U = ff.error_transfer_matrices(make(), S, omega, second_order=True)
    U_ref = np.stack([ff.error_transfer_matrix(p, S, omega, second_order=True) for p in make()])
    first_order = ff.cumulant_functions(make(), S, omega)
    assert K.shape == K_ref.shape and U.shape == U_ref.shape == (P, d*d, d*d)
    for j in range(P):
        err_K = np.abs(K[j] - K_ref[j]).max()/np.abs(K_ref[j]).max()
        err_U = np.abs(U[j] - U_ref[j]).max()/np.abs(U_ref[j]).max()
        print(f'd={d} pulse {j}: cumulant function {err_K:.3e}, error transfer matrix {err_U:.3e}')
        assert err_K <= TOL and err_U <= TOL
        assert np.abs(K[j] - first_order[j]).max() > 0.0        # the second-order term is there

"""ff.decay_amplitudes, ff.cumulant_functions, ff.error_transfer_matrices: many pulses in one pass, their control
matrices read where they lie in HBM -- against the reference's fixtures, against the loop of the single functions
on twin pulses built from the same inputs, and against themselves in other batches."""
import copy
import ctypes

import numpy as np
import pytest

import filter_functions_amd as ff
import workloads as wl
from conftest import load_golden, rel_err
from filter_functions_amd import _lib, batch, numeric, sequences
from filter_functions_amd._resident import Deferred, ResidentResult

pytestmark = pytest.mark.gpu

TOL = 1e-10          # the project's acceptance bar against the reference (test_gpu_parity.py)
LOOP = 1e-12         # against the loop: FP64 sums of at most 4096 non-cancelling terms in another order (4096 eps = 4.5e-13)

BATCHED = (ff.decay_amplitudes, ff.cumulant_functions, ff.error_transfer_matrices)
SINGLE = (numeric.calculate_decay_amplitudes, numeric.calculate_cumulant_function, ff.error_transfer_matrix)


def etm_pulse(g, name):
    basis = ff.Basis(g[f'{name}_basis'], btype=str(g[f'{name}_btype']))
    return ff.PulseSequence.from_arrays(
        g[f'{name}_c_opers'], g[f'{name}_c_oper_identifiers'], g[f'{name}_c_coeffs'],
        g[f'{name}_n_opers'], g[f'{name}_n_oper_identifiers'], g[f'{name}_n_coeffs'],
        g[f'{name}_dt'], basis)


def cfg2_pulse(seed, G=256, d=4, A=3, scale=1.0, basis=None):
    """A pulse of BASELINE config 2's shape (d = 4, three noise operators) from *seed*."""
    c_opers, c_coeffs, n_opers, n_coeffs, dt = wl.random_pulse_inputs(seed, d, G, A)
    if basis is None:
        basis = ff.Basis.pauli(int(np.log2(d)))
    return ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs*scale)), dt, basis)


def cfg2_omega(W, G=256):
    return wl.random_pulse_omega(wl.random_pulse_inputs(42, 4, G, 3)[-1], W)


def loop(single, pulses, *args):
    return np.stack([single(p, *args) for p in pulses])


def assert_etm_close(U, U_ref, bar):
    print('etm', np.abs(U - U_ref).max(), bar*np.abs(U_ref - np.eye(len(U_ref))).max() + 1e-15)
    assert np.abs(U - U_ref).max() < bar*np.abs(U_ref - np.eye(len(U_ref))).max() + 1e-15


def assert_like_loop(pulses, twins, S, omega, bar=LOOP):
    """All three batched functions on *pulses* against the single functions on *twins*, member by member."""
    for many, single in zip(BATCHED, SINGLE):
        got = many(pulses, S, omega)
        ref = loop(single, twins, S, omega)
        assert got.shape == ref.shape and got.dtype == np.float64
        for g, r in zip(got, ref):
            if many is ff.error_transfer_matrices:
                assert_etm_close(g, r, bar)
            else:
                print(many.__name__, rel_err(g, r))
                assert rel_err(g, r) < bar


def still_deferred(pulse):
    return type(pulse._frequency_data.peek('control_matrix')) is Deferred


@pytest.mark.parametrize('name', ['q1', 'q1id', 'p4', 'g3'])
def test_golden_parity(name):
    """Five copies of each fixture pulse with the control matrix cached, through all three functions, every member
    against the reference's outputs with the assertions of test_error_transfer_matrix_against_reference."""
    g = load_golden('etm')
    omega = g[f'{name}_omega']
    pulses = [etm_pulse(g, name) for _ in range(5)]
    for p in pulses:
        p.cache_control_matrix(omega)
    assert all(isinstance(p._resident, ResidentResult) and still_deferred(p) for p in pulses)
    for i in (1, 2, 3):
        S = g[f'{name}_S{i}']
        gamma = ff.decay_amplitudes(pulses, S, omega)
        ref = g[f'{name}_decay_amplitudes_S{i}']
        assert gamma.shape == (5,) + ref.shape and gamma.dtype == np.float64
        K = ff.cumulant_functions(pulses, S, omega)
        U = ff.error_transfer_matrices(pulses, S, omega)
        U_ref = g[f'{name}_error_transfer_matrix_S{i}']
        assert K.shape == gamma.shape and U.shape == (5,) + U_ref.shape
        for p in range(5):
            print(name, i, p, rel_err(gamma[p], ref), rel_err(K[p], g[f'{name}_cumulant_function_S{i}']))
            assert rel_err(gamma[p], ref) < TOL
            assert rel_err(K[p], g[f'{name}_cumulant_function_S{i}']) < TOL
            assert_etm_close(U[p], U_ref, TOL)
    sub = ff.decay_amplitudes(pulses, g[f'{name}_S1'], omega, n_oper_identifiers=pulses[0].n_oper_identifiers[1:])
    assert sub.shape == (5,) + g[f'{name}_decay_amplitudes_S1_sub'].shape
    for p in range(5):
        assert rel_err(sub[p], g[f'{name}_decay_amplitudes_S1_sub']) < TOL
    assert all(still_deferred(p) for p in pulses)          # nothing was fetched


def test_golden_parity_on_the_loop_route():
    """g6 (36 basis elements) in the same list shape: the single functions inside the call, the same values."""
    g = load_golden('etm')
    omega = g['g6_omega']
    pulses = [etm_pulse(g, 'g6') for _ in range(5)]
    for p in pulses:
        p.cache_control_matrix(omega)
    for i in (1, 2, 3):
        S = g[f'g6_S{i}']
        gamma = ff.decay_amplitudes(pulses, S, omega)
        K = ff.cumulant_functions(pulses, S, omega)
        U = ff.error_transfer_matrices(pulses, S, omega)
        for p in range(5):
            assert rel_err(gamma[p], g[f'g6_decay_amplitudes_S{i}']) < TOL
            assert rel_err(K[p], g[f'g6_cumulant_function_S{i}']) < TOL
            assert_etm_close(U[p], g[f'g6_error_transfer_matrix_S{i}'], TOL)
    sub = ff.decay_amplitudes(pulses, g['g6_S1'], omega, n_oper_identifiers=pulses[0].n_oper_identifiers[1:])
    assert rel_err(sub[3], g['g6_decay_amplitudes_S1_sub']) < TOL


@pytest.mark.parametrize('W,G', [(4096, 256), (96, 24)])
def test_batch_members_against_the_loop_and_in_place(W, G):
    """Seven pulses of config 2's shape with different seeds, members of one ff.get_filter_functions pass."""
    omega = cfg2_omega(W, G)
    pulses = [cfg2_pulse(100 + k, G) for k in range(7)]
    twins = [cfg2_pulse(100 + k, G) for k in range(7)]
    ff.get_filter_functions(pulses, omega)
    assert all(isinstance(p._resident, batch._Member) for p in pulses)
    for S in (1e-3/omega, np.outer([1e-3, 2e-3, 3e-3], 1/omega)):
        assert_like_loop(pulses, twins, S, omega)
    sub = ff.decay_amplitudes(pulses, 1e-3/omega, omega, n_oper_identifiers=pulses[0].n_oper_identifiers[1:])
    sub_ref = loop(numeric.calculate_decay_amplitudes, twins, 1e-3/omega, omega, twins[0].n_oper_identifiers[1:])
    assert sub.shape == sub_ref.shape == (7, 2, 16, 16)
    assert all(rel_err(g, r) < LOOP for g, r in zip(sub, sub_ref))
    # in place: nothing was fetched, and a later read returns what a twin taken in the same way returns
    assert all(still_deferred(p) for p in pulses)
    same_way = [cfg2_pulse(100 + k, G) for k in range(7)]
    ff.get_filter_functions(same_way, omega)
    for p, t in zip(pulses, same_way):
        assert np.array_equal(p.get_control_matrix(omega), t.get_control_matrix(omega))


@pytest.fixture(scope='module')
def study():
    omega = wl.rb_omega(301, wl.CONFIG3['T'])
    _, cliffords = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])
    cliffords = np.array(cliffords, dtype=object)
    lengths = [2, 3, 5, 17, 64, 65, 100, 151, 152]
    draws = [np.random.default_rng(300 + k).integers(0, 24, m) for k, m in enumerate(lengths)]
    return omega, [cliffords[i] for i in draws]


def test_sequence_results_against_the_loop_and_in_place(study):
    omega, seqs = study
    got = ff.concatenate_sequences(seqs)
    assert all(isinstance(p._resident, sequences._SequenceMember) for p in got)
    ref = [ff.concatenate(s) for s in seqs]
    for S in (wl.rb_spectrum(omega, 0.7), wl.rb_spectrum(omega, 0.0)[None]):
        assert_like_loop(got, ref, S, omega)
    assert all(still_deferred(p) for p in got)
    same_way = ff.concatenate_sequences(seqs)
    for p, t in zip(got, same_way):
        assert np.array_equal(p.get_control_matrix(omega), t.get_control_matrix(omega))


def test_the_examples_state_infidelity(study):
    """examples/randomized_benchmarking.py's state_infidelity -- the integral of |R[a, k]|^2 S over the basis elements
    other than ind = 3, over 2 pi d -- is the partial trace of the diagonal of Gamma over d."""
    omega, seqs = study
    got = ff.concatenate_sequences(seqs)
    twins = ff.concatenate_sequences(seqs)
    S = wl.rb_spectrum(omega, 0.7)
    gamma = ff.decay_amplitudes(got, S, omega)
    assert gamma.shape == (len(seqs), 1, 4, 4)
    trapezoid = getattr(np, 'trapezoid', None) or np.trapz
    ind, d = 3, 2
    keep = [k for k in range(4) if k != ind]
    measure = np.array([[gamma[p, a, keep, keep].sum()/d for a in range(1)] for p in range(len(seqs))])
    for p, twin in enumerate(twins):
        R = twin.get_control_matrix(omega)
        example = trapezoid((np.abs(R[:, keep])**2).sum(axis=1)*S, omega)/(2*np.pi*d)
        print('state infidelity', p, rel_err(measure[p], example))
        assert rel_err(measure[p], example) < LOOP
    assert all(still_deferred(p) for p in got)


def test_a_pulses_result_does_not_depend_on_its_batch():
    """The same pulse in a batch of 2 and of 64: bit for bit, all three outputs, real and cross-spectra."""
    W, G = 4096, 16
    omega = cfg2_omega(W, G)
    pulses = [cfg2_pulse(200 + k, G) for k in range(64)]
    ff.get_filter_functions(pulses, omega)
    rng = np.random.default_rng(3)
    cross = rng.standard_normal((3, 3, W)) + 1j*rng.standard_normal((3, 3, W))
    cross = 1e-3*(cross + cross.conj().swapaxes(0, 1))/omega
    for S in (np.outer([1e-3, 2e-3, 3e-3], 1/omega), cross):
        for many in BATCHED:
            small = many([pulses[5], pulses[40]], S, omega)
            large = many(pulses, S, omega)
            assert np.array_equal(small[0], large[5]) and np.array_equal(small[1], large[40])
            assert np.array_equal(many(pulses[::-1], S, omega), large[::-1])


def test_mixed_list_in_one_call():
    """Members of two passes, a single resident result, a host-array control matrix, a pulse with nothing cached, a
    d = 8 pulse on the loop route: output order, values against the loop, the caches of the formerly empty pulse."""
    W, G = 200, 16
    omega = cfg2_omega(W, G)
    seeds = dict(a=1, b=2, c=3, x=4, y=5, s=6, h=7, n=8, m=9)
    make = lambda: {k: cfg2_pulse(300 + v, G) for k, v in seeds.items()}     # noqa: E731
    eight = lambda: cfg2_pulse(310, 8, d=8, basis=ff.Basis(ff.Basis.pauli(3)[:16]))     # noqa: E731
    p, t = make(), make()
    ff.get_filter_functions([p['a'], p['b'], p['x']], omega)
    ff.get_filter_functions([p['y'], p['c']], omega)
    p['s'].cache_control_matrix(omega)
    p['h'].cache_control_matrix(omega)
    p['h'] = copy.deepcopy(p['h'])           # (a copy owns no device memory: its control matrix is a host array)
    assert p['h']._resident is None and isinstance(p['h']._frequency_data.peek('control_matrix'), np.ndarray)
    assert p['a']._resident.batch is p['b']._resident.batch is not p['c']._resident.batch
    order = ['a', 's', 'c', 'h', 'n', '8', 'b', 'm']
    pulses = [eight() if k == '8' else p[k] for k in order]
    twins = [eight() if k == '8' else t[k] for k in order]
    S = np.outer([1e-3, 2e-3, 3e-3], 1/omega)
    gamma = ff.decay_amplitudes(pulses, S, omega)
    # the formerly empty pulses: what cache_control_matrix leaves, and no filter function
    left = make()['n']
    left.cache_control_matrix(omega)
    for k in ('n', 'm'):
        assert 'filter_function' not in p[k]._frequency_data and still_deferred(p[k])
        assert sorted(p[k]._frequency_data) == sorted(left._frequency_data)
        assert sorted(p[k]._data) == sorted(left._data)
    assert p['n']._resident.batch is p['m']._resident.batch            # (they shared one pass)
    ref = loop(numeric.calculate_decay_amplitudes, twins, S, omega)
    assert gamma.shape == ref.shape == (8, 3, 16, 16)
    for k, g, r in zip(order, gamma, ref):
        print(k, rel_err(g, r))
        assert rel_err(g, r) < LOOP
    K = ff.cumulant_functions(pulses, S, omega)
    U = ff.error_transfer_matrices(pulses, S, omega)
    for g, r in zip(K, loop(numeric.calculate_cumulant_function, twins, S, omega)):
        assert rel_err(g, r) < LOOP
    for g, r in zip(U, loop(ff.error_transfer_matrix, twins, S, omega)):
        assert_etm_close(g, r, LOOP)
    for k in ('a', 'b', 'c', 's', 'n', 'm'):
        assert still_deferred(p[k])


def same_exception(call, reference):
    with pytest.raises(Exception) as ref:
        reference()
    with pytest.raises(type(ref.value)) as got:
        call()
    assert str(got.value) == str(ref.value)


def test_errors_are_the_loops():
    W, G = 64, 8
    omega = cfg2_omega(W, G)
    S = 1e-3/omega
    pulses = [cfg2_pulse(400 + k, G) for k in range(3)]
    ff.get_filter_functions(pulses, omega)
    twin = cfg2_pulse(400, G)
    qubit = wl.hadamard_pulse(ff)
    for many, single in zip(BATCHED, SINGLE):
        with pytest.raises(ValueError, match='same output shape'):
            many(pulses + [qubit], S, omega)
        same_exception(lambda: many(pulses, S, omega, ['nope']), lambda: single(twin, S, omega, ['nope']))
        same_exception(lambda: many(pulses, S[:-1], omega), lambda: single(twin, S[:-1], omega))
        same_exception(lambda: many(pulses, np.ones((3, 3, 3, W)), omega),
                       lambda: single(twin, np.ones((3, 3, 3, W)), omega))
        assert many([], S, omega).shape == (0,)


def test_a_member_that_overflows():
    """One member's noise coefficients scaled until its decay amplitudes overflow: the call does what the loop does
    for that list, and the other members' values are bit for bit what they are without it."""
    W, G = 64, 8
    omega = cfg2_omega(W, G)
    S = np.outer([1e-3, 2e-3, 3e-3], 1/omega)
    scales = [1.0, 1.0, 1e160, 1.0]
    build = lambda: [cfg2_pulse(500 + k, G, scale=s) for k, s in enumerate(scales)]      # noqa: E731
    for many, single in zip(BATCHED, SINGLE):
        pulses, twins = build(), build()
        outcome = None
        try:
            ref = loop(single, twins, S, omega)
        except Exception as err:       # noqa: BLE001  (whatever the loop raises is the contract)
            outcome = err
        if outcome is not None:
            with pytest.raises(type(outcome)) as got:
                many(pulses, S, omega)
            assert str(got.value) == str(outcome)
            others = [q for q, s in zip(build(), scales) if s == 1.0]
            assert np.isfinite(many(others, S, omega)).all()
            continue
        got = many(pulses, S, omega)
        assert not np.isfinite(ref[2]).all()
        assert np.array_equal(got[2], ref[2], equal_nan=True)
        others = [0, 1, 3]
        for k in others:
            if many is ff.error_transfer_matrices:
                assert_etm_close(got[k], ref[k], LOOP)
            else:
                assert rel_err(got[k], ref[k]) < LOOP
        without = many([pulses[k] for k in others], S, omega)
        assert np.array_equal(without, got[others])


def test_bad_arguments_at_the_c_entry():
    lib = _lib.load()
    W, G = 64, 8
    omega = np.ascontiguousarray(cfg2_omega(W, G))
    pulses = [cfg2_pulse(600 + k, G) for k in range(2)]
    ff.get_filter_functions(pulses, omega)
    member = pulses[0]._resident
    handles = (ctypes.c_void_p*2)(member.batch.handle.value, member.batch.handle.value)
    slots = np.array([0, 1], dtype=np.int32)
    basis = np.ascontiguousarray(np.asarray(pulses[0].basis), dtype=np.complex128)
    S = np.ascontiguousarray(1e-3/omega, dtype=np.complex128)
    idx = np.arange(3, dtype=np.int32)
    out = np.empty((2, 3, 16, 16))
    etm = np.empty((2, 16, 16))
    flags = np.zeros(2, dtype=np.int32)

    def call(handles=handles, slots=slots, table=None, P=2, A=3, N=16, W=W, d=4, omega=omega, basis=basis, single=0,
             S=S, s_ndim=1, idx=idx, n_idx=3, gamma=out, K=None, U=None, flags=flags):
        at = lambda a: None if a is None else a.ctypes.data     # noqa: E731
        return lib.ffk_resident_batch_processes(handles, at(slots), at(table), P, A, N, W, d, at(omega), at(basis),
                                                single, at(S), s_ndim, at(idx), n_idx, at(gamma), at(K), at(U),
                                                at(flags))
    assert call() == _lib.FFK_OK
    ref = numeric.calculate_decay_amplitudes(cfg2_pulse(600, G), 1e-3/omega, omega)
    assert rel_err(out[0], ref) < LOOP
    bad = [dict(handles=None), dict(slots=None), dict(omega=None), dict(basis=None), dict(S=None), dict(idx=None),
           dict(gamma=None), dict(gamma=None, U=etm, flags=None), dict(P=0), dict(P=65536), dict(A=2), dict(N=9),
           dict(N=17), dict(W=W + 1), dict(d=1), dict(d=3), dict(single=1), dict(s_ndim=0), dict(s_ndim=4),
           dict(n_idx=0), dict(n_idx=4), dict(idx=np.array([0, 1, 3], dtype=np.int32)),
           dict(idx=np.array([-1, 1, 2], dtype=np.int32)), dict(slots=np.array([0, 2], dtype=np.int32)),
           dict(slots=np.array([-1, 1], dtype=np.int32)),
           dict(handles=(ctypes.c_void_p*2)(None, member.batch.handle.value))]
    for kw in bad:
        assert call(**kw) == _lib.FFK_EINVAL, kw
        assert lib.ffk_last_error()
    assert call(gamma=None, U=etm) == _lib.FFK_OK and not flags.any()

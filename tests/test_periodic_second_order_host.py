"""CPU side of the second-order periodic-driving pass (ff.periodic_frequency_shifts, ff.periodic_cumulant_functions,
ff.periodic_error_transfer_matrices; ffk_periodic_shifts_dev / ffk_resident_periodic_shifts): the step plan, the
algebra of DESIGN.md section 7.16 in NumPy -- the sequential yardstick and the device's doubling, both in
periodic_shift_yardstick.py -- against the oracle evaluated from scratch on the tiled segments, public names, the ABI
in header, exports and binding, the workspace query without a GPU, the refusals of the entries before the device,
routing and pass splitting with the entry replaced by a stand-in, and the compositions with stand-ins.

Measured, max |Delta_n - oracle| / max |oracle| over n in {2, 3, 5, 7, 12} (3 segments, 2 noise operators, 11
frequencies with w = 0 among them, Delta_1 from the oracle):
    d = 2: sequential 1.6e-15 (np.longdouble 1.9e-15), doubling 1.5e-15;  d = 3 (GGM): 3.5e-15 (3.7e-15), 1.8e-14;
    d = 4 (Pauli): 3.2e-15 (3.2e-15), 5.1e-15 -- the oracle's own double-precision sum is the larger part.
"""
import ctypes

import numpy as np
import pytest

import ff_oracle as orc
import filter_functions_amd as ff
import periodic_shift_yardstick as shift_yard
from conftest import rel_err
from filter_functions_amd import _lib, batch, batch_second_order, expm_batch, periodic
from filter_functions_amd import periodic_second_order as pso
from filter_functions_amd import sequence_prefix_second_order
from test_periodic_host import host_pulse

ENTRIES = ('ffk_periodic_shifts_workspace_bytes', 'ffk_periodic_shifts_dev', 'ffk_resident_periodic_shifts')


# ---- the step plan --------------------------------------------------------------------------------------------------
def pairs(repeats):
    steps, _ = pso.step_plan(repeats)
    return [tuple(int(v) for v in row[:2]) for row in steps]


def test_step_plan_of_single_counts():
    steps, slots = pso.step_plan([1])
    assert steps.shape == (0, 4) and steps.dtype == np.int32 and slots.tolist() == [0] and slots.dtype == np.int32
    assert pairs([2]) == [(1, 1)]
    assert pairs([7]) == [(1, 1), (2, 2), (4, 2), (6, 1)]
    assert pairs([12]) == [(1, 1), (2, 2), (4, 4), (8, 4)]
    assert pairs([2**20]) == [(2**j, 2**j) for j in range(20)]
    top = 2**31 - 1
    want = [(2**j, 2**j) for j in range(30)] + [(2**31 - 2**(j + 1), 2**j) for j in range(29, -1, -1)]
    assert pairs([top]) == want and len(want) == 60
    steps, slots = pso.step_plan([top])
    assert int(steps[-1, 0]) + int(steps[-1, 1]) == top and slots.tolist() == [60]
    # every step reads slots that are written: slot 0 is Delta_1, the result of step s lies in slot s + 1
    for repeats in ([7], [12], [top], [5, 1000, 3, 999, 2**20 + 5]):
        steps, slots = pso.step_plan(repeats)
        value = {0: 1}
        for s, (m, mp, slot_m, slot_mp) in enumerate(steps.tolist()):
            assert slot_m <= s and slot_mp <= s and value[slot_m] == m and value[slot_mp] == mp
            assert mp & (mp - 1) == 0                                 # m' is a power of two from the chain
            value[s + 1] = m + mp
        assert [value[s] for s in slots.tolist()] == list(repeats)


def test_step_plan_shares_steps_and_a_counts_steps_depend_on_the_count_alone():
    alone = {n: pairs([n]) for n in (1, 2, 3, 7, 12, 13, 1000)}
    for repeats in ([7, 12], [12, 7, 1, 7], [1000, 13, 3, 2, 1, 12, 7]):
        steps, slots = pso.step_plan(repeats)
        made = [tuple(int(v) for v in row[:2]) for row in steps]
        assert len(set(made)) == len(made)                            # every (m, m') once
        assert set(made) == set().union(*(alone[n] for n in repeats))
        # the chain of steps behind a count's slot is that of the count alone
        by_value = {m + mp: (m, mp) for m, mp in made}
        for n in repeats:
            need, todo = set(), [n]
            while todo:
                v = todo.pop()
                if v > 1 and by_value[v] not in need:
                    need.add(by_value[v])
                    todo.extend(by_value[v])
            assert need == set(alone[n]), n
    # S <= floor(log2 n_max) + sum_k (popcount(n_k) - 1)
    repeats = [1000, 13, 3, 2, 1, 12, 7]
    assert len(pso.step_plan(repeats)[0]) <= 9 + sum(bin(n).count('1') - 1 for n in repeats)
    steps, slots = pso.step_plan([5, 5, 1, 5])
    assert len(steps) == 3 and slots.tolist() == [3, 3, 0, 3]
    for bad in ([0], [2**31], [3, -1]):
        with pytest.raises(ValueError):
            pso.step_plan(bad)
    assert len(pso.step_plan(np.arange(1, pso.MAX_COUNTS + 1) + 2**30)[0]) <= pso.MAX_STEPS


# ---- the algebra against the oracle from scratch --------------------------------------------------------------------
def herm(rng, d):
    m = rng.normal(size=(d, d)) + 1j*rng.normal(size=(d, d))
    return m + m.conj().T


@pytest.mark.parametrize('d', [2, 3, 4])
def test_yardstick_and_doubling_against_the_oracle_from_scratch(d):
    """Bar: 1e-10 of max |Delta_n|, the project's parity contract."""
    rng = np.random.default_rng(40 + d)
    basis = orc.basis_ggm(3) if d == 3 else orc.basis_pauli(d//2)
    G, A = 3, 2
    H = np.stack([herm(rng, d) for _ in range(G)])*0.7
    dt = rng.uniform(0.3, 0.9, G)
    n_opers = np.stack([herm(rng, d) for _ in range(A)])
    n_coeffs = rng.uniform(0.5, 1.5, (A, G))
    omega = np.concatenate([[0.0], np.sort(rng.uniform(0.0, 12.0, 10))])
    S = 1.0/(1.0 + omega**2) + 0.1
    idx = np.arange(A)

    def from_scratch(n):
        D, V, Q = orc.diagonalize(np.tile(H, (n, 1, 1)), np.tile(dt, n))
        F2 = orc.second_order_filter_function(D, V, Q, omega, basis, n_opers, np.tile(n_coeffs, (1, n)),
                                              np.tile(dt, n))
        return orc.frequency_shifts(F2, S, omega, idx)

    D, V, Q = orc.diagonalize(H, dt)
    R1 = orc.control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
    U, T = Q[-1], dt.sum()
    delta1 = from_scratch(1)
    counts = [2, 3, 5, 7, 12]
    sequential = shift_yard.sequential_frequency_shifts(R1, basis, U, T, omega, S, delta1, counts)
    wide = shift_yard.sequential_frequency_shifts(R1, basis, U, T, omega, S, delta1, counts, extended=True)
    doubling = shift_yard.doubling_frequency_shifts(R1, basis, U, T, omega, S, delta1, *pso.step_plan(counts))
    for k, n in enumerate(counts):
        ref = from_scratch(n)
        errors = rel_err(sequential[n], ref), rel_err(wide[n], ref), rel_err(doubling[k], ref)
        print(f'd = {d} n = {n}: sequential {errors[0]:.2e} extended {errors[1]:.2e} doubling {errors[2]:.2e}')
        assert max(errors) < 1e-10, (n, errors)
        # the second-order term is there: Delta_n is not n Delta_1
        assert rel_err(n*delta1, ref) > 1e-3
    # a spectrum of two dimensions, one row per operator
    S2 = np.stack([S, 2.0*S + 0.3])
    delta1 = orc.frequency_shifts(orc.second_order_filter_function(D, V, Q, omega, basis, n_opers, n_coeffs, dt), S2,
                                  omega, idx)
    D3, V3, Q3 = orc.diagonalize(np.tile(H, (3, 1, 1)), np.tile(dt, 3))
    ref = orc.frequency_shifts(orc.second_order_filter_function(D3, V3, Q3, omega, basis, n_opers,
                                                                np.tile(n_coeffs, (1, 3)), np.tile(dt, 3)),
                               S2, omega, idx)
    assert rel_err(shift_yard.sequential_frequency_shifts(R1, basis, U, T, omega, S2, delta1, [3])[3], ref) < 1e-10
    assert rel_err(shift_yard.doubling_frequency_shifts(R1, basis, U, T, omega, S2, delta1, *pso.step_plan([3]))[0],
                   ref) < 1e-10


# ---- names, ABI, workspace ------------------------------------------------------------------------------------------
def test_public_names():
    for name in pso.__all__:
        assert name in ff.__all__ and getattr(ff, name) is getattr(pso, name)
    assert ff.periodic_second_order is pso and 'periodic_second_order' in ff.__all__
    assert set(pso.__all__) == {'periodic_frequency_shifts', 'periodic_cumulant_functions',
                                'periodic_error_transfer_matrices'}


def test_binding_header_and_exports_agree():
    import test_abi
    names = test_abi.header_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in names and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES[ENTRIES[0]] == (ctypes.c_size_t, [ctypes.c_int]*9)
    assert len(_lib.SIGNATURES[ENTRIES[1]][1]) == 23 and len(_lib.SIGNATURES[ENTRIES[2]][1]) == 22


def test_workspace_query_needs_no_gpu():
    q = _lib.load().ffk_periodic_shifts_workspace_bytes
    # (P, K, S, n_host, A, W, d, n_idx, s_ndim)
    for P, K, S, n_host, A, W, d, n_idx, s_ndim in [(64, 25, 60, 0, 1, 500, 2, 1, 1), (16, 25, 60, 16, 3, 500, 4, 3, 2),
                                                     (3, 5, 4, 1, 2, 33, 3, 2, 1), (1, 1, 0, 0, 1, 2, 2, 1, 1)]:
        need = q(P, K, S, n_host, A, W, d, n_idx, s_ndim)
        tile = 8*P*n_idx*d**4
        assert need >= tile*(1 + S + S + 1 + K) + 16*A*d*d*W*n_host
        # what the Python side counts per pass covers it, and not by much
        counted = (pso.fixed_bytes(K, S, A, d*d, W, d, n_idx, s_ndim)
                   + P*pso.member_bytes(K, S, A, d*d, W, d, n_idx, n_host > 0))
        assert need <= counted <= need + 16*A*d*d*W*(P - n_host)*(n_host > 0) + 16*256, (P, K, S)
    good = (4, 5, 6, 0, 2, 33, 2, 2, 1)
    assert q(*good) > 0
    for at, bad in [(0, 0), (0, 65536), (1, 0), (1, 65536), (2, -1), (2, 65536), (3, -1), (3, 5), (4, 0), (5, 0),
                    (5, 1), (6, 1), (6, 5), (7, 0), (7, 3), (8, 3), (8, 0)]:
        args = list(good)
        args[at] = bad
        assert q(*args) == 0, (at, bad)


def _host_call(**change):
    P, A, W, d, K, n_idx, S = 2, 2, 5, 2, 3, 2, 2
    keep = dict(handles=(ctypes.c_void_p*P)(), slots=np.full(P, -1, dtype=np.int32),
                table=np.zeros((P, A, d*d, W), dtype=complex), omega=np.linspace(0, 1, W),
                basis=np.zeros((d*d, d, d), dtype=complex), V=np.zeros((P, d, d), dtype=complex),
                phi=np.zeros((P, d, d, 2)), T=np.ones(P),
                steps=np.array([[1, 1, 0, 0], [2, 1, 1, 0]], dtype=np.int32),
                count_slots=np.array([0, 1, 2], dtype=np.int32), spectrum=np.ones(W, dtype=complex),
                idx=np.arange(n_idx, dtype=np.int32), delta1=np.zeros((P, n_idx, d*d, d*d)),
                out=np.zeros((P, K, n_idx, d*d, d*d)))
    a = dict(P=P, A=A, W=W, d=d, K=K, S=S, s_ndim=1, n_idx=n_idx)
    a.update({k: v for k, v in change.items() if k in a})
    for k, v in change.items():
        if k in keep:
            keep[k] = v

    def at(x):
        return None if x is None else (x if isinstance(x, ctypes.Array) else x.ctypes.data)
    host = (at(keep['handles']), at(keep['slots']), at(keep['table']), a['P'], a['A'], a['W'], a['d'],
            at(keep['omega']), at(keep['basis']), at(keep['V']), at(keep['phi']), at(keep['T']), at(keep['steps']),
            a['S'], at(keep['count_slots']), a['K'], at(keep['spectrum']), a['s_ndim'], at(keep['idx']), a['n_idx'],
            at(keep['delta1']), at(keep['out']))
    dev = host[2:] + (None, 0, None)
    return host, dev, keep


def test_bad_arguments_are_refused_before_the_device():
    lib = _lib.load()
    cases = [(dict(omega=None), 'NULL'), (dict(out=None), 'NULL'), (dict(V=None), 'NULL'), (dict(steps=None), 'NULL'),
             (dict(count_slots=None), 'NULL'), (dict(delta1=None), 'NULL'), (dict(spectrum=None), 'NULL'),
             (dict(P=0), 'unsupported shape'), (dict(K=0), 'unsupported shape'), (dict(d=5), 'unsupported shape'),
             (dict(d=1), 'unsupported shape'), (dict(n_idx=3), 'unsupported shape'), (dict(S=-1), 'unsupported shape'),
             (dict(S=65536), 'unsupported shape'), (dict(s_ndim=3), 'unsupported shape'),
             (dict(W=1), 'unsupported shape')]
    for change, message in cases:
        host, dev, keep = _host_call(**change)
        for entry, args in ((lib.ffk_resident_periodic_shifts, host), (lib.ffk_periodic_shifts_dev, dev)):
            assert entry(*args) == _lib.FFK_EINVAL, change
            assert message in lib.ffk_last_error().decode(), (change, lib.ffk_last_error().decode())
    # the device-pointer entry without its workspace
    _, dev, keep = _host_call()
    assert lib.ffk_periodic_shifts_dev(*dev) == _lib.FFK_EINVAL and 'workspace' in lib.ffk_last_error().decode()
    # what only the host-pointer entry can read: the plan and the operator indices
    for change, message in [(dict(steps=np.array([[1, 1, 0, 0], [2, 1, 2, 0]], dtype=np.int32)), 'steps[1] reads'),
                            (dict(steps=np.array([[1, 1, 0, 1], [2, 1, 1, 0]], dtype=np.int32)), 'steps[0] reads'),
                            (dict(steps=np.array([[0, 1, 0, 0], [2, 1, 1, 0]], dtype=np.int32)), 'steps[0] = (0, 1)'),
                            (dict(steps=np.array([[2**31 - 1, 1, 0, 0], [2, 1, 1, 0]], dtype=np.int32)), 'steps[0]'),
                            (dict(count_slots=np.array([0, 3, 2], dtype=np.int32)), 'count_slots[1] = 3'),
                            (dict(idx=np.array([0, 2], dtype=np.int32)), 'idx[1] = 2')]:
        host, _, keep = _host_call(**change)
        assert lib.ffk_resident_periodic_shifts(*host) == _lib.FFK_EINVAL
        assert message in lib.ffk_last_error().decode(), lib.ffk_last_error().decode()


# ---- routing, with the entry and ff.frequency_shifts replaced by stand-ins ------------------------------------------
class StandIn:
    """Records every call of ffk_resident_periodic_shifts and fills `out` with the pass's number."""

    def __init__(self):
        self.calls = []

    def ffk_resident_periodic_shifts(self, handles, slots, table, P, A, W, d, omega, basis, V, phi, T, steps, S,
                                     count_slots, K, spectrum, s_ndim, idx, n_idx, delta1, out):
        n = P*K*n_idx*d**4
        np.ctypeslib.as_array((ctypes.c_double*n).from_address(out))[:] = len(self.calls)
        plan = np.ctypeslib.as_array((ctypes.c_int32*(4*S)).from_address(steps)).reshape(S, 4).copy() if S else None
        first = np.ctypeslib.as_array((ctypes.c_double*(P*n_idx*d**4)).from_address(delta1)).copy()
        self.calls.append(dict(P=P, K=K, S=S, d=d, A=A, s_ndim=s_ndim, n_idx=n_idx, hosts=table is not None,
                               handles=[h for h in handles], steps=plan, delta1=first.reshape(P, -1)))
        return _lib.FFK_OK


@pytest.fixture
def stand_in(monkeypatch):
    fake = StandIn()
    fake.first_order = []

    def frequency_shifts(pulses, spectrum, omega, n_oper_identifiers=None):
        fake.first_order.append(len(pulses))
        idx = ff.util.get_indices_from_identifiers(pulses[0].n_oper_identifiers, n_oper_identifiers)
        N = len(pulses[0].basis)
        return np.stack([np.full((len(idx), N, N), 100.0 + sum(map(ord, str(p.tau)))) for p in pulses])
    monkeypatch.setattr(pso._lib, 'load', lambda: fake)
    monkeypatch.setattr(batch_second_order, 'frequency_shifts', frequency_shifts)
    return fake


def test_routing_groups_by_shape_and_splits_under_the_budget(stand_in, monkeypatch):
    rng = np.random.default_rng(3)
    omega = np.linspace(0, 5, 9)
    same = [host_pulse(rng, 2, omega) for _ in range(5)]
    repeats = [1, 4, 9]
    out = ff.periodic_frequency_shifts(same[:3], repeats, np.ones(9), omega)
    assert out.shape == (3, 3, 2, 4, 4) and len(stand_in.calls) == 1 and stand_in.first_order == [3]
    call = stand_in.calls[0]
    assert call['P'] == 3 and call['K'] == 3 and call['S'] == 4 and call['s_ndim'] == 1 and call['hosts']
    assert call['handles'] == [None]*3
    assert call['steps'][:, :2].tolist() == [[1, 1], [2, 2], [4, 4], [8, 1]]
    # Delta_1 of ONE ff.frequency_shifts call reaches the pass in member order
    assert [row[0] for row in call['delta1']] == [100.0 + sum(map(ord, str(p.tau))) for p in same[:3]]
    del stand_in.calls[:], stand_in.first_order[:]
    # repeats = [1]: no step
    ff.periodic_frequency_shifts(same[:2], [1], np.ones((2, 9)), omega)
    assert stand_in.calls[0]['S'] == 0 and stand_in.calls[0]['steps'] is None and stand_in.calls[0]['s_ndim'] == 2
    del stand_in.calls[:], stand_in.first_order[:]
    with pytest.raises(ValueError, match='same output shape'):
        ff.periodic_frequency_shifts(same[:1] + [host_pulse(rng, 4, omega, A=2)], repeats, np.ones(9), omega)
    # a budget of two members: passes of one, two and two (batch.split_passes: sizes differ by one at most)
    per = pso.member_bytes(3, 4, 2, 4, 9, 2, 2, True)
    fixed = pso.fixed_bytes(3, 4, 2, 4, 9, 2, 2, 2)
    monkeypatch.setattr(batch, 'PASS_BYTES', fixed + 2*per)
    out = ff.periodic_frequency_shifts(same, repeats, np.ones((2, 9)), omega)
    assert out.shape == (5, 3, 2, 4, 4) and stand_in.first_order == [5]
    assert [c['P'] for c in stand_in.calls] == [1, 2, 2]
    assert [out[i, 0, 0, 0, 0] for i in range(5)] == [0, 1, 1, 2, 2]


def test_what_the_batched_route_does_not_take(stand_in, monkeypatch):
    """Cross-spectra, a complex spectrum, a non-unitary propagator, no count at all: the fallback."""
    rng = np.random.default_rng(4)
    omega = np.linspace(0, 5, 9)
    pulses = [host_pulse(rng, 2, omega), host_pulse(rng, 2, omega)]
    seen = []

    def fallback(pulse, repeats, spectrum, omega, n_oper_identifiers):
        seen.append([int(n) for n in repeats])
        return np.zeros((len(repeats), 2, 4, 4))
    monkeypatch.setattr(pso, '_fallback', fallback)
    ff.periodic_frequency_shifts(pulses, [1, 2], np.ones((2, 2, 9)), omega)
    assert not stand_in.calls and not stand_in.first_order and seen == [[1, 2]]*2
    del seen[:]
    ff.periodic_frequency_shifts(pulses, [3], np.ones(9)*(1 + 1j), omega)
    assert not stand_in.calls and seen == [[3]]*2
    del seen[:]
    assert ff.periodic_frequency_shifts(pulses, [], np.ones(9), omega).shape == (2, 0, 2, 4, 4)
    assert not stand_in.calls and seen == [[]]*2
    del seen[:]
    pulses[1].total_propagator = np.array([[1, 1], [0, 1]], dtype=complex)      # not normal: a residue is left
    ff.periodic_frequency_shifts(pulses, [3], np.ones(9), omega)
    assert [c['P'] for c in stand_in.calls] == [1] and stand_in.first_order == [1] and seen == [[3]]


def test_exceptions(stand_in):
    rng = np.random.default_rng(5)
    omega = np.linspace(0, 5, 9)
    pulses = [host_pulse(rng, 2, omega)]
    for f in (ff.periodic_frequency_shifts, ff.periodic_cumulant_functions, ff.periodic_error_transfer_matrices):
        with pytest.raises(TypeError, match='Can only concatenate PulseSequences'):
            f(pulses + ['pulse'], [1], np.ones(9), omega)
        for bad in ([0], [3, -1], [[1, 2]], [2**31]):
            with pytest.raises(ValueError):
                f(pulses, bad, np.ones(9), omega)
        with pytest.raises(TypeError):
            f(pulses, [1.5], np.ones(9), omega)
    with pytest.raises(ValueError, match='Spectrum should be of shape'):
        ff.periodic_frequency_shifts(pulses, [2], np.ones(8), omega)
    with pytest.raises(ValueError):
        ff.periodic_frequency_shifts(pulses, [2], np.ones(9), omega, n_oper_identifiers=['nope'])
    assert not stand_in.calls
    out = ff.periodic_frequency_shifts([], [1, 2], np.ones(9), omega)
    assert out.shape == (0,) and out.dtype == np.float64


# ---- the compositions, with stand-ins for Gamma, Delta, the cumulant entries and the exponential --------------------
def test_compositions(monkeypatch):
    rng = np.random.default_rng(6)
    omega = np.linspace(0, 5, 9)
    pulses = [host_pulse(rng, 2, omega), host_pulse(rng, 2, omega)]
    gamma = rng.normal(size=(2, 3, 2, 4, 4))
    delta = rng.normal(size=(2, 3, 2, 4, 4))
    seen = dict(gamma=0, delta=0, cumulants=[], expm=[])

    def decay(pulses, repeats, spectrum, omega, n_oper_identifiers=None):
        seen['gamma'] += 1
        return gamma

    def shifts(pulses, repeats, spectrum, omega, n_oper_identifiers=None):
        seen['delta'] += 1
        return delta

    def cumulants(g, dl, basis):
        seen['cumulants'].append((g.copy(), None if dl is None else dl.copy()))
        return g + (0 if dl is None else 10*dl)

    def expm(tiles):
        seen['expm'].append(tiles.shape)
        return tiles.sum(axis=1)
    monkeypatch.setattr(periodic, 'periodic_decay_amplitudes', decay)
    monkeypatch.setattr(pso, 'periodic_frequency_shifts', shifts)
    monkeypatch.setattr(sequence_prefix_second_order, '_cumulants', cumulants)
    monkeypatch.setattr(expm_batch, 'exponentiate_cumulant_functions', expm)
    # second_order=False runs no second-order code
    K1 = ff.periodic_cumulant_functions(pulses, [1, 2, 3], np.ones(9), omega)
    assert seen['gamma'] == 1 and seen['delta'] == 0 and len(seen['cumulants']) == 1
    assert seen['cumulants'][0][1] is None and np.array_equal(seen['cumulants'][0][0], gamma.reshape(-1, 4, 4))
    assert np.array_equal(K1, gamma)
    K2 = ff.periodic_cumulant_functions(pulses, [1, 2, 3], np.ones(9), omega, second_order=True)
    assert seen['delta'] == 1 and np.array_equal(seen['cumulants'][1][1], delta.reshape(-1, 4, 4))
    assert np.array_equal(K2, gamma + 10*delta)
    # ONE exponential over all P K matrices
    E = ff.periodic_error_transfer_matrices(pulses, [1, 2, 3], np.ones(9), omega, second_order=True)
    assert seen['expm'] == [(6, 2, 4, 4)] and E.shape == (2, 3, 4, 4)
    assert np.array_equal(E, (gamma + 10*delta).sum(axis=2))
    ff.periodic_error_transfer_matrices(pulses, [1, 2, 3], np.ones(9), omega)
    assert seen['delta'] == 2 and seen['expm'] == [(6, 2, 4, 4)]*2
    # a mismatch of the two shapes is an error
    delta = delta[:, :2]
    with pytest.raises(ValueError, match='not same shape'):
        ff.periodic_cumulant_functions(pulses, [1, 2, 3], np.ones(9), omega, second_order=True)

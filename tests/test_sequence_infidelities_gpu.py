"""ff.sequence_infidelities: infidelities of many gate sequences given as index arrays into one gate set, single-
and two-qubit gates, against the concatenation rule run on the host in extended precision from the same inputs
(the gates' cached control matrices and total propagators), against the loop over ff.concatenate and ff.infidelity,
and against itself in other passes."""
import ctypes

import numpy as np
import pytest

import filter_functions_amd as ff
import workloads as wl
from conftest import rel_err
from filter_functions_amd import _lib
from filter_functions_amd.sequences import resident_source

pytestmark = pytest.mark.gpu

TIGHT = 2e-13         # per tensor, sequences of fewer than 500 positions
LONG = 1e-12          # sequences of 500 positions or more
LD, CLD = np.longdouble, np.clongdouble
NAMES = ('IX', 'IZ', 'XI', 'ZI', 'ZZ')


def pauli_string(name):
    P = dict(zip('IXYZ', ff.util.paulis))
    return np.kron(P[name[0]], P[name[1]])


def two_qubit_gates(T, A, omega, seed, basis=None, names=None):
    """T random two-qubit gates of one and two segments (control on XI, IX and ZZ), every one carrying the first A
    noise operators of NAMES (or *names*), control matrices cached at omega."""
    rng = np.random.default_rng(seed)
    names = NAMES[:A] if names is None else names
    gates = []
    for k in range(T):
        G = 1 + k % 2
        gate = ff.PulseSequence([[pauli_string(c)/2, rng.normal(size=G), c] for c in ('XI', 'IX', 'ZZ')],
                                [[pauli_string(n)/2, 0.5 + rng.random(G), n] for n in names], 1.0 + rng.random(G),
                                basis=basis)
        gate.cache_control_matrix(omega)
        gates.append(gate)
    return gates


def draws(lengths, seed, n_gates):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, n_gates, m) for m in lengths]


def loop(gates, seqs, S, omega, names=None):
    table = np.asarray(gates, dtype=object)
    pulses = [ff.concatenate(table[s], omega=omega) for s in seqs]
    return np.stack([ff.infidelity(p, S, omega, n_oper_identifiers=names) for p in pulses]), pulses


def spectra(n_idx, omega, seed):
    """Spectra of one, two and three dimensions; the last a Hermitian cross-spectrum."""
    rng = np.random.default_rng(seed)
    W = len(omega)
    C = rng.random((n_idx, n_idx, W)) + 1j*rng.random((n_idx, n_idx, W))
    return [wl.rb_spectrum(omega, 0.7), rng.random((n_idx, W)), C + C.conj().swapaxes(0, 1)]


# ---- the yardstick: the recurrence, F and the trapezoid integral on the host in np.longdouble ----------------------
class Yardstick:
    """From the same inputs as the device: the gates' cached control matrices and total propagators, L_k formed in
    long double, phases exp(i fl64(omega tau))."""

    def __init__(self, gates, omega):
        self.omega, self.d = np.asarray(omega, dtype=np.float64), gates[0].d
        C = np.asarray(gates[0].basis).astype(CLD)
        self.U = [np.asarray(g.total_propagator).astype(CLD) for g in gates]
        # L_k[i, j] = tr(U^dag C_i U C_j)
        self.L = [np.einsum('ba,ibc,cd,jda->ij', U.conj(), C, U, C).real.astype(CLD) for U in self.U]
        self.v = [np.asarray(g.get_control_matrix(omega)).astype(CLD).transpose(0, 2, 1) for g in gates]   # (A, W, N)
        arg = [(self.omega*g.tau).astype(LD) for g in gates]             # rounded to double first, as the device
        self.p = [(np.cos(x) + 1j*np.sin(x))[None, :, None] for x in arg]

    def sequence(self, s):
        """(R (A, N, W), F (A, A, W), total propagator) of the sequence of gate numbers *s*."""
        S = np.zeros_like(self.v[0])
        for k in s[::-1]:
            S = self.v[k] + self.p[k]*(S @ self.L[k])
        total = np.eye(self.d, dtype=CLD)
        for k in s:
            total = self.U[k] @ total
        return S.transpose(0, 2, 1), np.einsum('awk,bwk->abw', S.conj(), S), total

    def infidelity(self, F, S, idx):
        S = np.asarray(S)
        idx = np.asarray(idx)
        picked = F[idx[:, None], idx] if S.ndim == 3 else F[idx, idx]
        f = (picked*S.astype(CLD if np.iscomplexobj(S) else LD)).real
        x = self.omega.astype(LD)
        pi = 4*np.arctan(LD(1))
        return ((f[..., 1:] + f[..., :-1])*np.diff(x)).sum(axis=-1)/2/(2*pi*self.d)


WORST = {'new': 0.0, 'loop': 0.0}


def check_against_yardstick_and_loop(gates, seqs, omega, names, seed):
    """Every sequence, every kind of spectrum: the new call against the yardstick under the project's bars and
    within twice the loop's own error; F and the total propagators against the yardstick and the loop."""
    yard = Yardstick(gates, omega)
    idx = ff.util.get_indices_from_identifiers(gates[0].n_oper_identifiers, names)
    refs = [yard.sequence([int(k) % len(gates) for k in s]) for s in seqs]
    bars = [LONG if len(s) >= 500 else TIGHT for s in seqs]
    pulses = None
    for S in spectra(len(idx), omega, seed):
        got, U, F = ff.sequence_infidelities(gates, seqs, S, omega, n_oper_identifiers=names, return_propagators=True,
                                             return_filter_functions=True)
        looped, pulses = loop(gates, seqs, S, omega, names)
        assert got.shape == looped.shape == (len(seqs),) + (len(idx),)*(2 if np.ndim(S) == 3 else 1)
        assert U.flags.owndata and F.flags.owndata and U.flags.writeable and F.flags.writeable
        for j, (R_ref, F_ref, U_ref) in enumerate(refs):
            ref = yard.infidelity(F_ref, S, idx)
            new, old = rel_err(got[j], ref), rel_err(looped[j], ref)
            print(f'W={len(omega)} A={len(gates[0].n_opers)} T={len(gates)} G={len(seqs[j])} S.ndim={np.ndim(S)}: '
                  f'infidelity new {new:.2e} loop {old:.2e}')
            WORST.update(new=max(WORST['new'], new), loop=max(WORST['loop'], old))
            assert new < bars[j], (j, new)
            assert new <= max(2e-13, 2*old), (j, new, old)
    for j, (R_ref, F_ref, U_ref) in enumerate(refs):
        F_loop = pulses[j].get_filter_function(omega)
        new, old = rel_err(F[j], F_ref), rel_err(F_loop, F_ref)
        print(f'G={len(seqs[j])}: F new {new:.2e} loop {old:.2e}, U new {rel_err(U[j], U_ref):.2e}')
        WORST.update(new=max(WORST['new'], new), loop=max(WORST['loop'], old))
        assert new < bars[j], (j, new)
        assert new <= max(2e-13, 2*old), (j, new, old)
        assert rel_err(U[j], U_ref) < bars[j], j
        assert rel_err(F[j], F_loop) < 1e-12 and rel_err(U[j], pulses[j].total_propagator) < 1e-12, j
        # the mirror and the real diagonal
        assert np.array_equal(F[j], F[j].conj().swapaxes(0, 1))
    print(f'worst so far: new {WORST["new"]:.2e}, loop {WORST["loop"]:.2e}')


LENGTHS = [1, 2, 3, 63, 64, 65, 130]


@pytest.mark.parametrize('W, A, T, pauli', [(7, 1, 3, True), (64, 2, 3, False), (65, 3, 3, True), (70, 4, 3, False),
                                            (70, 1, 40, False), (65, 2, 40, True), (64, 3, 40, False),
                                            (7, 4, 40, True)])
def test_two_qubit_gates_against_extended_precision(W, A, T, pauli):
    """T = 3: the tables staged in LDS; T = 40: read from L2.  W: a partial tile of 16 frequencies, a full wavefront,
    one frequency past it, a partial second block."""
    omega = wl.rb_omega(W, 1.0, m_max=3)
    gates = two_qubit_gates(T, A, omega, seed=10*W + A, basis=ff.Basis.pauli(2) if pauli else None)
    assert len(gates[0].basis) == 16 and gates[0].d == 4
    seqs = draws(LENGTHS, W + T, T)
    seqs[2] = np.array([-1, 0, -T])                       # negative indices wrap
    names = None if A == 1 else [NAMES[A - 1], NAMES[0]]    # a subset, not in sorted order
    check_against_yardstick_and_loop(gates, seqs, omega, names, seed=W)


def test_a_thousand_two_qubit_gates():
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(40, 1, omega, seed=5)
    check_against_yardstick_and_loop(gates, draws([1000, 500], 1, 40), omega, None, seed=2)


def test_single_qubit_gates_against_extended_precision():
    omega = wl.rb_omega(70, wl.CONFIG3['T'])
    _, cliffords = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])
    check_against_yardstick_and_loop(cliffords, draws([1, 2, 65, 152], 3, 24), omega, None, seed=3)


# ---- the route really taken ----------------------------------------------------------------------------------------
def test_route_really_taken(monkeypatch):
    omega = wl.rb_omega(40, 1.0, m_max=3)
    S = wl.rb_spectrum(omega, 0.7)
    _, cliffords = wl.rb_cliffords(ff, omega, 1.0)
    d4 = two_qubit_gates(3, 2, omega, seed=1)
    X, Z = ff.util.paulis[1], ff.util.paulis[3]
    spin1 = [ff.PulseSequence([[np.diag([1.0, 0.0, -1.0]), [0.3 + 0.1*k], 'Z']],
                              [[np.diag([1.0, -1.0, 0.0]), [1.0], 'N']], [1.0]) for k in range(2)]
    bare = ff.PulseSequence([[X/2, [0.4], 'X']], [[Z/2, [1.0], 'Z']], [1.0])
    five = two_qubit_gates(3, 5, omega, seed=2)
    for g in spin1 + [bare]:
        g.cache_control_matrix(omega)
    others = [(spin1, [[0, 1], [1, 1, 0]]), (list(cliffords[:3]) + [bare], [[0, 3], [1, 2, 3]]),
              (five, [[0, 1, 2], [2, 2]])]
    eligible = [(cliffords, draws([1, 2, 30], 1, 24)), (d4, draws([1, 2, 30], 2, 3))]
    expected = [loop(g, s, S, omega)[0] for g, s in eligible + others]

    def refuse(*args, **kwargs):
        raise AssertionError('the loop ran')
    with monkeypatch.context() as patch:
        patch.setattr(ff, 'concatenate', refuse)
        got = [ff.sequence_infidelities(g, s, S, omega) for g, s in eligible]
        for g, s in others:
            with pytest.raises(AssertionError, match='the loop ran'):
                ff.sequence_infidelities(g, s, S, omega)
    for value, ref in zip(got, expected):
        assert rel_err(value, ref) < 1e-13
    for (g, s), ref in zip(others, expected[2:]):
        value, U, F = ff.sequence_infidelities(g, s, S, omega, return_propagators=True, return_filter_functions=True)
        assert value.shape == ref.shape and rel_err(value, ref) < 1e-13
        pulses = loop(g, s, S, omega)[1]
        assert rel_err(U, [p.total_propagator for p in pulses]) < 1e-13
        assert rel_err(F, [p.get_filter_function(omega) for p in pulses]) < 1e-13


# ---- bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('A, T', [(1, 3), (2, 40), (4, 3)])
def test_a_sequence_does_not_depend_on_its_pass(A, T):
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(T, A, omega, seed=A)
    S = spectra(A, omega, 4)[2]
    probe = draws([77], 8, T)[0]
    others = draws(np.random.default_rng(1).integers(1, 140, 39), 9, T)
    kw = dict(return_propagators=True, return_filter_functions=True)
    alone = ff.sequence_infidelities(gates, [probe], S, omega, **kw)
    first = ff.sequence_infidelities(gates, [probe] + others, S, omega, **kw)
    last = ff.sequence_infidelities(gates, others + [probe], S, omega, **kw)
    # (another table as well: only the gates a pass uses are in it)
    for a, f, l in zip(alone, first, last):
        assert np.array_equal(a[0], f[0]) and np.array_equal(a[0], l[-1])


def test_resident_gates_and_host_arrays_give_the_same_bits():
    omega = wl.rb_omega(70, 1.0, m_max=3)
    S = wl.rb_spectrum(omega, 0.7)
    seqs = draws([1, 2, 17, 64, 100], 6, 4)
    single = two_qubit_gates(4, 2, omega, seed=3)                     # cache_control_matrix: single resident results
    assert all(resident_source(g, 4, 70, 16, 2)[1] == -1 for g in single)
    members = [ff.PulseSequence(list(zip(g.c_opers, g.c_coeffs, g.c_oper_identifiers)),
                                list(zip(g.n_opers, g.n_coeffs, g.n_oper_identifiers)), g.dt) for g in single]
    ff.get_filter_functions(members, omega)                           # members of batched passes (one per shape)
    assert sorted(resident_source(g, 4, 70, 16, 2)[1] for g in members) == [0, 0, 1, 1]
    kw = dict(return_propagators=True, return_filter_functions=True)
    for resident in (single, members):
        got = ff.sequence_infidelities(resident, seqs, S, omega, **kw)
        host = [ff.PulseSequence(list(zip(g.c_opers, g.c_coeffs, g.c_oper_identifiers)),
                                 list(zip(g.n_opers, g.n_coeffs, g.n_oper_identifiers)), g.dt) for g in resident]
        for h, g in zip(host, resident):
            h.cache_control_matrix(omega, np.array(g.get_control_matrix(omega)))
            h.total_propagator = np.array(g.total_propagator)
            assert resident_source(h, 4, 70, 16, 2) is None
        for a, b in zip(got, ff.sequence_infidelities(host, seqs, S, omega, **kw)):
            assert np.array_equal(a, b)
    # a mixed table: some rows uploaded, some read in place
    mixed = [single[0], host[1], members[2], host[3]]
    for a, b in zip(got, ff.sequence_infidelities(mixed, seqs, S, omega, **kw)):
        assert np.array_equal(a, b)


def test_single_qubit_results_are_those_of_the_sequence_pass():
    omega = wl.rb_omega(301, wl.CONFIG3['T'])
    _, cliffords = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])
    cliffords = np.array(cliffords, dtype=object)
    seqs = draws([2, 3, 64, 65, 152, 400], 12, 24)
    pulses = ff.concatenate_sequences([cliffords[s] for s in seqs])
    for S in (wl.rb_spectrum(omega, 0.0), wl.rb_spectrum(omega, 0.7)):
        got, U, F = ff.sequence_infidelities(cliffords, seqs, S, omega, return_propagators=True,
                                             return_filter_functions=True)
        assert np.array_equal(got, ff.infidelities(pulses, S, omega))
    for j, p in enumerate(pulses):
        assert np.array_equal(F[j], p.get_filter_function(omega))
        assert np.array_equal(U[j], p.total_propagator)


# ---- other cases ---------------------------------------------------------------------------------------------------
def test_one_frequency_gives_zeros():
    omega = np.array([0.5])
    X = ff.util.paulis[1]
    single = [ff.PulseSequence([[X/2, [0.3 + 0.1*k], 'X']], [[X/2, [1.0], 'X']], [1.0]) for k in range(3)]
    for g in single:
        g.cache_control_matrix(omega)
    for gates in (two_qubit_gates(3, 2, omega, seed=1), single):
        got = ff.sequence_infidelities(gates, [[0, 1], [2]], np.ones(1), omega)
        assert got.shape == (2, len(gates[0].n_opers)) and not got.any()
        got, U = ff.sequence_infidelities(gates, [[0, 1], [2]], np.ones(1), omega, return_propagators=True)
        assert not got.any() and rel_err(U[0], gates[1].total_propagator @ gates[0].total_propagator) < 1e-14


def test_indices_exceptions_and_caches():
    omega = wl.rb_omega(20, 1.0, m_max=3)
    S = wl.rb_spectrum(omega, 0.7)
    gates = two_qubit_gates(4, 1, omega, seed=7)
    caches = lambda: [(sorted(g._data), sorted(g._frequency_data),                       # noqa: E731
                       {k: id(g._frequency_data.peek(k)) for k in g._frequency_data}) for g in gates]
    before = caches()
    got = ff.sequence_infidelities(gates, [[-1, 0, -4], [3, 0, 0]], S, omega)
    assert caches() == before
    assert np.array_equal(got[0], got[1])                                                # negative indices wrap
    with pytest.raises(IndexError):
        ff.sequence_infidelities(gates, [[0, 4]], S, omega)
    with pytest.raises(IndexError):
        ff.sequence_infidelities(gates, [[-5]], S, omega)
    with pytest.raises(ValueError):
        ff.sequence_infidelities(gates, [[0], []], S, omega)
    with pytest.raises(TypeError):
        ff.sequence_infidelities(gates, [[0.0, 1.0]], S, omega)
    # the loop's messages for a spectrum that does not fit the grid and for unknown identifiers
    for kwargs in (dict(spectrum=np.ones(7)), dict(spectrum=S, n_oper_identifiers=['Q'])):
        with pytest.raises(ValueError) as loop_error:
            loop(gates, [[0, 1]], kwargs['spectrum'], omega, kwargs.get('n_oper_identifiers'))
        with pytest.raises(ValueError) as error:
            ff.sequence_infidelities(gates, [[0, 1]], omega=omega, **kwargs)
        assert str(error.value) == str(loop_error.value)
    # gates without a control matrix on the grid are completed by one batched call, then read in place
    fresh = [ff.PulseSequence(list(zip(g.c_opers, g.c_coeffs, g.c_oper_identifiers)),
                              list(zip(g.n_opers, g.n_coeffs, g.n_oper_identifiers)), g.dt) for g in gates]
    assert rel_err(ff.sequence_infidelities(fresh, [[3, 0, 0], [1, 2]], S, omega),
                   ff.sequence_infidelities(gates, [[3, 0, 0], [1, 2]], S, omega)) < 1e-13
    assert all(g.is_cached('control_matrix') and g.is_cached('filter_function') for g in fresh)
    assert all(resident_source(g, 4, 20, 16, 1) is not None for g in fresh)


def test_bad_csr_through_the_c_entry():
    """FFK_EINVAL before anything touches the device; the stream stays usable."""
    omega = np.ascontiguousarray(wl.rb_omega(20, 1.0, m_max=3))
    gate = two_qubit_gates(1, 1, omega, seed=9)[0]
    lib = _lib.load()
    U = np.ascontiguousarray(gate.total_propagator[None], dtype=np.complex128)
    table = np.ascontiguousarray(gate.get_control_matrix(omega)[None], dtype=np.complex128)
    tau = np.array([gate.tau])
    basis = np.ascontiguousarray(np.asarray(gate.basis), dtype=np.complex128)
    S = np.ascontiguousarray(wl.rb_spectrum(omega, 0.7))
    idx = np.zeros(1, dtype=np.int32)
    gates = (ctypes.c_void_p*1)(None)
    slots = np.array([-1], dtype=np.int32)
    out = np.full((2, 1), -1.0)

    def call(offsets, index):
        offsets = np.asarray(offsets, dtype=np.int32)
        index = np.asarray(index, dtype=np.int32)
        return lib.ffk_sequence_infidelities(
            gates, slots.ctypes.data, table.ctypes.data, U.ctypes.data, tau.ctypes.data, 1, offsets.ctypes.data,
            index.ctypes.data, len(offsets) - 1, omega.ctypes.data, len(omega), basis.ctypes.data, 1, 4, 1, 16,
            S.ctypes.data, 1, 1, idx.ctypes.data, 1, 4, out.ctypes.data, None, None)
    assert call([0, 2, 3], [0, 1, 0]) == _lib.FFK_EINVAL
    assert 'index' in lib.ffk_last_error().decode()
    assert call([0, 2, 1], [0, 0, 0]) == _lib.FFK_EINVAL
    assert call([1, 2, 3], [0, 0, 0]) == _lib.FFK_EINVAL
    assert (out == -1.0).all()
    assert call([0, 2, 3], [0, 0, 0]) == 0
    assert rel_err(out, ff.sequence_infidelities([gate], [[0, 0], [0]], S, omega)) == 0

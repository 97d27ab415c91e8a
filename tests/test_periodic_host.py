"""CPU side of the periodic-driving pass (ff.periodic_*, ffk_periodic_dev / ffk_resident_periodic): public names, the
ABI in header, exports and binding, the workspace query without a GPU, the refusals of the entries before the device,
routing and pass splitting with the entry replaced by a stand-in, the loop's exceptions, the eigensystem helper where
eigenphases coincide, and the closed form in NumPy (periodic_yardstick.py) against the oracle."""
import ctypes

import numpy as np
import pytest

import ff_oracle as orc
import filter_functions_amd as ff
import periodic_yardstick as yard
from conftest import rel_err
from filter_functions_amd import _lib, batch, periodic

ENTRIES = ('ffk_periodic_workspace_bytes', 'ffk_periodic_dev', 'ffk_resident_periodic')
PAULI = np.array([[[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]], dtype=complex)


def test_public_names():
    for name in periodic.__all__:
        assert name in ff.__all__ and getattr(ff, name) is getattr(periodic, name)
    assert ff.periodic is periodic and 'periodic' in ff.__all__
    assert set(periodic.__all__) == {'periodic_filter_functions', 'periodic_infidelities',
                                     'periodic_decay_amplitudes'}


def test_binding_header_and_exports_agree():
    import test_abi
    names = test_abi.header_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in names and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES[ENTRIES[0]] == (ctypes.c_size_t, [ctypes.c_int]*9)
    assert len(_lib.SIGNATURES[ENTRIES[1]][1]) == 22 and len(_lib.SIGNATURES[ENTRIES[2]][1]) == 21


def test_workspace_query_needs_no_gpu():
    q = _lib.load().ffk_periodic_workspace_bytes
    # (P, K, n_host, A, W, d, n_idx, s_ndim, stage)
    for P, K, n_host, A, W, d, n_idx, s_ndim, stage in [(64, 25, 0, 1, 500, 2, 1, 1, 2), (16, 25, 16, 3, 500, 4, 3, 2, 3),
                                                         (3, 5, 1, 2, 33, 3, 2, 1, 1), (1, 1, 0, 1, 2, 2, 1, 1, 3)]:
        need = q(P, K, n_host, A, W, d, n_idx, s_ndim, stage)
        out = 8*periodic.out_elements(stage, K, n_idx, W, d*d)*P
        assert need >= out + 16*A*d*d*W*n_host
        # what the Python side counts per pass covers it, and not by much
        counted = (periodic.fixed_bytes(stage, K, A, d*d, W, d, n_idx, s_ndim)
                   + P*periodic.member_bytes(stage, K, A, d*d, W, d, n_idx, n_host > 0))
        assert need <= counted <= need + 16*A*d*d*W*(P - n_host)*(n_host > 0) + 16*256, (P, K, stage)
    good = (4, 5, 0, 2, 33, 2, 2, 1, 2)
    assert q(*good) > 0
    for at, bad in [(0, 0), (0, 65536), (1, 0), (1, 65536), (2, -1), (2, 5), (3, 0), (4, 0), (4, 1), (5, 1), (5, 5),
                    (6, 0), (6, 3), (7, 3), (7, 0), (8, 0), (8, 4)]:
        args = list(good)
        args[at] = bad
        assert q(*args) == 0, (at, bad)
    assert q(4, 5, 0, 2, 1, 2, 2, 0, 1) > 0          # filter functions need no spectrum and take one frequency


def _host_call(**change):
    P, A, W, d, K, n_idx = 2, 2, 5, 2, 3, 2
    keep = dict(handles=(ctypes.c_void_p*P)(), slots=np.full(P, -1, dtype=np.int32),
                table=np.zeros((P, A, d*d, W), dtype=complex), omega=np.linspace(0, 1, W),
                basis=np.zeros((d*d, d, d), dtype=complex), V=np.zeros((P, d, d), dtype=complex),
                phi=np.zeros((P, d, d, 2)), T=np.ones(P), repeats=np.array([1, 2, 3], dtype=np.int32),
                S=np.ones(W, dtype=complex), idx=np.arange(n_idx, dtype=np.int32), out=np.zeros((P, K, n_idx)))
    a = dict(P=P, A=A, W=W, d=d, K=K, s_ndim=1, n_idx=n_idx, d_inf=d, stage=2)
    a.update({k: v for k, v in change.items() if k in a})
    for k, v in change.items():
        if k in keep:
            keep[k] = v

    def at(x):
        return None if x is None else (x if isinstance(x, ctypes.Array) else x.ctypes.data)
    host = (at(keep['handles']), at(keep['slots']), at(keep['table']), a['P'], a['A'], a['W'], a['d'],
            at(keep['omega']), at(keep['basis']), at(keep['V']), at(keep['phi']), at(keep['T']), at(keep['repeats']),
            a['K'], at(keep['S']), a['s_ndim'], at(keep['idx']), a['n_idx'], a['d_inf'], a['stage'], at(keep['out']))
    dev = host[2:3] + host[3:] + (None, 0, None)
    return host, dev, keep


def test_bad_arguments_are_refused_before_the_device():
    lib = _lib.load()
    cases = [(dict(omega=None), 'NULL'), (dict(out=None), 'NULL'), (dict(V=None), 'NULL'), (dict(repeats=None), 'NULL'),
             (dict(P=0), 'unsupported shape'), (dict(K=0), 'unsupported shape'), (dict(d=5), 'unsupported shape'),
             (dict(d=1), 'unsupported shape'), (dict(n_idx=3), 'unsupported shape'), (dict(stage=4), 'unsupported shape'),
             (dict(s_ndim=3), 'unsupported shape'), (dict(W=1), 'unsupported shape'), (dict(S=None), 'needs a spectrum'),
             (dict(d_inf=0), 'needs a spectrum')]
    for change, message in cases:
        host, dev, keep = _host_call(**change)
        for entry, args in ((lib.ffk_resident_periodic, host), (lib.ffk_periodic_dev, dev)):
            assert entry(*args) == _lib.FFK_EINVAL, change
            assert message in lib.ffk_last_error().decode(), (change, lib.ffk_last_error().decode())
    # what only the host-pointer entry can read: a repeat count below 1, an operator index out of range
    for change, message in [(dict(repeats=np.array([1, 0, 3], dtype=np.int32)), 'repeats[1] = 0'),
                            (dict(idx=np.array([0, 2], dtype=np.int32)), 'idx[1] = 2')]:
        host, _, keep = _host_call(**change)
        assert lib.ffk_resident_periodic(*host) == _lib.FFK_EINVAL
        assert message in lib.ffk_last_error().decode()


# ---- routing, with the entry replaced by a stand-in -----------------------------------------------------------------
def host_pulse(rng, d, omega, A=2, U=None):
    """A pulse whose caches hold a host control matrix on *omega* and a total propagator: nothing here needs a GPU."""
    n = {2: 1, 4: 2}.get(d)
    basis = ff.Basis.ggm(d) if n is None else ff.Basis.pauli(n)
    herm = lambda: (lambda m: m + m.conj().T)(rng.normal(size=(d, d)) + 1j*rng.normal(size=(d, d)))   # noqa: E731
    pulse = ff.PulseSequence([[herm(), rng.normal(size=3)]], [[herm(), np.ones(3)] for _ in range(A)],
                             rng.uniform(0.5, 1.5, 3), basis)
    if U is None:
        w, v = np.linalg.eigh(herm())
        U = (v*np.exp(-1j*w)) @ v.conj().T
    pulse.total_propagator = U
    R = rng.normal(size=(A, len(basis), len(omega))) + 1j*rng.normal(size=(A, len(basis), len(omega)))
    pulse.cache_control_matrix(omega, R)
    return pulse


class StandIn:
    """Records every call of ffk_resident_periodic and fills `out` with the pass's number."""

    def __init__(self):
        self.calls = []

    def ffk_resident_periodic(self, handles, slots, table, P, A, W, d, omega, basis, V, phi, T, repeats, K, S, s_ndim,
                              idx, n_idx, d_inf, stage, out):
        n = periodic.out_elements(stage, K, n_idx, W, d*d)*P
        np.ctypeslib.as_array((ctypes.c_double*n).from_address(out))[:] = len(self.calls)
        self.calls.append(dict(P=P, K=K, d=d, A=A, stage=stage, s_ndim=s_ndim, n_idx=n_idx, hosts=table is not None,
                               handles=[h for h in handles]))
        return _lib.FFK_OK


@pytest.fixture
def stand_in(monkeypatch):
    fake = StandIn()
    monkeypatch.setattr(periodic._lib, 'load', lambda: fake)
    return fake


def test_routing_groups_by_shape_and_splits_under_the_budget(stand_in, monkeypatch):
    rng = np.random.default_rng(3)
    omega = np.linspace(0, 5, 9)
    pulses = [host_pulse(rng, 2, omega), host_pulse(rng, 4, omega, A=3), host_pulse(rng, 2, omega),
              host_pulse(rng, 3, omega), host_pulse(rng, 2, omega)]
    repeats = [1, 4, 9]
    F = ff.periodic_filter_functions(pulses[:1] + pulses[2:3] + pulses[4:], repeats, omega)
    assert F.shape == (3, 3, 2, 9) and len(stand_in.calls) == 1
    assert stand_in.calls[0]['P'] == 3 and stand_in.calls[0]['stage'] == 1 and stand_in.calls[0]['hosts']
    assert stand_in.calls[0]['handles'] == [None]*3
    del stand_in.calls[:]
    # three shapes: three passes, the results back in input order
    with pytest.raises(ValueError, match='same output shape'):
        ff.periodic_infidelities(pulses, repeats, np.ones(9), omega)
    same = [pulses[0], pulses[2], pulses[4]]
    out = ff.periodic_infidelities(same + [host_pulse(rng, 2, omega)], repeats, np.ones(9), omega)
    assert out.shape == (4, 3, 2) and [c['P'] for c in stand_in.calls] == [4]
    assert stand_in.calls[0]['stage'] == 2 and stand_in.calls[0]['s_ndim'] == 1
    del stand_in.calls[:]
    # a budget of two members: passes of two, one and ... (batch.split_passes: sizes differ by one at most)
    per = periodic.member_bytes(3, 3, 2, 4, 9, 2, 2, True)
    fixed = periodic.fixed_bytes(3, 3, 2, 4, 9, 2, 2, 2)
    monkeypatch.setattr(batch, 'PASS_BYTES', fixed + 2*per)
    five = same + [host_pulse(rng, 2, omega), host_pulse(rng, 2, omega)]
    gamma = ff.periodic_decay_amplitudes(five, repeats, np.ones((2, 9)), omega)
    assert gamma.shape == (5, 3, 2, 4, 4)
    assert [c['P'] for c in stand_in.calls] == [1, 2, 2] and all(c['stage'] == 3 for c in stand_in.calls)
    assert [gamma[i, 0, 0, 0, 0] for i in range(5)] == [0, 1, 1, 2, 2]


def test_what_the_batched_route_does_not_take(stand_in, monkeypatch):
    """Cross-spectra, a complex spectrum, an incomplete basis, a non-unitary propagator: the loop's expression."""
    rng = np.random.default_rng(4)
    omega = np.linspace(0, 5, 9)
    pulses = [host_pulse(rng, 2, omega), host_pulse(rng, 2, omega)]
    seen = []
    monkeypatch.setattr(periodic, '_single', lambda stage, pulse, n, *args: seen.append((stage, n)) or np.zeros(2))
    cross = np.ones((2, 2, 9))
    assert ff.periodic_infidelities(pulses, [1, 2], cross, omega).shape == (2, 2, 2)
    assert not stand_in.calls and seen == [(2, 1), (2, 2)]*2
    del seen[:]
    ff.periodic_infidelities(pulses, [3], np.ones(9)*(1 + 1j), omega)
    assert not stand_in.calls and seen == [(2, 3)]*2
    del seen[:]
    pulses[1].total_propagator = np.array([[1, 1], [0, 1]], dtype=complex)      # not normal: a residue is left
    ff.periodic_infidelities(pulses, [3], np.ones(9), omega)
    assert [c['P'] for c in stand_in.calls] == [1] and seen == [(2, 3)]
    assert periodic._eligible(pulses[0])
    partial = ff.Basis(np.asarray(ff.Basis.pauli(1))[:3])
    assert not periodic._eligible(type('P', (), dict(basis=partial, n_opers=np.zeros((1, 2, 2))))())


def test_the_loops_exceptions(stand_in):
    rng = np.random.default_rng(5)
    omega = np.linspace(0, 5, 9)
    pulses = [host_pulse(rng, 2, omega)]
    with pytest.raises(TypeError, match='Can only concatenate PulseSequences'):
        ff.periodic_filter_functions(pulses + ['pulse'], [1], omega)
    for bad in ([0], [3, -1], [[1, 2]]):
        with pytest.raises(ValueError):
            ff.periodic_infidelities(pulses, bad, np.ones(9), omega)
    with pytest.raises(TypeError):
        ff.periodic_infidelities(pulses, [1.5], np.ones(9), omega)
    with pytest.raises(ValueError, match='Spectrum should be of shape'):
        ff.periodic_infidelities(pulses, [2], np.ones(8), omega)
    with pytest.raises(ValueError, match='Spectrum should be of shape'):
        ff.periodic_decay_amplitudes(pulses, [2], np.ones((3, 9)), omega)
    with pytest.raises(ValueError):
        ff.periodic_infidelities(pulses, [2], np.ones(9), omega, n_oper_identifiers=['nope'])
    assert not stand_in.calls
    for f, args in ((ff.periodic_filter_functions, ()), (ff.periodic_infidelities, (np.ones(9),))):
        out = f([], [1, 2], *args, omega)
        assert out.shape == (0,) and out.dtype == np.float64


# ---- the eigensystem where eigenphases coincide ---------------------------------------------------------------------
def _random_unitary(rng, d):
    q, r = np.linalg.qr(rng.normal(size=(d, d)) + 1j*rng.normal(size=(d, d)))
    return q*(np.diag(r)/np.abs(np.diag(r)))


def test_eigensystem_returns_a_unitary_where_phases_coincide():
    rng = np.random.default_rng(6)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    pi_rotation = -1j*np.einsum('i,ijk->jk', axis, PAULI)                       # exp(-i pi/2 n.sigma)
    frame = _random_unitary(rng, 4)
    degenerate = (frame*np.exp(1j*np.array([0.3, 0.3, 1.1, -2.0]))) @ frame.conj().T
    for U in (np.eye(2), -np.eye(2), pi_rotation, degenerate, np.eye(4), -np.eye(3)):
        V, phi, residue = periodic.eigensystem(U)
        d = len(U)
        assert np.abs(V.conj().T @ V - np.eye(d)).max() <= 1e-14
        assert residue <= 1e-14
        assert np.abs(U - (V*np.exp(1j*phi)) @ V.conj().T).max() == residue
        assert phi.dtype == np.float64 and np.all(np.abs(phi) <= np.pi)
    assert sorted(np.round(periodic.eigensystem(degenerate)[1], 12)) == [-2.0, 0.3, 0.3, 1.1]
    # the yardstick's own helper is the same decomposition
    V, phi = yard.eigensystem(degenerate)
    assert np.abs(degenerate - (V*np.exp(1j*phi)) @ V.conj().T).max() <= 1e-14


# ---- the closed form against the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize('d', [2, 3, 4])
def test_closed_form_against_the_oracle(d):
    """The project's parity contract (1e-10, as test_control_matrix_periodic_by_doubling) for the closed form in
    NumPy: generic phases, resonances w T = phi_j - phi_k on the grid, a two-fold degenerate eigenphase."""
    rng = np.random.default_rng(10 + d)
    basis = orc.basis_ggm(3) if d == 3 else orc.basis_pauli(d//2)
    T = 1.7
    phases = rng.uniform(-np.pi, np.pi, d)
    phases[1] = phases[0] if d > 2 else phases[1]                               # a degenerate pair
    frame = _random_unitary(rng, d)
    U = (frame*np.exp(1j*phases)) @ frame.conj().T
    resonances = np.mod(phases[:, None] - phases[None, :], 2*np.pi).ravel()/T
    omega = np.sort(np.concatenate([[0.0, 1e-10], resonances[resonances > 0][:4], rng.uniform(0, 25, 20)]))
    R1 = rng.normal(size=(2, d*d, len(omega))) + 1j*rng.normal(size=(2, d*d, len(omega)))
    L = orc.liouville_representation(U, basis)
    for n in (1, 2, 3, 7, 1000):
        ref = orc.control_matrix_periodic(orc.cexp(omega*T), R1, L, n)
        got = yard.closed_form_control_matrix(R1, basis, U, T, omega, n)
        assert rel_err(got, ref) < 1e-10, n
        F = yard.closed_form_filter_function(R1, basis, U, T, omega, n)
        assert rel_err(F, yard.filter_function_of(ref)) < 1e-10, n


def test_extended_precision_series_against_the_closed_form():
    """The 60-digit yardstick of the GPU tests: at n = 1 it is R1 itself, and it agrees with the closed form to what
    double precision allows at n = 1000 (n eps w T of the phase)."""
    rng = np.random.default_rng(20)
    basis = orc.basis_pauli(1)
    U = _random_unitary(rng, 2)
    T, omega = 0.9, np.array([0.0, 1e-10, 0.7, 13.0])
    R1 = rng.normal(size=(1, 4, 4)) + 1j*rng.normal(size=(1, 4, 4))
    exact = yard.series_control_matrices_mp(R1, basis, U, T, omega, [1, 7, 1000])
    assert rel_err(exact[1], R1) < 4e-16
    for n in (7, 1000):
        assert rel_err(yard.closed_form_control_matrix(R1, basis, U, T, omega, n), exact[n]) < 1e-11, n

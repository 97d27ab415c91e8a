"""Batched filter functions and infidelities (ff.get_filter_functions / ff.infidelities): many pulses of one
shape in one pass, against the golden fixtures and against the single-pulse path, pulse by pulse."""
import copy

import numpy as np
import pytest

import filter_functions_amd as ff
import workloads as wl
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

TIGHT = 2e-13
NAMES = ['rand_d2_ggm', 'rand_d3_ggm', 'rand_d4_pauli', 'rand_d8_pauli', 'rand_d16_ggm', 'hadamard', 'cfg2_small']


def pulse_from(g, c_coeffs=None, dt=None):
    basis = ff.Basis(g['basis'], btype=str(g['btype']))
    G = len(g['dt'] if dt is None else dt)
    return ff.PulseSequence.from_arrays(g['c_opers'], g['c_oper_identifiers'],
                                        g['c_coeffs'] if c_coeffs is None else c_coeffs,
                                        g['n_opers'], g['n_oper_identifiers'], np.asarray(g['n_coeffs'])[:, :G],
                                        g['dt'] if dt is None else dt, basis)


def family(g, P=5, seed=0):
    """The fixture pulse and P - 1 seeded perturbations of its amplitudes and durations."""
    rng = np.random.default_rng(seed)
    c, dt = np.asarray(g['c_coeffs'], dtype=float), np.asarray(g['dt'], dtype=float)
    out = [(c, dt)]
    for _ in range(P - 1):
        out.append((c*(1 + 0.05*rng.standard_normal(c.shape)), dt*(1 + 0.05*rng.random(dt.shape))))
    return out


def build(g, members):
    return [pulse_from(g, c, dt) for c, dt in members]


@pytest.mark.parametrize('name', NAMES)
def test_batch_matches_golden_and_single_path(name):
    g = load_golden(name)
    omega = g['omega']
    members = family(g)
    pulses = build(g, members)
    F = ff.get_filter_functions(pulses, omega)
    A = len(g['n_opers'])
    assert F.shape == (5, A, A, len(omega)) and F.dtype == np.complex128
    # the fixture member against the reference's numbers
    assert rel_err(F[0], g['filter_function']) < 1e-12
    assert rel_err(pulses[0].get_control_matrix(omega), g['control_matrix']) < 1e-12
    assert rel_err(pulses[0].propagators, g['propagators']) < 1e-12
    # every member against a fresh single-pulse call on an identical pulse
    for p, pulse in enumerate(pulses):
        single = build(g, [members[p]])[0]
        assert rel_err(F[p], single.get_filter_function(omega)) < TIGHT, p
        assert rel_err(pulse.get_control_matrix(omega), single.get_control_matrix(omega)) < TIGHT, p
        assert rel_err(pulse.propagators, single.propagators) < TIGHT, p
        scale = max(1.0, np.abs(single.eigvals).max())
        assert np.abs(pulse.eigvals - single.eigvals).max() < 1e-13*scale, p
    if 'infidelity_S1' in g:
        for key in ('S1', 'S2', 'S3'):
            got = ff.infidelities(build(g, members), g[key], omega)
            assert got.shape == (5,) + g['infidelity_' + key].shape and got.dtype == np.float64
            assert rel_err(got[0], g['infidelity_' + key]) < 1e-12, key
            for p in range(5):
                want = ff.infidelity(build(g, [members[p]])[0], g[key], omega)
                assert rel_err(got[p], want) < TIGHT, (key, p)
        if 'subset_identifiers' in g:
            ids = [str(s) for s in g['subset_identifiers']]
            got = ff.infidelities(build(g, members), g['S1'], omega, n_oper_identifiers=ids)
            assert rel_err(got[0], g['infidelity_S1_subset']) < 1e-12
            for p in range(5):
                want = ff.infidelity(build(g, [members[p]])[0], g['S1'], omega, n_oper_identifiers=ids)
                assert rel_err(got[p], want) < TIGHT, p


def test_no_cross_talk_between_pulses():
    g = load_golden('rand_d4_pauli')
    omega = g['omega']
    members = family(g, P=6, seed=3)
    F = ff.get_filter_functions(build(g, members), omega)
    R = ff.get_filter_functions(build(g, members[::-1]), omega)
    assert np.array_equal(F, R[::-1])
    S = 1e-3*np.exp(-(omega/np.abs(omega).max())**2)       # (finite: these grids contain 0)
    assert np.array_equal(ff.infidelities(build(g, members), S, omega),
                          ff.infidelities(build(g, members[::-1]), S, omega)[::-1])
    hadamard = [wl.hadamard_pulse(ff) for _ in range(64)]
    omega = np.geomspace(1e-2, 1e2, 400)
    F = ff.get_filter_functions(hadamard, omega)
    assert all(np.array_equal(F[0], F[p]) for p in range(64))


def test_caches_after_a_batch():
    g = load_golden('cfg2_small')
    omega = g['omega']
    members = family(g, P=4, seed=1)
    pulses = build(g, members)
    F = ff.get_filter_functions(pulses, omega)
    assert not F.flags.writeable
    for p, pulse in enumerate(pulses):
        cached = pulse.get_filter_function(omega)
        assert pulse.get_filter_function(omega) is cached
        assert np.shares_memory(cached, F[p]) and np.array_equal(cached, F[p])
        assert not cached.flags.writeable
        assert pulse.is_cached('control matrix') and pulse.is_cached('filter function')
        assert pulse.is_cached('eigvals') and pulse.is_cached('total propagator')
        single = build(g, [members[p]])[0]
        assert rel_err(pulse.get_control_matrix(omega), single.get_control_matrix(omega)) < TIGHT
        assert rel_err(pulse.total_propagator_liouville, single.total_propagator_liouville) < 1e-13
        assert rel_err(pulse.get_total_phases(omega), single.get_total_phases(omega)) < 1e-15
        S2 = np.outer(np.arange(1, len(g['n_opers']) + 1), 1e-3/omega)
        assert rel_err(ff.infidelity(pulse, S2, omega), ff.infidelity(single, S2, omega)) < TIGHT
        writable = pulse.get_filter_function(omega, writable=True)
        assert writable.flags.writeable and np.array_equal(writable, F[p])
    # copies own host arrays; cleanup drops what it drops for a resident pulse
    twin = copy.deepcopy(pulses[1])
    assert twin._resident is None and np.array_equal(twin.get_filter_function(omega), F[1])
    assert np.array_equal(twin.get_control_matrix(omega), pulses[1].get_control_matrix(omega))
    pulses[2].cleanup('all')
    assert not pulses[2].is_cached('filter function') and pulses[2]._resident is None
    assert rel_err(pulses[2].get_filter_function(omega), F[2]) < TIGHT
    # the other members keep the batch alive
    del pulses[0], F
    assert pulses[0].get_control_matrix(omega).shape[0] == len(g['n_opers'])


def test_mixed_list_keeps_input_order():
    g4, g2 = load_golden('edge_degenerate_d4'), load_golden('rand_d2_ggm')
    A = len(g4['n_opers'])
    assert len(g2['n_opers']) == A
    omega = g4['omega']
    S = 1e-3*np.exp(-(omega/np.abs(omega).max())**2)       # (finite: these grids contain 0)
    m4, m2 = family(g4, P=4, seed=5), family(g2, P=3, seed=6)
    short = [(c[:, :-1], dt[:-1]) for c, dt in family(g4, P=2, seed=7)]      # another G
    make = lambda: ([pulse_from(g4, *m4[0]), pulse_from(g2, *m2[0]), pulse_from(g4, *short[0]),   # noqa: E731
                     pulse_from(g4, *m4[1]), pulse_from(g2, *m2[1]), pulse_from(g4, *short[1]),
                     pulse_from(g4, *m4[2]), pulse_from(g2, *m2[2]), pulse_from(g4, *m4[3])])
    pulses = make()
    pulses[3].get_control_matrix(omega)            # something cached: the single route
    got = ff.infidelities(pulses, S, omega)
    want = np.array([ff.infidelity(p, S, omega) for p in make()])
    assert got.shape == want.shape
    assert rel_err(got, want) < TIGHT
    pulses = make()
    pulses[3].get_control_matrix(omega)
    F = ff.get_filter_functions(pulses, omega)
    assert rel_err(F, np.array([p.get_filter_function(omega) for p in make()])) < TIGHT
    assert ff.get_filter_functions([], omega).shape == (0,)
    assert ff.infidelities([], S, omega).dtype == np.float64
    # shape mismatches
    other = pulse_from(load_golden('rand_d4_pauli'))          # three noise operators
    assert len(other.n_opers) != A
    with pytest.raises(ValueError):
        ff.get_filter_functions([pulse_from(g4), other], omega)
    with pytest.raises(ValueError):
        ff.infidelities([pulse_from(g4), pulse_from(load_golden('rand_d4_pauli'))], S, omega)
    with pytest.raises(ValueError):
        ff.infidelities([pulse_from(g4), pulse_from(g4)], S, omega, n_oper_identifiers=['not an identifier'])
    with pytest.raises(ValueError):
        ff.infidelities([pulse_from(g4)], S, omega, which='nonsense')


def test_non_converging_member_is_named():
    c_opers, c_coeffs, n_opers, n_coeffs, dt = wl.random_pulse_inputs(seed=1, d=2, G=12, A=2, n_cops=2)
    omega = wl.random_pulse_omega(dt, 64)
    basis = ff.Basis.pauli(1)

    def make(bad):
        c = c_coeffs.copy()
        if bad:
            c[0, 5] = np.nan
        return ff.PulseSequence(list(zip(c_opers, c)), list(zip(n_opers, n_coeffs)), dt, basis)
    pulses = [make(p == 3) for p in range(6)]
    with pytest.raises(np.linalg.LinAlgError, match='pulse 3'):
        ff.infidelities(pulses, 1e-3/omega, omega)
    assert not any(p.is_cached('filter function') for p in pulses)
    pulses = [make(p == 3) for p in range(6)]
    with pytest.raises(np.linalg.LinAlgError, match='pulse 3'):
        ff.get_filter_functions(pulses, omega)
    assert not any(p.is_cached('filter function') for p in pulses)
    # the library is fine afterwards
    good = [make(False) for _ in range(3)]
    assert ff.get_filter_functions(good, omega).shape == (3, 2, 2, 64)


def test_config2_full_size():
    omega = None
    singles, pulses = [], []
    basis = ff.Basis.pauli(2)
    for seed in range(8):
        cfg = dict(wl.CONFIG2, seed=100 + seed)
        c_opers, c_coeffs, n_opers, n_coeffs, dt = wl.random_pulse_inputs(**cfg)
        if omega is None:
            omega = wl.random_pulse_omega(dt, cfg['W'])
        for out in (singles, pulses):
            out.append(ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt, basis))
    S = 1e-3*np.exp(-(omega/np.abs(omega).max())**2)       # (finite: these grids contain 0)
    got = ff.infidelities(pulses, S, omega)
    for p in range(8):
        assert rel_err(got[p], ff.infidelity(singles[p], S, omega)) < TIGHT, p
        assert rel_err(pulses[p].get_filter_function(omega), singles[p].get_filter_function(omega)) < TIGHT, p

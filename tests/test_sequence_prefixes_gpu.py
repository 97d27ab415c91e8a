"""ff.sequence_prefix_infidelities and ff.sequence_prefix_decay_amplitudes: infidelities, decay amplitudes and their
diagonals after 1, 2, ..., G gates of many gate sequences, with and without a closing gate behind every truncation,
against a forward walk of the concatenation rule and the trapezoid integral run on the host in extended precision from
the same inputs (tied once to the Yardstick of test_sequence_infidelities_gpu.py on the truncations themselves),
against the truncations handed to ff.sequence_infidelities / ff.sequence_decay_amplitudes as separate sequences,
against the loop over ff.concatenate at a few truncations, and against itself in other passes (bit for bit)."""
import numpy as np
import pytest

import filter_functions_amd as ff
import workloads as wl
from conftest import rel_err
from filter_functions_amd import numeric
from filter_functions_amd import sequence_prefixes as sx
from filter_functions_amd.sequences import resident_source
from test_sequence_infidelities_gpu import CLD, LD, LONG, NAMES, TIGHT, Yardstick, draws, two_qubit_gates
from test_sequence_processes_gpu import gamma_yardstick, real_spectra, single_qubit_gates

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 63, 64, 65, 130]
PARENT = 1e-12        # against the truncations as separate sequences of the sibling entries, and against the loop


def closers(seqs, seed, n_gates):
    """One closing gate behind every position of every sequence, negative indices among them."""
    rng = np.random.default_rng(seed)
    return [rng.integers(-n_gates, n_gates, len(s)) for s in seqs]


def truncations(seqs, close):
    """Every truncation of every sequence, its closing gate appended, as sequences of their own (in order)."""
    return [np.concatenate([s[:m], [] if close is None else [close[p][m - 1]]]).astype(int)
            for p, s in enumerate(seqs) for m in range(1, len(s) + 1)]


def curves(flat, seqs):
    """The values of :func:`truncations` back as one array per sequence."""
    ends = np.cumsum([len(s) for s in seqs])
    return [np.asarray(flat[end - len(s):end]) for s, end in zip(seqs, ends)]


# ---- the yardstick: a forward walk in np.longdouble -------------------------------------------------------------------
def walk(yard, s, close=None):
    """The control matrices (A, N, W) of the truncations of the sequence of gate numbers *s*, one after the other:
    Cum_m = Cum_{m-1} + phi_{m-1} (v_k Lam_m), Lam_{m+1} = L_k Lam_m; with a closing gate c, Cum_m + phi_m (v_c
    Lam_{m+1})."""
    T = len(yard.v)
    N = yard.v[0].shape[-1]
    Lam = np.eye(N, dtype=LD)
    Cum = np.zeros_like(yard.v[0])
    phi = np.ones_like(yard.p[0])
    for m, k in enumerate(s):
        k = int(k) % T
        Cum = Cum + phi*(yard.v[k] @ Lam)
        Lam = yard.L[k] @ Lam
        phi = phi*yard.p[k]
        R = Cum if close is None else Cum + phi*(yard.v[int(close[m]) % T] @ Lam)
        yield R.transpose(0, 2, 1)


def gamma_weights(yard, S, idx):
    """c_w S(w) / 2 pi of the trapezoid rule in long double, (n_idx, W)."""
    S = np.broadcast_to(np.asarray(S, dtype=np.float64), (len(idx), len(yard.omega))).astype(LD)
    x = yard.omega.astype(LD)
    c = np.zeros(len(x), dtype=LD)
    c[1:] += np.diff(x)/2
    c[:-1] += np.diff(x)/2
    return S*c/(8*np.arctan(LD(1)))


def gamma_curve(yard, s, close, weights, idx):
    """Gamma (G, n_idx, N, N) of every truncation under each set of *weights*, a list of (n_idx, W) arrays: a list of
    curves."""
    out = [[] for _ in weights]
    idx = np.asarray(idx)
    for R in walk(yard, s, close):
        re, im = R[idx].real, R[idx].imag
        for curve, w in zip(out, weights):
            curve.append((re*w[:, None, :]) @ re.transpose(0, 2, 1) + (im*w[:, None, :]) @ im.transpose(0, 2, 1))
    return [np.array(curve) for curve in out]


def test_the_walk_is_the_rule_of_the_truncations():
    omega = wl.rb_omega(33, 1.0, m_max=3)
    for gates in (two_qubit_gates(5, 2, omega, seed=1), single_qubit_gates(5, 3, omega, seed=1)):
        yard = Yardstick(gates, omega)
        s = draws([70], 3, 5)[0]
        close = closers([s], 4, 5)[0]
        S = real_spectra(2, omega, 5)[1]
        idx = [1, 0]
        plain = dict(enumerate(walk(yard, s), 1))
        closed = dict(enumerate(walk(yard, s, close), 1))
        curve = gamma_curve(yard, s, close, [gamma_weights(yard, S, idx)], idx)[0]
        for m in (1, 2, 33, 64, 70):
            assert rel_err(plain[m], yard.sequence([int(k) for k in s[:m]])[0]) < 1e-16
            R = yard.sequence([int(k) for k in s[:m]] + [int(close[m - 1]) % 5])[0]
            assert rel_err(closed[m], R) < 1e-16
            assert rel_err(curve[m - 1], gamma_yardstick(yard, R, S, idx)) < 1e-16


WORST = {'new': 0.0, 'parent': 0.0, 'diagonal': 0.0}


def check_against_yardstick_parent_and_loop(gates, seqs, omega, names, seed, with_loop=True):
    """Every sequence, spectra of one and two dimensions, with and without closing gates, all three modes: the new
    calls against the yardstick under the project's bars and within twice the parent route's own error, against the
    parent route, and against the loop at a few truncations."""
    yard = Yardstick(gates, omega)
    d, N, T = yard.d, len(gates[0].basis), len(gates)
    idx = ff.util.get_indices_from_identifiers(gates[0].n_oper_identifiers, names)
    bars = [LONG if len(s) >= 500 else TIGHT for s in seqs]
    spectra = real_spectra(len(idx), omega, seed)
    table = np.asarray(gates, dtype=object)
    kw = dict(n_oper_identifiers=names)
    for close in (None, closers(seqs, seed + 1, T)):
        weights = [gamma_weights(yard, S, idx) for S in spectra]
        refs = [gamma_curve(yard, s, None if close is None else close[p], weights, idx) for p, s in enumerate(seqs)]
        flat = truncations(seqs, close)
        for n, S in enumerate(spectra):
            infid = ff.sequence_prefix_infidelities(gates, seqs, S, omega, closing=close, **kw)
            diag = ff.sequence_prefix_decay_amplitudes(gates, seqs, S, omega, closing=close, diagonal=True, **kw)
            gamma = ff.sequence_prefix_decay_amplitudes(gates, seqs, S, omega, closing=close, **kw)
            parent_infid = curves(ff.sequence_infidelities(gates, flat, S, omega, **kw), seqs)
            parent_gamma = curves(ff.sequence_decay_amplitudes(gates, flat, S, omega, **kw), seqs)
            for p, s in enumerate(seqs):
                G = len(s)
                ref = refs[p][n]
                assert infid[p].shape == (G, len(idx)) and diag[p].shape == (G, len(idx), N)
                assert gamma[p].shape == (G, len(idx), N, N) and gamma[p].dtype == np.float64
                assert np.array_equal(gamma[p], gamma[p].swapaxes(-1, -2))
                ref_diag = np.diagonal(ref, axis1=-2, axis2=-1)
                pairs = (('Gamma', gamma[p], parent_gamma[p], ref),
                         ('diagonal', diag[p], np.diagonal(parent_gamma[p], axis1=-2, axis2=-1), ref_diag),
                         ('infidelity', infid[p], parent_infid[p], ref_diag.sum(axis=-1)/d))
                for what, new, old, want in pairs:
                    e_new, e_old = rel_err(new, want), rel_err(old, want)
                    print(f'd={d} W={len(omega)} A={len(gates[0].n_opers)} T={T} G={G} S.ndim={np.ndim(S)} '
                          f'closing={close is not None}: {what} new {e_new:.2e} parent {e_old:.2e} '
                          f'new against parent {rel_err(new, old):.2e}')
                    WORST.update(new=max(WORST['new'], e_new), parent=max(WORST['parent'], e_old))
                    assert e_new < bars[p], (what, p, e_new)
                    assert e_new <= max(2e-13, 2*e_old), (what, p, e_new, e_old)
                    assert rel_err(new, old) < PARENT, (what, p)
                # the diagonal's own arithmetic against the diagonal of Gamma
                e = rel_err(diag[p], np.diagonal(gamma[p], axis1=-2, axis2=-1))
                WORST['diagonal'] = max(WORST['diagonal'], e)
                assert e < bars[p], (p, e)
                if not with_loop:
                    continue
                for m in sorted({1, 2, 64, 65, G} & set(range(1, G + 1))):
                    pulse = ff.concatenate(list(table[s[:m]]) + ([gates[close[p][m - 1]]] if close is not None else []),
                                           omega=omega)
                    looped = numeric.calculate_decay_amplitudes(pulse, S, omega, names)
                    scale = np.abs(looped).max()
                    assert np.abs(gamma[p][m - 1] - looped).max() < PARENT*scale, (p, m)
                    assert np.abs(diag[p][m - 1] - np.diagonal(looped, axis1=-2, axis2=-1)).max() < PARENT*scale
                    assert rel_err(infid[p][m - 1], ff.infidelity(pulse, S, omega, names)) < PARENT, (p, m)
    print(f'worst so far: new {WORST["new"]:.2e}, parent {WORST["parent"]:.2e}, diagonal against Gamma '
          f'{WORST["diagonal"]:.2e}')


# ---- accuracy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W, A, T, pauli', [(7, 1, 3, True), (64, 2, 3, False), (65, 3, 3, True), (70, 4, 3, False),
                                            (33, 2, 40, True), (7, 4, 40, False)])
def test_two_qubit_gates_against_extended_precision(W, A, T, pauli):
    """T = 3: the tables staged in LDS; T = 40: read from L2.  W: a partial tile of 16 frequencies, a partial block, a
    full block, one frequency past it, a partial second block of either width."""
    omega = wl.rb_omega(W, 1.0, m_max=3)
    gates = two_qubit_gates(T, A, omega, seed=10*W + A, basis=ff.Basis.pauli(2) if pauli else ff.Basis.ggm(4))
    assert len(gates[0].basis) == 16 and gates[0].d == 4
    seqs = draws(LENGTHS, W + T, T)
    seqs[2] = np.array([-1, 0, -T])                       # negative indices wrap
    names = None if A == 1 else [NAMES[A - 1], NAMES[0]]    # a subset, not in sorted order
    check_against_yardstick_parent_and_loop(gates, seqs, omega, names, seed=W)


@pytest.mark.parametrize('W, A, T', [(70, 1, 24), (7, 2, 8), (64, 3, 8), (65, 4, 8), (65, 4, 24)])
def test_single_qubit_gates_against_extended_precision(W, A, T):
    """A = 1: the Clifford gate set; the tables staged in LDS and, the last, in L2."""
    if A == 1:
        omega = wl.rb_omega(W, wl.CONFIG3['T'])
        gates = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])[1]
    else:
        omega = wl.rb_omega(W, 1.0, m_max=3)
        gates = single_qubit_gates(T, A, omega, seed=W + A)
    names = None if A == 1 else ['B', 'A']
    seqs = draws(LENGTHS, W, T)
    seqs[2] = np.array([-1, 0, -T])
    check_against_yardstick_parent_and_loop(gates, seqs, omega, names, seed=A)


@pytest.mark.parametrize('d', [2, 4])
def test_five_hundred_positions(d):
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(40, 1, omega, seed=5) if d == 4 else single_qubit_gates(8, 2, omega, seed=5)
    check_against_yardstick_parent_and_loop(gates, draws([500], 1, len(gates)), omega, None, seed=2, with_loop=False)


# ---- bits ----------------------------------------------------------------------------------------------------------
def all_modes(gates, seqs, S, omega, **kwargs):
    """The three kinds of curves of a call, one list after the other."""
    return (ff.sequence_prefix_infidelities(gates, seqs, S, omega, **kwargs)
            + ff.sequence_prefix_decay_amplitudes(gates, seqs, S, omega, diagonal=True, **kwargs)
            + ff.sequence_prefix_decay_amplitudes(gates, seqs, S, omega, **kwargs))


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('d, A, T', [(4, 1, 3), (4, 2, 40), (4, 4, 3), (2, 1, 24), (2, 4, 24)])
def test_a_curve_does_not_depend_on_its_pass_or_the_split(d, A, T, monkeypatch):
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(T, A, omega, seed=A) if d == 4 else single_qubit_gates(T, A, omega, seed=A)
    S = real_spectra(A, omega, 4)[1]
    probe = draws([77], 8, T)[0]
    others = draws(np.random.default_rng(1).integers(1, 140, 39), 9, T)
    for close in (None, closers([probe] + others, 5, T)):
        one = lambda seqs, c: all_modes(gates, seqs, S, omega, closing=c)                       # noqa: E731
        alone = one([probe], None if close is None else close[:1])
        first = one([probe] + others, close)
        last = one(others + [probe], None if close is None else close[1:] + close[:1])
        assert same(alone, first[0::40]) and same(alone, last[39::40])
        # several passes, each kind of curve: a budget of the tables and the bytes of 400 positions, which the
        # sequences' own bytes come out of (the 40 sequences hold 77 + 39 draws from 1 ... 139 positions; none holds
        # more than 139)
        seqs, c = others + [probe], None if close is None else close[1:] + close[:1]
        n_positions = sum(len(s) for s in seqs)
        for n, (mode, diagonal) in enumerate((('infidelities', None), ('diagonal', True), ('decay_amplitudes', False))):
            with monkeypatch.context() as patch:
                per_position = sx.pass_bytes(d, A, 70, A, 1, mode, close is not None)
                patch.setattr(sx, 'PASS_BYTES', sx.table_bytes(T, d, A, 70, A, 1, 2) + 400*per_position)
                calls = []
                run_pass = sx._run_pass
                patch.setattr(sx, '_run_pass',
                              lambda *args: calls.append(sum(len(i) for i in args[1])) or run_pass(*args))
                if diagonal is None:
                    split = ff.sequence_prefix_infidelities(gates, seqs, S, omega, closing=c)
                else:
                    split = ff.sequence_prefix_decay_amplitudes(gates, seqs, S, omega, closing=c, diagonal=diagonal)
            assert len(calls) >= n_positions/400 and max(calls) <= 400 and sum(calls) == n_positions, (mode, calls)
            assert same(split, last[40*n:40*n + 40]), mode


@pytest.mark.parametrize('d', [2, 4])
def test_truncation_is_exact(d):
    """Position m sees nothing behind it: the curve of s[:m] is the first m rows of the curve of s."""
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(3, 3, omega, seed=3) if d == 4 else single_qubit_gates(5, 3, omega, seed=3)
    names = [gates[0].n_oper_identifiers[2], gates[0].n_oper_identifiers[0]]
    S = real_spectra(2, omega, 6)[1]
    seqs = draws([130, 70], 7, len(gates))
    for close in (None, closers(seqs, 8, len(gates))):
        whole = all_modes(gates, seqs, S, omega, closing=close, n_oper_identifiers=names)
        for m in (1, 63, 64, 65):
            part = all_modes(gates, [s[:m] for s in seqs], S, omega, n_oper_identifiers=names,
                             closing=None if close is None else [c[:m] for c in close])
            assert same([curve[:m] for curve in whole], part), m


@pytest.mark.parametrize('d', [2, 4])
def test_stacked_spectra_give_the_bits_of_single_calls(d):
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(3, 3, omega, seed=3) if d == 4 else single_qubit_gates(5, 3, omega, seed=3)
    names = [gates[0].n_oper_identifiers[2], gates[0].n_oper_identifiers[0]]
    seqs = draws([1, 5, 64, 100], 7, len(gates))
    close = closers(seqs, 2, len(gates))
    rng = np.random.default_rng(0)
    for S in (np.stack([wl.rb_spectrum(omega, alpha) for alpha in (0.0, 0.7, 1.5)]), rng.random((3, 2, 70))):
        stacked = all_modes(gates, seqs, S, omega, n_oper_identifiers=names, closing=close, stacked=True)
        assert all(curve.shape[0] == 3 for curve in stacked)
        for k in range(3):
            single = all_modes(gates, seqs, S[k], omega, n_oper_identifiers=names, closing=close)
            assert same([curve[k] for curve in stacked], single), k


def test_resident_gates_and_host_arrays_give_the_same_bits():
    omega = wl.rb_omega(70, 1.0, m_max=3)
    S = real_spectra(2, omega, 1)[1]
    seqs = draws([1, 2, 17, 64, 100], 6, 4)
    close = closers(seqs, 3, 4)
    single = two_qubit_gates(4, 2, omega, seed=3)                     # cache_control_matrix: single resident results
    assert all(resident_source(g, 4, 70, 16, 2)[1] == -1 for g in single)
    got = all_modes(single, seqs, S, omega, closing=close)
    host = [ff.PulseSequence(list(zip(g.c_opers, g.c_coeffs, g.c_oper_identifiers)),
                             list(zip(g.n_opers, g.n_coeffs, g.n_oper_identifiers)), g.dt) for g in single]
    for h, g in zip(host, single):
        h.cache_control_matrix(omega, np.array(g.get_control_matrix(omega)))
        h.total_propagator = np.array(g.total_propagator)
        assert resident_source(h, 4, 70, 16, 2) is None
    # every row uploaded, and a mixed table
    for table in (host, [single[0], host[1], single[2], host[3]]):
        assert same(got, all_modes(table, seqs, S, omega, closing=close))


def test_tables_in_lds_and_in_l2_give_the_same_bits():
    """A pass whose sequences use few gates stages their tables in LDS; among sequences that use 70 (single-qubit)
    or 40 (two-qubit) gates the tables are read from L2."""
    omega = wl.rb_omega(70, wl.CONFIG3['T'])
    X, Y = ff.util.paulis[1], ff.util.paulis[2]
    rng = np.random.default_rng(2)
    gates = list(wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])[1])
    for _ in range(46):
        extra = ff.PulseSequence([[X/2, [rng.normal()], 'X'], [Y/2, [rng.normal()], 'Y']], [[X/2, [1], 'X']],
                                 [1.0 + rng.random()])
        extra.cache_control_matrix(omega)
        gates.append(extra)
    S = wl.rb_spectrum(omega, 0.7)
    for table, few, many in ((gates, 24, 70), (two_qubit_gates(40, 2, omega, seed=9), 3, 40)):
        d, A = table[0].d, len(table[0].n_opers)
        probes = draws([1, 30, 130], 3, few)
        # closing gates among the first `few` gates as well (a negative index would wrap against the whole table)
        for close in (None, [np.random.default_rng(4 + p).integers(0, few, len(s)) for p, s in enumerate(probes)]):
            used = np.unique(np.concatenate(probes + (close or [])))
            # 122880 of 153600 bytes at d = 2 (24 gates), 103424 at d = 4 (3 gates); 70 and 40 gates do not fit
            assert used.max() < few and sx.staged(d, len(used), A) and not sx.staged(d, many, A)
            tables = []
            run_pass = sx._run_pass

            def recording(gates, indices, close, *args):
                tables.append(len(np.unique(np.concatenate(list(indices) + list(close or [])))))
                return run_pass(gates, indices, close, *args)
            sx._run_pass = recording
            try:
                staged = all_modes(table, probes, S, omega, closing=close)
                among = all_modes(table, probes + [np.arange(many)], S, omega,
                                  closing=None if close is None else close + [np.zeros(many, dtype=int)])
            finally:
                sx._run_pass = run_pass
            # what the passes really held: the small tables three times, then the large ones
            assert tables == [len(used)]*3 + [many]*3, tables
            assert same(staged, [curve for n, curve in enumerate(among) if n % 4 != 3])


# ---- propagators, the route, the loop route, exceptions, caches -------------------------------------------------------
def test_return_propagators_against_the_host_helper_and_the_loop():
    omega = wl.rb_omega(20, 1.0, m_max=3)
    S = wl.rb_spectrum(omega, 0.7)
    for gates in (two_qubit_gates(4, 1, omega, seed=8), single_qubit_gates(4, 2, omega, seed=8)):
        seqs = draws([1, 3, 130], 2, 4)
        table = np.asarray(gates, dtype=object)
        for close in (None, closers(seqs, 1, 4)):
            helper = ff.sequence_prefix_propagators(gates, seqs, closing=close)
            for function in (ff.sequence_prefix_infidelities, ff.sequence_prefix_decay_amplitudes):
                values, U = function(gates, seqs, S, omega, closing=close, return_propagators=True)
                assert same(values, function(gates, seqs, S, omega, closing=close)) and same(U, helper)
            for p, s in enumerate(seqs):
                for m in {1, 3, len(s)} & set(range(1, len(s) + 1)):
                    pulse = ff.concatenate(list(table[s[:m]]) + ([gates[close[p][m - 1]]] if close is not None else []),
                                           omega=omega)
                    assert rel_err(helper[p][m - 1], pulse.total_propagator) < 1e-13, (p, m)


def loops_expression(gates, seqs, close, S, omega, names=None):
    """What the functions document: the loop over the truncations, (infidelities, diagonals, decay amplitudes,
    propagators)."""
    table = np.asarray(gates, dtype=object)
    out = [[], [], [], []]
    for p, s in enumerate(seqs):
        pulses = [ff.concatenate(list(table[s[:m]]) + ([gates[close[p][m - 1]]] if close is not None else []),
                                 omega=omega) for m in range(1, len(s) + 1)]
        gamma = [numeric.calculate_decay_amplitudes(pulse, S, omega, names) for pulse in pulses]
        out[0].append(np.stack([ff.infidelity(pulse, S, omega, names) for pulse in pulses]))
        out[1].append(np.stack([np.diagonal(g, axis1=-2, axis2=-1) for g in gamma]))
        out[2].append(np.stack(gamma))
        out[3].append(np.stack([np.array(pulse.total_propagator) for pulse in pulses]))
    return out


def test_route_really_taken_and_the_loop_route(monkeypatch):
    omega = wl.rb_omega(20, 1.0, m_max=3)
    S = wl.rb_spectrum(omega, 0.7)
    rng = np.random.default_rng(3)
    cliffords = wl.rb_cliffords(ff, omega, 1.0)[1]
    d4 = two_qubit_gates(3, 2, omega, seed=1)
    C = rng.random((2, 2, 20)) + 1j*rng.random((2, 2, 20))
    cross = C + C.conj().swapaxes(0, 1)
    spin1 = [ff.PulseSequence([[np.diag([1.0, 0.0, -1.0]), [0.3 + 0.1*k], 'Z']],
                              [[np.diag([1.0, -1.0, 0.0]), [1.0], 'N']], [1.0]) for k in range(2)]
    for g in spin1:
        g.cache_control_matrix(omega)
    eligible = [(cliffords, draws([1, 2, 30], 1, 24), S), (d4, draws([1, 2, 30], 2, 3), S)]
    others = [(d4, [np.array([0, 1, 2]), np.array([2, 2])], cross), (spin1, [np.array([0, 1]), np.array([1, 1, 0])], S)]

    def refuse(*args, **kwargs):
        raise AssertionError('the loop ran')
    for g, s, spectrum in eligible:
        close = closers(s, 6, len(g))
        expected = loops_expression(g, s, close, spectrum, omega)
        with monkeypatch.context() as patch:
            patch.setattr(ff, 'concatenate', refuse)
            got = all_modes(g, s, spectrum, omega, closing=close)
        for value, ref in zip(got, expected[0] + expected[1] + expected[2]):
            assert value.shape == ref.shape and rel_err(value, ref) < PARENT
    # cross-spectra and d = 3: the loop's expression, to the bit
    for g, s, spectrum in others:
        for close in (None, closers(s, 7, len(g))):
            with monkeypatch.context() as patch:
                patch.setattr(ff, 'concatenate', refuse)
                with pytest.raises(AssertionError, match='the loop ran'):
                    ff.sequence_prefix_infidelities(g, s, spectrum, omega, closing=close)
            expected = loops_expression(g, s, close, spectrum, omega)
            infid, U = ff.sequence_prefix_infidelities(g, s, spectrum, omega, closing=close, return_propagators=True)
            assert same(infid, expected[0]) and same(U, expected[3])
            assert same(ff.sequence_prefix_decay_amplitudes(g, s, spectrum, omega, closing=close, diagonal=True),
                        expected[1])
            assert same(ff.sequence_prefix_decay_amplitudes(g, s, spectrum, omega, closing=close), expected[2])
    stacked = ff.sequence_prefix_decay_amplitudes(d4, others[0][1], np.stack([cross, 2*cross]), omega, stacked=True)
    assert [a.shape for a in stacked] == [(2, 3, 2, 2, 16, 16), (2, 2, 2, 2, 16, 16)]
    assert same([a[1] for a in stacked], ff.sequence_prefix_decay_amplitudes(d4, others[0][1], 2*cross, omega))


def test_indices_exceptions_and_caches():
    omega = wl.rb_omega(20, 1.0, m_max=3)
    S = wl.rb_spectrum(omega, 0.7)
    gates = two_qubit_gates(4, 1, omega, seed=7)
    caches = lambda: [(sorted(g._data), sorted(g._frequency_data),                       # noqa: E731
                       {k: id(g._frequency_data.peek(k)) for k in g._frequency_data}) for g in gates]
    before = caches()
    got = ff.sequence_prefix_decay_amplitudes(gates, [[-1, 0, -4], [3, 0, 0]], S, omega, closing=[[-2, 1, 0], [2, -3, 0]])
    assert caches() == before
    assert np.array_equal(got[0], got[1])                                                # negative indices wrap
    for function in (ff.sequence_prefix_infidelities, ff.sequence_prefix_decay_amplitudes):
        with pytest.raises(IndexError):
            function(gates, [[0, 4]], S, omega)
        with pytest.raises(IndexError):
            function(gates, [[0, 1]], S, omega, closing=[[0, 4]])
        with pytest.raises(ValueError):
            function(gates, [[0], []], S, omega)
        with pytest.raises(ValueError):
            function(gates, [[0, 1]], S, omega, closing=[[0]])
        with pytest.raises(TypeError):
            function(gates, [[0.0, 1.0]], S, omega)
        with pytest.raises(TypeError):
            function(gates, [[0, 1]], S, omega, closing=[[0.0, 1.0]])
    assert caches() == before
    # the loop's messages for a spectrum that does not fit the grid and for unknown identifiers
    pulse = ff.concatenate([gates[0], gates[1]], omega=omega)
    for kwargs in (dict(spectrum=np.ones(7)), dict(spectrum=S, n_oper_identifiers=['Q'])):
        with pytest.raises(ValueError) as loop_error:
            numeric.calculate_decay_amplitudes(pulse, kwargs['spectrum'], omega, kwargs.get('n_oper_identifiers'))
        with pytest.raises(ValueError) as error:
            ff.sequence_prefix_decay_amplitudes(gates, [[0, 1]], omega=omega, **kwargs)
        assert str(error.value) == str(loop_error.value)
    # gates without a control matrix on the grid are completed by one batched call, then read in place
    fresh = [ff.PulseSequence(list(zip(g.c_opers, g.c_coeffs, g.c_oper_identifiers)),
                              list(zip(g.n_opers, g.n_coeffs, g.n_oper_identifiers)), g.dt) for g in gates]
    a = ff.sequence_prefix_infidelities(fresh, [[3, 0, 0], [1, 2]], S, omega)
    b = ff.sequence_prefix_infidelities(gates, [[3, 0, 0], [1, 2]], S, omega)
    assert all(rel_err(x, y) < 1e-13 for x, y in zip(a, b))
    assert all(resident_source(g, 4, 20, 16, 1) is not None for g in fresh)

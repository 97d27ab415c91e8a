"""ff.sequence_prefix_frequency_shifts and ff.sequence_prefix_cumulant_functions: the frequency shifts after 1, 2, ..., G
gates of many gate sequences, with and without a closing gate behind every truncation, against the forward form of the
second-order concatenation rule kept after every position on the host in extended precision (the ShiftYardstick of
test_sequence_second_order_gpu.py, extended and tied to it on the truncations themselves), against the loop over
ff.concatenate(..., calc_second_order_FF=True) at a few truncations, against the truncations handed to
ff.sequence_frequency_shifts as sequences of their own, and against itself in other passes (bit for bit)."""
import numpy as np
import pytest

import filter_functions_amd as ff
import workloads as wl
from conftest import rel_err
from filter_functions_amd import _lib, numeric
from filter_functions_amd import sequence_prefix_second_order as sp2
from filter_functions_amd.sequences import resident_source
from test_sequence_infidelities_gpu import CLD, LD, LONG, NAMES, TIGHT, draws, two_qubit_gates
from test_sequence_prefixes_gpu import closers, same
from test_sequence_processes_gpu import BAR, real_spectra, single_qubit_gates
from test_sequence_second_order_gpu import ShiftYardstick

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 63, 64, 65, 130]
LOOPED = (1, 2, 3, 65)             # the lengths at which the loop is evaluated as well (at T = 3)


class PrefixShiftYardstick(ShiftYardstick):
    """ShiftYardstick.shifts with `delta` kept after every position; with a closing gate c behind the position it adds
    Lam_{m+1}^T own[c] Lam_{m+1} and the Gram of phase (v[c] @ Lam_{m+1}) with `cum`.  All in long double, from the
    device's inputs."""

    def curve(self, s, close, S, idx, gate_shifts):
        idx = np.asarray(idx)
        W, N = len(self.omega), self.v[0].shape[-1]
        x = self.omega.astype(LD)
        pi = 4*np.arctan(LD(1))
        weight = np.zeros(W, dtype=LD)
        weight[:-1] += np.diff(x)/2
        weight[1:] += np.diff(x)/2
        weight = weight*np.broadcast_to(np.asarray(S, dtype=np.float64), (len(idx), W)).astype(LD)/(2*pi)
        own = np.asarray(gate_shifts).astype(LD)
        Lam = np.eye(N, dtype=LD)
        phase = np.ones((1, W, 1), dtype=CLD)
        cum = np.zeros((len(idx), W, N), dtype=CLD)
        delta = np.zeros((len(idx), N, N), dtype=LD)
        rows = []
        for m, k in enumerate(s):
            Rs = phase*(self.v[k][idx] @ Lam)
            delta += Lam.T @ own[k] @ Lam
            delta += np.einsum('iwk,iwl,iw->ikl', Rs.conj(), cum, weight).real
            cum += Rs
            phase = phase*self.p[k]
            Lam = self.L[k].real @ Lam
            row = delta.copy()
            if close is not None:
                c = close[m]
                Rc = phase*(self.v[c][idx] @ Lam)
                row += Lam.T @ own[c] @ Lam
                row += np.einsum('iwk,iwl,iw->ikl', Rc.conj(), cum, weight).real
            rows.append(row)
        return np.array(rows)


def wrapped(s, T):
    return [int(k) % T for k in s]


def test_the_curve_is_the_shift_yardstick_of_the_truncations():
    omega = wl.rb_omega(33, 1.0, m_max=3)
    for gates in (two_qubit_gates(5, 2, omega, seed=1), single_qubit_gates(5, 3, omega, seed=1)):
        yard = PrefixShiftYardstick(gates, omega)
        s = wrapped(draws([70], 3, 5)[0], 5)
        close = wrapped(closers([s], 4, 5)[0], 5)
        idx = [1, 0]
        for S in real_spectra(2, omega, 5):
            own = ff.frequency_shifts(gates, S, omega, [gates[0].n_oper_identifiers[i] for i in idx])
            plain = yard.curve(s, None, S, idx, own)
            closed = yard.curve(s, close, S, idx, own)
            for m in (1, 2, 33, 64, 70):
                assert np.abs(plain[m - 1] - yard.shifts(s[:m], S, idx, own)).max() < 1e-16*np.abs(plain).max(), m
                ref = yard.shifts(s[:m] + [close[m - 1]], S, idx, own)
                assert np.abs(closed[m - 1] - ref).max() < 1e-16*np.abs(closed).max(), m


WORST = {'new': 0.0, 'loop': 0.0, 'parent': 0.0, 'new against parent': 0.0}


def curve_errors(got, ref):
    """Per selected operator: the error of the curve tensor (G, N, N), max-normalised over the whole curve."""
    return [rel_err(got[:, a], ref[:, a]) for a in range(ref.shape[1])]


def check(gates, seqs, omega, names, seed, looped=(), parent=True):
    """Every sequence, spectra of one and two dimensions, with and without closing gates: the new call against the
    yardstick under the project's bars per (sequence, operator) curve; where the loop is evaluated, within twice the
    loop's own error and within 1e-12 of the loop; the truncations as sequences of ff.sequence_frequency_shifts within
    TIGHT."""
    yard = PrefixShiftYardstick(gates, omega)
    T, N, d = len(gates), len(gates[0].basis), gates[0].d
    idx = ff.util.get_indices_from_identifiers(gates[0].n_oper_identifiers, names)
    bars = [LONG if len(s) >= 500 else TIGHT for s in seqs]
    table = np.asarray(gates, dtype=object)
    kw = dict(n_oper_identifiers=names)
    pulses = {}
    for S in real_spectra(len(idx), omega, seed):
        for close in (None, closers(seqs, seed + 1, T)):
            got = ff.sequence_prefix_frequency_shifts(gates, seqs, S, omega, closing=close, **kw)
            # (before the loop caches the gates' second-order filter functions: the route the call above took)
            own = ff.frequency_shifts(gates, S, omega, names)
            for p, s in enumerate(seqs):
                G = len(s)
                c = None if close is None else wrapped(close[p], T)
                ref = yard.curve(wrapped(s, T), c, S, idx, own)
                assert got[p].shape == (G, len(idx), N, N) and got[p].dtype == np.float64
                errors = curve_errors(got[p], ref)
                print(f'd={d} W={len(omega)} A={len(gates[0].n_opers)} T={T} G={G} S.ndim={np.ndim(S)} '
                      f'closing={close is not None}: Delta new {max(errors):.2e}')
                WORST['new'] = max(WORST['new'], *errors)
                assert max(errors) < bars[p], (p, errors)
                if G in looped:
                    for m in sorted({1, 2, G} & set(range(1, G + 1))):
                        key = (p, m, close is not None)
                        if key not in pulses:
                            members = list(table[s[:m]]) + ([gates[close[p][m - 1]]] if close is not None else [])
                            pulses[key] = ff.concatenate(members, calc_second_order_FF=True, omega=omega)
                        loop = numeric.calculate_frequency_shifts(pulses[key], S, omega, names)
                        for a in range(len(idx)):
                            scale = np.abs(ref[:, a]).max()
                            new = np.abs(got[p][m - 1, a] - ref[m - 1, a]).max()/scale
                            old = float(np.abs(loop[a] - ref[m - 1, a]).max()/scale)
                            WORST['loop'] = max(WORST['loop'], old)
                            print(f'    G={G} m={m} operator {a}: new {new:.2e} loop {old:.2e}')
                            assert new <= max(2e-13, 2*old), (p, m, a, new, old)
                            assert np.abs(got[p][m - 1, a] - loop[a]).max() < 1e-12*scale, (p, m, a)
            if not parent:
                continue
            # the parent route: the truncations (with their closing gates) as sequences of their own
            where = [(p, m) for p, s in enumerate(seqs) for m in sorted({1, 2, 64, 65, len(s)} & set(range(1, len(s) + 1)))
                     if close is not None or m == len(s)]
            flat = [np.concatenate([seqs[p][:m], [] if close is None else [close[p][m - 1]]]).astype(int)
                    for p, m in where]
            old = ff.sequence_frequency_shifts(gates, flat, S, omega, **kw)
            equal = 0
            for (p, m), value in zip(where, old):
                for a in range(len(idx)):
                    scale = np.abs(got[p][:, a]).max()
                    e = float(np.abs(got[p][m - 1, a] - value[a]).max()/scale)
                    WORST['new against parent'] = max(WORST['new against parent'], e)
                    assert e < TIGHT, (p, m, a, e)
                equal += np.array_equal(got[p][m - 1], value)
            print(f'    parent route: {equal} of {len(where)} truncations bit-equal (closing={close is not None})')
    print(f'worst so far: {WORST}')


# ---- accuracy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W, A, T', [(7, 1, 3), (64, 2, 3), (65, 3, 3), (70, 4, 3), (33, 2, 40), (7, 4, 40)])
def test_two_qubit_gates_against_extended_precision(W, A, T):
    """T = 3: the tables staged in LDS; T = 40: read from L2.  W: a partial tile of 16 frequencies, a full block, one
    frequency past it, a partial second block.  Pauli and default basis in turn.  The loop is evaluated at T = 3."""
    omega = wl.rb_omega(W, 1.0, m_max=3)
    gates = two_qubit_gates(T, A, omega, seed=10*W + A, basis=ff.Basis.pauli(2) if A % 2 else None)
    assert len(gates[0].basis) == 16 and gates[0].d == 4
    seqs = draws(LENGTHS, W + T, T)
    seqs[2] = np.array([-1, 0, -T])                       # negative indices wrap
    names = None if A == 1 else [NAMES[A - 1], NAMES[0]]    # a subset, not in sorted order
    check(gates, seqs, omega, names, seed=W, looped=LOOPED if T == 3 else ())


def inverses(gates, seqs):
    """The gate that inverts every truncation of every sequence (up to a phase), picked from the propagators."""
    U = np.array([np.asarray(g.total_propagator) for g in gates])
    out = []
    for total in ff.sequence_prefix_propagators(gates, seqs):
        overlap = np.abs(np.einsum('cab,mba->mc', U, total))
        assert np.allclose(overlap.max(axis=1), 2.0, atol=1e-6)
        out.append(overlap.argmax(axis=1))
    return out


def test_cliffords_closed_by_their_inverses_at_the_studys_grid():
    """The case the study plots: 24 Cliffords, 301 frequencies, every truncation closed by its true inverse."""
    omega = wl.rb_omega(301, wl.CONFIG3['T'])
    gates = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])[1]
    seqs = draws([1, 2, 3, 64, 65, 152], 301, 24)
    close = inverses(gates, seqs)
    yard = PrefixShiftYardstick(gates, omega)
    S = np.stack([wl.rb_spectrum(omega, alpha) for alpha in (0.0, 0.7)])
    got, U = ff.sequence_prefix_frequency_shifts(gates, seqs, S, omega, closing=close, stacked=True,
                                                 return_propagators=True)
    own = [ff.frequency_shifts(gates, S[k], omega) for k in range(2)]
    for p, s in enumerate(seqs):
        # closed by its inverse every truncation is the identity up to a phase
        assert np.allclose(np.abs(np.trace(U[p], axis1=-2, axis2=-1)), 2.0, atol=1e-6)
        for k in range(2):
            ref = yard.curve(wrapped(s, 24), wrapped(close[p], 24), S[k], [0], own[k])
            e = max(curve_errors(got[p][k], ref))
            print(f'Cliffords W=301 G={len(s)} spectrum {k}: Delta new {e:.2e}')
            WORST['new'] = max(WORST['new'], e)
            assert e < TIGHT, (p, k, e)
    # the loop at a few truncations of the sequences of 1, 2, 3 and 65 gates
    table = np.asarray(gates, dtype=object)
    for p in (0, 1, 2, 4):
        s = seqs[p]
        scale = np.abs(got[p][1]).max()
        for m in sorted({1, 2, len(s)} & set(range(1, len(s) + 1))):
            pulse = ff.concatenate(list(table[s[:m]]) + [gates[close[p][m - 1]]], calc_second_order_FF=True, omega=omega)
            loop = numeric.calculate_frequency_shifts(pulse, S[1], omega)
            assert np.abs(got[p][1, m - 1] - loop).max() < 1e-12*scale, (p, m)


@pytest.mark.parametrize('W, A, T', [(7, 2, 3), (64, 3, 3), (65, 4, 3), (65, 4, 24)])
def test_single_qubit_gates_against_extended_precision(W, A, T):
    """Random gate sets staged in LDS and, the last, read from L2; up to 152 positions."""
    omega = wl.rb_omega(W, 1.0, m_max=3)
    gates = single_qubit_gates(T, A, omega, seed=W + A)
    seqs = draws([1, 2, 3, 64, 65, 152], W, T)
    seqs[2] = np.array([-1, 0, -T])
    check(gates, seqs, omega, ['B', 'A'], seed=A, looped=LOOPED if T == 3 else ())


@pytest.mark.parametrize('d', [2, 4])
def test_five_hundred_positions(d):
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(40, 1, omega, seed=5) if d == 4 else single_qubit_gates(8, 2, omega, seed=5)
    check(gates, draws([500], 1, len(gates)), omega, None, seed=2, parent=False)


# ---- bits ----------------------------------------------------------------------------------------------------------
def fixed_shifts(patch, gates, S, omega, names=None, stacked=False):
    """Holds the gates' own shifts fixed for the calls that follow: what ff.frequency_shifts gives now."""
    spectra = list(S) if stacked else [S]
    own = [ff.frequency_shifts(gates, one, omega, names) for one in spectra]
    calls = iter(range(10**9))
    patch.setattr(sp2, '_gate_shifts', lambda g, spectrum, w, n: own[next(calls) % len(own)] if stacked else own[0])
    return own


@pytest.mark.parametrize('d, A, T', [(4, 1, 3), (4, 2, 40), (4, 4, 3), (2, 1, 24), (2, 4, 24)])
def test_a_curve_does_not_depend_on_its_pass_or_the_split(d, A, T, monkeypatch):
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(T, A, omega, seed=A) if d == 4 else single_qubit_gates(T, A, omega, seed=A)
    S = real_spectra(A, omega, 4)[1]
    probe = draws([77], 8, T)[0]
    others = draws(np.random.default_rng(1).integers(1, 140, 39), 9, T)
    for close in (None, closers([probe] + others, 5, T)):
        one = lambda seqs, c: ff.sequence_prefix_frequency_shifts(gates, seqs, S, omega, closing=c)     # noqa: E731
        alone = one([probe], None if close is None else close[:1])
        first = one([probe] + others, close)
        seqs, c = others + [probe], None if close is None else close[1:] + close[:1]
        last = one(seqs, c)
        assert np.array_equal(alone[0], first[0]) and np.array_equal(alone[0], last[39])
        # seven or more passes: a budget of the tables and the bytes of 400 positions (no sequence holds more than 139)
        n_positions = sum(len(s) for s in seqs)
        with monkeypatch.context() as patch:
            per_position = sp2.pass_bytes(d, A, 70, A, 1, close is not None)
            patch.setattr(sp2, 'PASS_BYTES', sp2.table_bytes(T, d, A, 70, A, 1, 2) + 400*per_position)
            calls = []
            run_pass = sp2._run_pass
            patch.setattr(sp2, '_run_pass', lambda *args: calls.append(sum(len(i) for i in args[1])) or run_pass(*args))
            split = one(seqs, c)
        assert len(calls) >= 7 and max(calls) <= 400 and sum(calls) == n_positions, calls
        assert same(split, last)


@pytest.mark.parametrize('d', [2, 4])
def test_truncation_is_exact_and_row_zero_is_the_gates_own_shift(d):
    """Position m sees nothing behind it; without a closing gate the first position is the gate alone (Lam = 1,
    C_0 = 0)."""
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(3, 3, omega, seed=3) if d == 4 else single_qubit_gates(5, 3, omega, seed=3)
    names = [gates[0].n_oper_identifiers[2], gates[0].n_oper_identifiers[0]]
    seqs = draws([130, 70], 7, len(gates))
    for S in real_spectra(2, omega, 6):
        own = ff.frequency_shifts(gates, S, omega, names)
        for close in (None, closers(seqs, 8, len(gates))):
            whole = ff.sequence_prefix_frequency_shifts(gates, seqs, S, omega, closing=close, n_oper_identifiers=names)
            for m in (1, 63, 64, 65):
                part = ff.sequence_prefix_frequency_shifts(gates, [s[:m] for s in seqs], S, omega,
                                                           n_oper_identifiers=names,
                                                           closing=None if close is None else [c[:m] for c in close])
                assert same([curve[:m] for curve in whole], part), m
            for p, s in enumerate(seqs):
                equal = np.array_equal(whole[p][0] + 0.0, own[s[0]] + 0.0)
                assert equal == (close is None), (p, close is None)


@pytest.mark.parametrize('d', [2, 4])
def test_stacked_spectra_give_the_bits_of_single_calls(d):
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(3, 3, omega, seed=3) if d == 4 else single_qubit_gates(5, 3, omega, seed=3)
    names = [gates[0].n_oper_identifiers[2], gates[0].n_oper_identifiers[0]]
    seqs = draws([1, 5, 64, 100], 7, len(gates))
    rng = np.random.default_rng(0)
    for S in (np.stack([wl.rb_spectrum(omega, alpha) for alpha in (0.0, 0.7, 1.5)]), rng.random((3, 2, 70))):
        for close in (None, closers(seqs, 2, len(gates))):
            stacked = ff.sequence_prefix_frequency_shifts(gates, seqs, S, omega, n_oper_identifiers=names,
                                                          closing=close, stacked=True)
            assert all(curve.shape == (3, len(s), 2, d*d, d*d) for curve, s in zip(stacked, seqs))
            for k in range(3):
                single = ff.sequence_prefix_frequency_shifts(gates, seqs, S[k], omega, n_oper_identifiers=names,
                                                             closing=close)
                assert same([curve[k] for curve in stacked], single), k


def test_resident_gates_and_host_arrays_give_the_same_bits(monkeypatch):
    omega = wl.rb_omega(70, 1.0, m_max=3)
    S = real_spectra(2, omega, 1)[1]
    seqs = draws([1, 2, 17, 64, 100], 6, 4)
    single = two_qubit_gates(4, 2, omega, seed=3)                     # cache_control_matrix: single resident results
    assert all(resident_source(g, 4, 70, 16, 2)[1] == -1 for g in single)
    # (the gates' own shifts held fixed: the host copies below would take another route through ff.frequency_shifts)
    fixed_shifts(monkeypatch, single, S, omega)
    host = [ff.PulseSequence(list(zip(g.c_opers, g.c_coeffs, g.c_oper_identifiers)),
                             list(zip(g.n_opers, g.n_coeffs, g.n_oper_identifiers)), g.dt) for g in single]
    for h, g in zip(host, single):
        h.cache_control_matrix(omega, np.array(g.get_control_matrix(omega)))
        h.total_propagator = np.array(g.total_propagator)
        assert resident_source(h, 4, 70, 16, 2) is None
    for close in (None, closers(seqs, 3, 4)):
        got = ff.sequence_prefix_frequency_shifts(single, seqs, S, omega, closing=close)
        # every row uploaded, and a mixed table
        for table in (host, [single[0], host[1], single[2], host[3]]):
            assert same(got, ff.sequence_prefix_frequency_shifts(table, seqs, S, omega, closing=close))


def test_tables_in_lds_and_in_l2_give_the_same_bits(monkeypatch):
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
        with monkeypatch.context() as patch:
            fixed_shifts(patch, table, S, omega)
            # closing gates among the first `few` gates as well (a negative index would wrap against the whole table)
            for close in (None, [np.random.default_rng(4 + p).integers(0, few, len(s)) for p, s in enumerate(probes)]):
                used = np.unique(np.concatenate(probes + (close or [])))
                closing = close is not None
                assert used.max() < few and sp2.staged(d, len(used), A, closing) and not sp2.staged(d, many, A, closing)
                tables = []
                run_pass = sp2._run_pass

                def recording(gates, indices, close, *args):
                    tables.append(len(np.unique(np.concatenate(list(indices) + list(close or [])))))
                    return run_pass(gates, indices, close, *args)
                patch.setattr(sp2, '_run_pass', recording)
                staged = ff.sequence_prefix_frequency_shifts(table, probes, S, omega, closing=close)
                among = ff.sequence_prefix_frequency_shifts(
                    table, probes + [np.arange(many)], S, omega,
                    closing=None if close is None else close + [np.zeros(many, dtype=int)])
                patch.setattr(sp2, '_run_pass', run_pass)
                # the form each pass took: the small table, then the large one
                assert tables == [len(used), many], tables
                assert same(staged, among[:3])


# ---- the route, the loop route, propagators, cumulant functions, exceptions, caches ------------------------------------
def loops_expression(gates, seqs, close, S, omega, names=None):
    """What the function documents: the loop over the truncations, (frequency shifts, propagators)."""
    table = np.asarray(gates, dtype=object)
    shifts, total = [], []
    for p, s in enumerate(seqs):
        pulses = [ff.concatenate(list(table[s[:m]]) + ([gates[close[p][m - 1]]] if close is not None else []),
                                 calc_second_order_FF=True, omega=omega) for m in range(1, len(s) + 1)]
        shifts.append(np.stack([numeric.calculate_frequency_shifts(pulse, S, omega, names) for pulse in pulses]))
        total.append(np.stack([np.array(pulse.total_propagator) for pulse in pulses]))
    return shifts, total


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
    eligible = [(cliffords, draws([1, 2, 9], 1, 24), S), (d4, draws([1, 2, 9], 2, 3), S)]
    others = [(d4, [np.array([0, 1, 2]), np.array([2, 2])], cross), (spin1, [np.array([0, 1]), np.array([1, 1, 0])], S)]

    def refuse(*args, **kwargs):
        raise AssertionError('the loop ran')
    for g, s, spectrum in eligible:
        close = closers(s, 6, len(g))
        with monkeypatch.context() as patch:
            patch.setattr(ff, 'concatenate', refuse)
            patch.setattr(sp2, '_loop', refuse)
            patch.setattr(sp2, '_single', refuse)
            got, U = ff.sequence_prefix_frequency_shifts(g, s, spectrum, omega, closing=close, return_propagators=True)
        shifts, total = loops_expression(g, s, close, spectrum, omega)
        assert same(U, ff.sequence_prefix_propagators(g, s, closing=close))
        for value, ref, u, u_ref in zip(got, shifts, U, total):
            assert value.shape == ref.shape and rel_err(value, ref) < 1e-12 and rel_err(u, u_ref) < 1e-13
    # cross-spectra and d = 3: the loop's expression, to the bit
    for g, s, spectrum in others:
        for close in (None, closers(s, 7, len(g))):
            with monkeypatch.context() as patch:
                patch.setattr(ff, 'concatenate', refuse)
                with pytest.raises(AssertionError, match='the loop ran'):
                    ff.sequence_prefix_frequency_shifts(g, s, spectrum, omega, closing=close)
            shifts, total = loops_expression(g, s, close, spectrum, omega)
            got, U = ff.sequence_prefix_frequency_shifts(g, s, spectrum, omega, closing=close, return_propagators=True)
            assert same(got, shifts) and same(U, total)
    stacked = ff.sequence_prefix_frequency_shifts(d4, others[0][1], np.stack([cross, 2*cross]), omega, stacked=True)
    assert [a.shape for a in stacked] == [(2, 3, 2, 2, 16, 16), (2, 2, 2, 2, 16, 16)]
    assert same([a[1] for a in stacked], ff.sequence_prefix_frequency_shifts(d4, others[0][1], 2*cross, omega))


@pytest.mark.parametrize('d', [2, 4])
def test_cumulant_functions_against_the_loop_the_parent_route_and_the_composition(d):
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(4, 2, omega, seed=11, basis=ff.Basis.pauli(2)) if d == 4 \
        else single_qubit_gates(4, 2, omega, seed=11)
    seqs = draws([1, 2, 5], 5, 4)
    close = closers(seqs, 12, 4)
    S = np.outer([1e-3, 2e-3], 1/omega)
    table = np.asarray(gates, dtype=object)
    N = d*d
    for c in (None, close):
        # first order: the keyword absent, the keyword False, and the composition by hand, bit for bit
        first = ff.sequence_prefix_cumulant_functions(gates, seqs, S, omega, closing=c)
        assert same(first, ff.sequence_prefix_cumulant_functions(gates, seqs, S, omega, closing=c, second_order=False))
        gamma = ff.sequence_prefix_decay_amplitudes(gates, seqs, S, omega, closing=c)
        tiles = np.ascontiguousarray(np.concatenate([g.reshape(-1, N, N) for g in gamma]))
        by_hand = np.empty_like(tiles)
        basis = _lib.as_c128(np.asarray(gates[0].basis))
        single_qubit = int(d == 2 and getattr(gates[0].basis, 'btype', None) in ('Pauli', 'GGM'))
        _lib.check(_lib.load().ffk_cumulant_function(tiles.ctypes.data, len(tiles), N, d, basis.ctypes.data,
                                                     single_qubit, by_hand.ctypes.data))
        assert np.array_equal(np.concatenate([k.reshape(-1, N, N) for k in first]), by_hand)
        second, U = ff.sequence_prefix_cumulant_functions(gates, seqs, S, omega, closing=c, second_order=True,
                                                          return_propagators=True)
        assert same(U, ff.sequence_prefix_propagators(gates, seqs, closing=c))
        for p, s in enumerate(seqs):
            assert second[p].shape == first[p].shape == (len(s), 2, N, N)
            for m in sorted({1, 2, len(s)} & set(range(1, len(s) + 1))):
                pulse = ff.concatenate(list(table[s[:m]]) + ([gates[c[p][m - 1]]] if c is not None else []),
                                       calc_second_order_FF=True, omega=omega)
                ref = numeric.calculate_cumulant_function(pulse, S, omega, second_order=True)
                e = rel_err(second[p][m - 1], ref)
                print(f'd={d} G={len(s)} m={m} closing={c is not None}: K {e:.2e}, second-order share '
                      f'{rel_err(second[p][m - 1], first[p][m - 1]):.2e}')
                assert e < BAR, (p, m, e)
                assert rel_err(first[p][m - 1], numeric.calculate_cumulant_function(pulse, S, omega)) < BAR
            assert not np.array_equal(second[p][-1], first[p][-1])
        if c is None:
            whole = ff.sequence_cumulant_functions(gates, seqs, S, omega, second_order=True)
            for p in range(len(seqs)):
                assert rel_err(second[p][-1], whole[p]) < BAR, p
    # stacked: the bits of the single calls
    stacked = ff.sequence_prefix_cumulant_functions(gates, seqs, np.stack([S, 2*S]), omega, closing=close,
                                                    second_order=True, stacked=True)
    single = ff.sequence_prefix_cumulant_functions(gates, seqs, 2*S, omega, closing=close, second_order=True)
    assert same([k[1] for k in stacked], single)


def test_indices_exceptions_and_caches():
    omega = wl.rb_omega(20, 1.0, m_max=3)
    S = wl.rb_spectrum(omega, 0.7)
    gates = two_qubit_gates(4, 1, omega, seed=7)
    ff.frequency_shifts(gates, S, omega)                  # (what that call leaves in the gates' caches is its own)
    caches = lambda: [(sorted(g._data), sorted(g._frequency_data),                       # noqa: E731
                       {k: id(g._frequency_data.peek(k)) for k in g._frequency_data}) for g in gates]
    before = caches()
    got = ff.sequence_prefix_frequency_shifts(gates, [[-1, 0, -4], [3, 0, 0]], S, omega, closing=[[-2, 1, 0], [2, -3, 0]])
    assert caches() == before
    assert np.array_equal(got[0], got[1])                                                # negative indices wrap
    for function in (ff.sequence_prefix_frequency_shifts, ff.sequence_prefix_cumulant_functions):
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
    pulse = ff.concatenate([gates[0], gates[1]], calc_second_order_FF=True, omega=omega)
    for kwargs in (dict(spectrum=np.ones(7)), dict(spectrum=S, n_oper_identifiers=['Q'])):
        with pytest.raises(ValueError) as loop_error:
            numeric.calculate_frequency_shifts(pulse, kwargs['spectrum'], omega, kwargs.get('n_oper_identifiers'))
        with pytest.raises(ValueError) as error:
            ff.sequence_prefix_frequency_shifts(gates, [[0, 1]], omega=omega, **kwargs)
        assert str(error.value) == str(loop_error.value)

"""ff.sequence_frequency_shifts and second_order=True of ff.sequence_cumulant_functions /
ff.sequence_error_transfer_matrices: the frequency shifts of many gate sequences given as index arrays into one gate
set, against the forward form of the second-order concatenation rule summed on the host in extended precision from the
same inputs (the Yardstick of test_sequence_infidelities_gpu.py, extended), against the loop over ff.concatenate(...,
calc_second_order_FF=True), against a route that uses no concatenation rule at all, against the reference's fixture,
and against itself in other passes (bit for bit)."""
import numpy as np
import pytest

import ff_oracle as orc
import filter_functions_amd as ff
import workloads as wl
from conftest import load_golden, rel_err
from filter_functions_amd import numeric
from filter_functions_amd import sequence_second_order as so
from filter_functions_amd.sequences import resident_source
from test_gpu_parity import TOL
from test_sequence_infidelities_gpu import CLD, LD, LONG, NAMES, TIGHT, Yardstick, draws, two_qubit_gates
from test_sequence_processes_gpu import BAR, real_spectra, single_qubit_gates

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 63, 64, 65, 130]
LOOPED = (1, 2, 3, 65)             # the lengths at which the loop is evaluated as well


class ShiftYardstick(Yardstick):
    """The forward form of the rule in long double,
        Delta = sum_g [Lam_g^T Delta_gate Lam_g + sum_w trapezoid(w) S_a(w) Re(conj Rs_g[k, w] Cum_{g-1}[l, w]) / 2 pi],
    from the device's inputs: the gates' cached control matrices, total propagators, and Delta_gate as
    ff.frequency_shifts returns it, cast up."""

    def shifts(self, s, S, idx, gate_shifts):
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
        for k in s:
            Rs = phase*(self.v[k][idx] @ Lam)
            delta += Lam.T @ own[k] @ Lam
            delta += np.einsum('iwk,iwl,iw->ikl', Rs.conj(), cum, weight).real
            cum += Rs
            phase = phase*self.p[k]
            Lam = self.L[k].real @ Lam
        return delta


def looped_shifts(gates, seqs, S, omega, names=None):
    table = np.asarray(gates, dtype=object)
    return [numeric.calculate_frequency_shifts(ff.concatenate(table[s], calc_second_order_FF=True, omega=omega), S,
                                               omega, names) for s in seqs]


WORST = {'new': 0.0, 'loop': 0.0}


def check_against_yardstick_and_loop(gates, seqs, omega, names, seed, looped=LOOPED):
    """Every sequence, spectra of one and two dimensions, every (sequence, operator) tile: the new call against the
    yardstick under the project's bars; where the loop is evaluated, within twice the loop's own error and within
    1e-12 of the loop."""
    yard = ShiftYardstick(gates, omega)
    idx = ff.util.get_indices_from_identifiers(gates[0].n_oper_identifiers, names)
    N = len(gates[0].basis)
    bars = [LONG if len(s) >= 500 else TIGHT for s in seqs]
    with_loop = [j for j, s in enumerate(seqs) if len(s) in looped]
    for S in real_spectra(len(idx), omega, seed):
        got, U = ff.sequence_frequency_shifts(gates, seqs, S, omega, n_oper_identifiers=names,
                                              return_propagators=True)
        # (before the loop caches the gates' second-order filter functions: the route the call above took)
        own = ff.frequency_shifts(gates, S, omega, names)
        assert got.shape == (len(seqs), len(idx), N, N) and got.dtype == np.float64
        loop = dict(zip(with_loop, looped_shifts(gates, [seqs[j] for j in with_loop], S, omega, names)))
        for j, s in enumerate(seqs):
            ref = yard.shifts([int(k) % len(gates) for k in s], S, idx, own)
            for a in range(len(idx)):
                new = rel_err(got[j, a], ref[a])
                old = rel_err(loop[j][a], ref[a]) if j in loop else float('nan')
                print(f'd={yard.d} W={len(omega)} A={len(gates[0].n_opers)} T={len(gates)} G={len(s)} '
                      f'S.ndim={np.ndim(S)} operator {a}: Delta new {new:.2e} loop {old:.2e}')
                WORST['new'] = max(WORST['new'], new)
                assert new < bars[j], (j, a, new)
                if j in loop:
                    WORST['loop'] = max(WORST['loop'], old)
                    assert new <= max(2e-13, 2*old), (j, a, new, old)
                    assert rel_err(got[j, a], loop[j][a]) < 1e-12, (j, a)
            total = np.eye(yard.d, dtype=CLD)
            for k in s:
                total = yard.U[int(k) % len(gates)] @ total
            assert rel_err(U[j], total) < bars[j], j
    print(f'worst so far: new {WORST["new"]:.2e}, loop {WORST["loop"]:.2e}')


# ---- accuracy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W, A, T, pauli', [(7, 1, 3, True), (64, 2, 3, False), (65, 3, 3, True), (70, 4, 3, False),
                                            (70, 1, 40, False), (65, 2, 40, True), (64, 3, 40, False),
                                            (7, 4, 40, True)])
def test_two_qubit_gates_against_extended_precision(W, A, T, pauli):
    """T = 3: the tables staged in LDS; T = 40: read from L2.  W: a partial tile of 16 frequencies, a full block, one
    frequency past it, a partial second block.  The loop is evaluated at T = 3."""
    omega = wl.rb_omega(W, 1.0, m_max=3)
    gates = two_qubit_gates(T, A, omega, seed=10*W + A, basis=ff.Basis.pauli(2) if pauli else None)
    assert len(gates[0].basis) == 16 and gates[0].d == 4
    seqs = draws(LENGTHS, W + T, T)
    seqs[2] = np.array([-1, 0, -T])                       # negative indices wrap
    names = None if A == 1 else [NAMES[A - 1], NAMES[0]]    # a subset, not in sorted order
    check_against_yardstick_and_loop(gates, seqs, omega, names, seed=W, looped=LOOPED if T == 3 else (2,))


def test_five_hundred_two_qubit_gates():
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(40, 1, omega, seed=5)
    check_against_yardstick_and_loop(gates, draws([500], 1, 40), omega, None, seed=2, looped=())


@pytest.mark.parametrize('W, A, T', [(301, 1, 24), (7, 2, 3), (64, 3, 3), (65, 4, 3), (65, 4, 24)])
def test_single_qubit_gates_against_extended_precision(W, A, T):
    """A = 1: the Clifford gate set at the study's grid; random gate sets staged in LDS and, the last, read from L2."""
    if A == 1:
        omega = wl.rb_omega(W, wl.CONFIG3['T'])
        gates = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])[1]
    else:
        omega = wl.rb_omega(W, 1.0, m_max=3)
        gates = single_qubit_gates(T, A, omega, seed=W + A)
    names = None if A == 1 else ['B', 'A']
    check_against_yardstick_and_loop(gates, draws([1, 2, 3, 64, 65, 152], W, T), omega, names, seed=A,
                                     looped=LOOPED if T == 3 or A == 1 else (2,))


# ---- other routes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [2, 4])
def test_against_the_joined_segments_without_any_concatenation_rule(d):
    omega = wl.rb_omega(33, 1.0, m_max=3)
    gates = two_qubit_gates(3, 2, omega, seed=21) if d == 4 else single_qubit_gates(3, 2, omega, seed=21)
    S = real_spectra(2, omega, 3)[1]
    seqs = [[0, 1], [2, 0, 1], [1, 1, 2, 0]]
    got = ff.sequence_frequency_shifts(gates, seqs, S, omega)
    table = np.asarray(gates, dtype=object)
    for j, s in enumerate(seqs):
        joined = ff.concatenate_without_filter_function(table[s])
        ref = numeric.calculate_frequency_shifts(joined, S, omega)
        print(f'd={d} G={len(s)}: against the joined segments {rel_err(got[j], ref):.2e}')
        assert rel_err(got[j], ref) < TOL, j


@pytest.mark.parametrize('name', ['q1', 'p4'])
def test_against_the_reference_fixture(name, monkeypatch):
    g = load_golden('second_order_concat')
    omega = g[f'{name}_omega']
    pulses = []
    for i in range(3):
        basis = ff.Basis(g[f'{name}_p{i}_basis'], btype=str(g[f'{name}_p{i}_btype']))
        pulses.append(ff.PulseSequence.from_arrays(
            g[f'{name}_p{i}_c_opers'], g[f'{name}_p{i}_c_oper_identifiers'], g[f'{name}_p{i}_c_coeffs'],
            g[f'{name}_p{i}_n_opers'], g[f'{name}_p{i}_n_oper_identifiers'], g[f'{name}_p{i}_n_coeffs'],
            g[f'{name}_p{i}_dt'], basis))
    S = 1.0/(1.0 + omega**2)
    idx = np.arange(len(pulses[0].n_opers))
    ref = orc.frequency_shifts(g[f'{name}_filter_function_2'], S, omega, idx)
    # both gate sets are eligible and take the pass
    assert so.eligibility(pulses) is not None

    def refuse(*args, **kwargs):
        raise AssertionError('the loop ran')
    monkeypatch.setattr(so, '_loop', refuse)
    monkeypatch.setattr(so, '_single', refuse)
    got = ff.sequence_frequency_shifts(pulses, [[0, 1, 2]], S, omega)
    print(f'{name}: against the reference {rel_err(got[0], ref):.2e}')
    assert got.shape == (1,) + ref.shape and rel_err(got[0], ref) < TOL


@pytest.mark.parametrize('d', [2, 4])
def test_a_sequence_of_one_gate_returns_the_gates_own_shifts(d):
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(4, 3, omega, seed=2) if d == 4 else single_qubit_gates(4, 3, omega, seed=2)
    names = [gates[0].n_oper_identifiers[2], gates[0].n_oper_identifiers[0]]
    for S in real_spectra(2, omega, 5):
        got = ff.sequence_frequency_shifts(gates, [[2], [0], [3, 1], [-1]], S, omega, n_oper_identifiers=names)
        own = ff.frequency_shifts(gates, S, omega, names)
        for j, k in ((0, 2), (1, 0), (3, 3)):
            assert np.array_equal(got[j] + 0.0, own[k] + 0.0), (j, k)
        assert not np.array_equal(got[2], own[3])


# ---- bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d, A, T', [(4, 1, 3), (4, 2, 40), (4, 4, 3), (2, 1, 24), (2, 4, 24)])
def test_a_sequence_does_not_depend_on_its_pass_or_the_split(d, A, T, monkeypatch):
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(T, A, omega, seed=A) if d == 4 else single_qubit_gates(T, A, omega, seed=A)
    S = real_spectra(A, omega, 4)[1]
    probe = draws([77], 8, T)[0]
    others = draws(np.random.default_rng(1).integers(1, 140, 39), 9, T)
    alone = ff.sequence_frequency_shifts(gates, [probe], S, omega, return_propagators=True)
    first = ff.sequence_frequency_shifts(gates, [probe] + others, S, omega, return_propagators=True)
    last = ff.sequence_frequency_shifts(gates, others + [probe], S, omega, return_propagators=True)
    for a, f, l in zip(alone, first, last):
        assert np.array_equal(a[0], f[0]) and np.array_equal(a[0], l[-1])
    # several passes: a budget of the tables and seven sequences
    with monkeypatch.context() as patch:
        longest = max(len(s) for s in [probe] + others)
        patch.setattr(so, 'PASS_BYTES',
                      so.table_bytes(T, d, A, 70, A, 1, 2) + 7*so.pass_bytes(longest, d, A, 70, A, 1))
        calls = []
        run_pass = so._run_pass
        patch.setattr(so, '_run_pass', lambda *args: calls.append(len(args[1])) or run_pass(*args))
        split = ff.sequence_frequency_shifts(gates, others + [probe], S, omega, return_propagators=True)
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
        stacked, U = ff.sequence_frequency_shifts(gates, seqs, S, omega, n_oper_identifiers=names, stacked=True,
                                                  return_propagators=True)
        assert stacked.shape == (3, 4, 2, d*d, d*d)
        for k in range(3):
            single, U_single = ff.sequence_frequency_shifts(gates, seqs, S[k], omega, n_oper_identifiers=names,
                                                            return_propagators=True)
            assert np.array_equal(stacked[k], single) and np.array_equal(U, U_single)


def test_resident_gates_and_host_arrays_give_the_same_bits():
    omega = wl.rb_omega(70, 1.0, m_max=3)
    S = real_spectra(2, omega, 1)[1]
    seqs = draws([1, 2, 17, 64, 100], 6, 4)
    single = two_qubit_gates(4, 2, omega, seed=3)                     # cache_control_matrix: single resident results
    assert all(resident_source(g, 4, 70, 16, 2)[1] == -1 for g in single)
    own = np.stack([ff.frequency_shifts(single, S, omega)])
    # (the gates' own shifts held fixed: the host copies below would take another route through ff.frequency_shifts)
    with pytest.MonkeyPatch.context() as patch:
        patch.setattr(so, '_gate_shifts', lambda gates, spectrum, omega, names: own[0])
        got = ff.sequence_frequency_shifts(single, seqs, S, omega, return_propagators=True)
        host = [ff.PulseSequence(list(zip(g.c_opers, g.c_coeffs, g.c_oper_identifiers)),
                                 list(zip(g.n_opers, g.n_coeffs, g.n_oper_identifiers)), g.dt) for g in single]
        for h, g in zip(host, single):
            h.cache_control_matrix(omega, np.array(g.get_control_matrix(omega)))
            h.total_propagator = np.array(g.total_propagator)
            assert resident_source(h, 4, 70, 16, 2) is None
        # every row uploaded, and a mixed table
        for table in (host, [single[0], host[1], single[2], host[3]]):
            for a, b in zip(got, ff.sequence_frequency_shifts(table, seqs, S, omega, return_propagators=True)):
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
    assert so.eligibility(gates) is not None
    S = wl.rb_spectrum(omega, 0.7)
    probes = draws([1, 30, 152], 3, 24)
    staged = ff.sequence_frequency_shifts(gates, probes, S, omega)
    among = ff.sequence_frequency_shifts(gates, probes + [np.arange(70)], S, omega)
    assert np.array_equal(staged, among[:3])


# ---- second_order=True ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [2, 4])
def test_second_order_cumulant_functions_and_error_transfer_matrices_against_the_loop(d):
    omega = wl.rb_omega(70, 1.0, m_max=3)
    gates = two_qubit_gates(4, 2, omega, seed=11, basis=ff.Basis.pauli(2)) if d == 4 \
        else single_qubit_gates(4, 2, omega, seed=11)
    seqs = draws([1, 2, 5], 5, 4)
    eye = np.eye(d*d)
    S = np.outer([1e-3, 2e-3], 1/omega)
    # the default path: the same bits with the keyword as without it
    for function in (ff.sequence_cumulant_functions, ff.sequence_error_transfer_matrices):
        assert np.array_equal(function(gates, seqs, S, omega), function(gates, seqs, S, omega, second_order=False))
    K = ff.sequence_cumulant_functions(gates, seqs, S, omega, second_order=True)
    U = ff.sequence_error_transfer_matrices(gates, seqs, S, omega, second_order=True)
    first = ff.sequence_cumulant_functions(gates, seqs, S, omega)
    table = np.asarray(gates, dtype=object)
    pulses = [ff.concatenate(table[s], calc_second_order_FF=True, omega=omega) for s in seqs]
    K_ref = np.stack([numeric.calculate_cumulant_function(p, S, omega, second_order=True) for p in pulses])
    U_ref = np.stack([ff.error_transfer_matrix(p, S, omega, second_order=True) for p in pulses])
    assert K.shape == K_ref.shape and U.shape == U_ref.shape == (3, d*d, d*d)
    for j in range(len(seqs)):
        print(f'd={d} G={len(seqs[j])}: K {rel_err(K[j], K_ref[j]):.2e}, U {np.abs(U[j] - U_ref[j]).max():.2e} of '
              f'{np.abs(U_ref[j] - eye).max():.2e}; second-order share {rel_err(K[j], first[j]):.2e}')
        assert rel_err(K[j], K_ref[j]) < BAR, j
        assert np.abs(U[j] - U_ref[j]).max() < BAR*np.abs(U_ref[j] - eye).max() + 1e-15, j
        assert not np.array_equal(K[j], first[j])

"""ff.sequence_prefix_error_transfer_matrices on the GPU: every checked row against the loop over the truncations and the
last row against ff.sequence_error_transfer_matrices, the bits of a curve whatever surrounds it, the fallbacks and the
propagators."""
import numpy as np
import pytest

import filter_functions_amd as ff
import workloads as wl
from filter_functions_amd import expm_batch
from test_processes_gpu import assert_etm_close
from test_sequence_infidelities_gpu import draws, two_qubit_gates
from test_sequence_prefixes_gpu import closers, same
from test_sequence_processes_gpu import BAR, real_spectra, single_qubit_gates

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 65]


def gate_set(d, T, A, omega, seed):
    if d == 4:
        return two_qubit_gates(T, A, omega, seed=seed, basis=ff.Basis.pauli(2))
    return single_qubit_gates(T, A, omega, seed=seed)


def truncation(gates, s, m, close, omega, second_order=False):
    """The loop's pulse of the first m gates of s, closed by gates[close[m - 1]] if *close* is given."""
    table = np.asarray(gates, dtype=object)
    return ff.concatenate(list(table[s[:m]]) + ([gates[close[m - 1]]] if close is not None else []),
                          calc_second_order_FF=second_order, omega=omega)


@pytest.mark.parametrize('second_order', [False, True])
@pytest.mark.parametrize('W, A', [(7, 1), (64, 2), (65, 3)])
@pytest.mark.parametrize('d', [2, 4])
def test_rows_against_the_loop_and_the_whole_sequences(d, W, A, second_order):
    omega = wl.rb_omega(W, 1.0, m_max=3)
    gates = gate_set(d, 3, A, omega, seed=10*d + A)
    seqs = draws(LENGTHS, 3 + A, 3)
    N = d*d
    for S in real_spectra(A, omega, 2):                   # spectra of one and of two dimensions
        for close in (None, closers(seqs, 4, 3)):
            got = ff.sequence_prefix_error_transfer_matrices(gates, seqs, S, omega, closing=close,
                                                             second_order=second_order)
            assert [u.shape for u in got] == [(len(s), N, N) for s in seqs] and all(u.dtype == np.float64 for u in got)
            for p, s in enumerate(seqs):
                for m in sorted({1, 2, len(s)} & set(range(1, len(s) + 1))):
                    pulse = truncation(gates, s, m, None if close is None else close[p], omega, second_order)
                    ref = ff.error_transfer_matrix(pulse, S, omega, second_order=second_order)
                    assert_etm_close(got[p][m - 1], ref, BAR)
            if close is None:
                whole = ff.sequence_error_transfer_matrices(gates, seqs, S, omega, second_order=second_order)
                for p in range(len(seqs)):
                    assert_etm_close(got[p][-1], whole[p], BAR)


@pytest.mark.parametrize('d', [2, 4])
def test_a_curve_has_the_same_bits_alone_among_forty_truncated_and_stacked(d):
    omega = wl.rb_omega(33, 1.0, m_max=3)
    gates = gate_set(d, 3, 2, omega, seed=d)
    S = real_spectra(2, omega, 5)[1]
    probe = draws([65], 8, 3)[0]
    others = draws(np.random.default_rng(1).integers(1, 70, 39), 9, 3)
    for close in (None, closers([probe] + others, 5, 3)):
        def curve(seqs, c, **kw):
            return ff.sequence_prefix_error_transfer_matrices(gates, seqs, S, omega, closing=c, second_order=True,
                                                              **kw)
        alone = curve([probe], None if close is None else close[:1])
        among = curve(others[:20] + [probe] + others[20:],
                      None if close is None else close[1:21] + close[:1] + close[21:])
        assert np.array_equal(among[20], alone[0])
        for m in (1, 63, 64, 65):
            cut = curve([probe[:m]], None if close is None else [close[0][:m]])
            assert np.array_equal(cut[0], alone[0][:m]), m
    # stacked: slice k is the single call's
    spectra = np.stack([S, 2*S, 0.5*S])
    seqs = [probe] + others[:4]
    stacked = ff.sequence_prefix_error_transfer_matrices(gates, seqs, spectra, omega, second_order=True, stacked=True)
    assert [u.shape for u in stacked] == [(3, len(s), d*d, d*d) for s in seqs]
    for k in range(3):
        single = ff.sequence_prefix_error_transfer_matrices(gates, seqs, spectra[k], omega, second_order=True)
        assert same([u[k] for u in stacked], single), k


def test_fallbacks_and_propagators():
    omega = wl.rb_omega(20, 1.0, m_max=3)
    rng = np.random.default_rng(3)
    d4 = gate_set(4, 3, 2, omega, seed=1)
    C = rng.random((2, 2, 20)) + 1j*rng.random((2, 2, 20))
    cross = 1e-2*(C + C.conj().swapaxes(0, 1))
    spin1 = [ff.PulseSequence([[np.diag([1.0, 0.0, -1.0]), [0.3 + 0.1*k], 'Z']],
                              [[np.diag([1.0, -1.0, 0.0]), [1.0], 'N']], [1.0]) for k in range(2)]
    for g in spin1:
        g.cache_control_matrix(omega)
    S = wl.rb_spectrum(omega, 0.7)
    for gates, seqs, spectrum in ((d4, [np.array([0, 1, 2]), np.array([2, 2])], cross),
                                  (spin1, [np.array([0, 1]), np.array([1, 1, 0])], S)):
        N = gates[0].basis.shape[0]
        for close in (None, closers(seqs, 7, len(gates))):
            got, U = ff.sequence_prefix_error_transfer_matrices(gates, seqs, spectrum, omega, closing=close,
                                                                return_propagators=True)
            K, U_K = ff.sequence_prefix_cumulant_functions(gates, seqs, spectrum, omega, closing=close,
                                                           return_propagators=True)
            assert same(U, U_K)             # (the loop's propagators on these routes, as that call returns them)
            for p, s in enumerate(seqs):
                assert got[p].shape == (len(s), N, N)
                for m in range(1, len(s) + 1):
                    pulse = truncation(gates, s, m, None if close is None else close[p], omega)
                    ref = ff.error_transfer_matrix(pulse, spectrum, omega)
                    assert_etm_close(np.asarray(got[p][m - 1]), np.asarray(ref), BAR)
                    # the exponential of the loop's cumulant function, summed over both operator axes
                    assert np.array_equal(got[p][m - 1],
                                          ff.exponentiate_cumulant_functions(np.asarray(K[p][m - 1])[None])[0])


def test_every_position_goes_through_one_exponential(monkeypatch):
    omega = wl.rb_omega(20, 1.0, m_max=3)
    gates = gate_set(2, 3, 2, omega, seed=2)
    seqs = draws([5, 1, 9], 1, 3)
    S = np.stack(real_spectra(2, omega, 6)[1:]*2)
    shapes = []
    real = expm_batch.exponentiate_cumulant_functions

    def counting(tiles):
        shapes.append(np.shape(tiles))
        return real(tiles)
    monkeypatch.setattr(expm_batch, 'exponentiate_cumulant_functions', counting)
    ff.sequence_prefix_error_transfer_matrices(gates, seqs, S, omega, stacked=True)
    assert shapes == [(2*15, 2, 4, 4)]

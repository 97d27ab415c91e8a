"""The d = 4 accumulate kernel's two producer forms on the same inputs (GPU test): W_a folded by the prologue and
copied into the ring by LDS-DMA (PRE = true: the control-matrix call) against W_a folded by the producers
(PRE = false: the per-segment steps of cache_intermediates=True), for A = 1 ... 8 -- every operator-group plan of
a launch (3, 2, 1 operators per block and the mixed 3 + 2 / 2 + 2 / 3 + 2 + 2 plans).  Reference loop:
numeric.py:846-869."""
import numpy as np
import pytest

import filter_functions_amd as ff
from conftest import rel_err
from filter_functions_amd import numeric


def _inputs(A, G, W, seed):
    rng = np.random.default_rng(seed)
    d = 4

    def herm(n):
        x = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
        return x + x.conj().transpose(0, 2, 1)
    c_opers = herm(3)
    c_coeffs = rng.standard_normal((3, G))
    H = np.einsum('ig,ijk->gjk', c_coeffs, c_opers)
    dt = 1 - rng.random(G)
    D, V, Q = numeric.diagonalize(H, dt)
    n_opers = herm(A)
    n_coeffs = rng.random((A, G))
    omega = np.geomspace(1e-2/dt.sum(), 1e2/dt.min(), W)
    basis = np.asarray(ff.Basis.pauli(2))
    return D, V, Q, omega, basis, n_opers, n_coeffs, dt


@pytest.mark.gpu
@pytest.mark.parametrize('A', range(1, 9))
def test_folded_operands_by_dma_match_the_producer_fold(A):
    G, W = 37, 200              # several tiles per block and producer; the last frequency block is partial
    D, V, Q, omega, basis, n_opers, n_coeffs, dt = _inputs(A, G, W, seed=100 + A)
    R, inter = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt,
                                                             cache_intermediates=True)
    steps = inter['control_matrix_step']
    assert steps.shape == (G, A, 16, W)
    # one segment per block (PRE = false) summed over the segments against the ring of tiles (PRE = true)
    assert rel_err(R, steps.sum(axis=0)) < 1e-13
    # and the DMA-fed kernel is deterministic
    again = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
    assert np.array_equal(again, R)


@pytest.mark.gpu
def test_single_segment_forms_are_bit_identical():
    """With one segment both forms compute the same products in the same order: bit-identical."""
    for A in (1, 2, 3, 5):
        D, V, Q, omega, basis, n_opers, n_coeffs, dt = _inputs(A, 1, 130, seed=7 + A)
        R, inter = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt,
                                                                 cache_intermediates=True)
        assert np.array_equal(R, inter['control_matrix_step'][0]), A

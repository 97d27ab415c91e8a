"""The d = 4 accumulate kernel where its producers meet entries next to a resonance (GPU test).

A producer evaluates the real factor q = 2 sin((w + dE) dt/2)/(w + dE) of an entry from the addition theorem, and
from the short sine polynomial where |w + dE| < 2^-4/dt (ffk_math.h::phased_q, ctrl_pq.hip).  The diagonal entry
has dE = 0, so that every frequency below 2^-4/dt takes the second form for every segment: on a logarithmic grid
that is the common case, not a rare one.  The frequencies here are built per 64-frequency tile of the kernel
(lane = frequency, the near form is entered per wavefront):

    tile 0   w = 0 and 63 frequencies below 2^-4/max(dt): every lane near on the diagonal, for every segment
    tile 1   both sides of 2^-4/dt_g of several segments, and frequencies in between: mixed lanes
    tile 2   -dE (1 + eps), eps in {0, +-2^-52, 1e-12}, and both sides of |x dt| = 2^-4, for off-diagonal level
             pairs of two segments
    tile 3   (ragged: 8 frequencies, 1e2 ... 1e3) far above every threshold and level splitting

G = 13 segments: the ring of eight slots is reused, the four producers get 4, 3, 3, 3 tiles; one segment is idle
(H = 0: every entry is a diagonal entry) and one has zero length (the threshold is +inf: every entry near).

Bit identity of the two producer forms (W_a folded by the prologue and copied in by LDS-DMA, against W_a folded
by the producers: the per-segment steps of cache_intermediates=True) holds where both sum the same products in
the same order, which is one segment per block (tests/test_pq_folded_operands_gpu.py): the sum over 13 segments is
formed in the matrix cores' accumulators by the one and on the host by the other.  So every segment is evaluated
alone by both forms and compared with np.array_equal, and the whole pulse with that file's bound, 1e-13.
"""
import numpy as np
import pytest

import ff_oracle as orc
import filter_functions_amd as ff
from conftest import rel_err
from filter_functions_amd import _lib, numeric

pytestmark = pytest.mark.gpu

G, W, D = 13, 200, 4
IDLE, EMPTY = 4, 7           # the idle segment and the zero-length one
TIGHT = 2e-13                # tests/test_gpu_parity.py::test_segment_chunking_is_result_invariant


def _herm(rng, n):
    x = rng.standard_normal((n, D, D)) + 1j*rng.standard_normal((n, D, D))
    return x + x.conj().transpose(0, 2, 1)


_CACHE = {}


def _pulse():
    """The segments and the frequency tiles, once for all tests of the file."""
    if 'pulse' in _CACHE:
        return _CACHE['pulse']
    rng = np.random.default_rng(2024)
    H = np.einsum('ijk,il->ljk', _herm(rng, 3), rng.standard_normal((3, G)))
    H[IDLE] = 0.0
    dt = 0.5 + rng.random(G)
    dt[EMPTY] = 0.0
    eigvals, eigvecs, propagators = numeric.diagonalize(H, dt)
    live = dt > 0
    thr = 0.0625/dt[live]
    tile0 = np.concatenate(([0.0], np.geomspace(1e-7, 0.9*thr.min(), 63)))
    tile1 = []
    for g in (0, 2, 5, 9, 12):
        for nudge in (1 - 2.0**-40, 1 + 2.0**-40, 0.97, 1.03):
            tile1.append(0.0625/dt[g]*nudge)
    tile1 = np.concatenate((tile1, np.linspace(0.5*thr.min(), 2*thr.max(), 64 - len(tile1))))
    tile2 = []
    for g in (1, G - 1):
        dE = (eigvals[g][:, None] - eigvals[g][None, :]).ravel()
        dE = dE[dE != 0][:4]
        for eps in (0.0, 2.0**-52, -2.0**-52, 1e-12):
            tile2.extend(-dE*(1 + eps))
        for edge in (2.0**-4, -2.0**-4):
            for nudge in (1 - 2.0**-40, 1 + 2.0**-40):
                tile2.extend(-dE + edge*nudge/dt[g])
    # (not higher: the reference rounds the argument w t_g of its phase factor, which costs it w t u = 1e-12 of a
    # column at w = 1e3, t = 10 -- at w = 1e5 that rounding alone is worth 1e-10 and the bound per column of 1e-11
    # below would measure the oracle)
    tile3 = np.geomspace(1e2, 1e3, 8)
    omega = np.concatenate((tile0, tile1, tile2, tile3))
    assert omega.shape == (W,) and len(tile0) == len(tile1) == len(tile2) == 64
    assert (np.abs(tile0) < thr.min()).all() and (tile3 > 100*thr.max()).all()
    _CACHE['pulse'] = eigvals, eigvecs, propagators, dt, omega
    return _CACHE['pulse']


def _case(A):
    """Operators, the control matrix of both producer forms and the oracle's, once per operator count."""
    if A in _CACHE:
        return _CACHE[A]
    eigvals, eigvecs, propagators, dt, omega = _pulse()
    rng = np.random.default_rng(500 + A)
    n_opers = _herm(rng, A)
    n_coeffs = rng.random((A, G)) + 0.5
    basis = np.asarray(ff.Basis.pauli(2))
    R, inter = numeric.calculate_control_matrix_from_scratch(eigvals, eigvecs, propagators, omega, basis, n_opers,
                                                             n_coeffs, dt, cache_intermediates=True)
    t = np.concatenate(([0], dt.cumsum()))
    R_ref = orc.control_matrix_from_scratch(eigvals, eigvecs, propagators, omega, basis, n_opers, n_coeffs, dt, t)
    _CACHE[A] = basis, n_opers, n_coeffs, t, R, inter['control_matrix_step'], R_ref
    return _CACHE[A]


@pytest.mark.parametrize('A', [1, 2, 3, 4])
def test_near_resonance_tiles_match_the_oracle(A):
    _, _, _, _, omega = _pulse()
    _, _, _, _, R, _, R_ref = _case(A)
    assert R.shape == (A, 16, W)
    assert np.isfinite(R).all()
    err = rel_err(R, R_ref)
    num = np.abs(R - R_ref).max(axis=(0, 1))
    den = np.abs(R_ref).max(axis=(0, 1))
    print(f'A={A}: rel_err {err:.2e}, worst column {np.max(num/den):.2e} at omega = {omega[np.argmax(num/den)]!r}')
    assert err < 1e-12
    # frequency by frequency, so that one bad column cannot hide behind the norm of the rest
    assert (num <= 1e-11*den).all(), omega[np.argmax(num/den)]


@pytest.mark.parametrize('A', [1, 2, 3, 4])
def test_both_producer_forms_agree(A):
    eigvals, eigvecs, propagators, dt, omega = _pulse()
    basis, n_opers, n_coeffs, t, R, steps, _ = _case(A)
    assert steps.shape == (G, A, 16, W)
    print(f'A={A}: whole pulse, DMA form against the summed steps: {rel_err(R, steps.sum(axis=0)):.2e}')
    assert rel_err(R, steps.sum(axis=0)) < 1e-13
    # one segment per launch: the same products in the same order, bit for bit
    for g in range(G):
        Rg, inter = numeric.calculate_control_matrix_from_scratch(
            eigvals[g:g + 1], eigvecs[g:g + 1], propagators[g:g + 2], omega, basis, n_opers, n_coeffs[:, g:g + 1],
            dt[g:g + 1], t[g:g + 2], cache_intermediates=True)
        assert np.array_equal(Rg, inter['control_matrix_step'][0]), g
        # and the segment alone is the pulse's step
        assert np.array_equal(Rg, steps[g]), g


@pytest.mark.parametrize('A', [1, 2, 3, 4])
def test_forced_chunk_counts_agree(A):
    eigvals, eigvecs, propagators, dt, omega = _pulse()
    basis, n_opers, n_coeffs, t, R, _, R_ref = _case(A)
    lib = _lib.load()
    results = []
    try:
        for chunks in (1, 3):
            _lib.check(lib.ffk_set_segment_chunks(chunks))
            results.append(numeric.calculate_control_matrix_from_scratch(eigvals, eigvecs, propagators, omega, basis,
                                                                         n_opers, n_coeffs, dt, t))
            assert _lib.stats()['chunks'] == chunks
    finally:
        lib.ffk_set_segment_chunks(0)
    print(f'A={A}: chunks 1 against 3: {rel_err(results[0], results[1]):.2e}')
    assert rel_err(results[0], results[1]) < TIGHT
    for Rc in results:
        assert np.isfinite(Rc).all() and rel_err(Rc, R_ref) < 1e-12

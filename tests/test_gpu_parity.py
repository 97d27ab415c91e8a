"""GPU parity tests: the HIP path, called through the C ABI (ctypes), against
(i) golden fixtures generated from the upstream reference, (ii) the reference's own golden
infidelity vector and analytic DD formulas, (iii) the CPU oracle on seeded inputs up to the full
BASELINE config-2 size, (iv) size-independent properties.

Tolerance contract (DESIGN.md "Numerics"): for a complex tensor T, max|T - T_ref| <=
tol * max|T_ref| with tol = 1e-10 as the acceptance bar of BASELINE.json; the assertions below
use the much tighter values the implementation actually reaches so that regressions show.
"""
import os
import numpy as np
import pytest

import ff_oracle as orc
import filter_functions_amd as ff
from conftest import ROOT, load_golden, rel_err
from filter_functions_amd import _lib, gradient, numeric, util

pytestmark = pytest.mark.gpu

RAND = ['rand_d2_ggm', 'rand_d3_ggm', 'rand_d4_pauli', 'rand_d4_ggm', 'rand_d5_ggm',
        'rand_d8_pauli', 'rand_d16_ggm', 'edge_degenerate_d4', 'edge_single_segment_d2',
        'cfg2_small', 'hadamard',
        'rand_d17_ggm', 'rand_d20_ggm', 'rand_d32_pauli']     # d > 16: csrc/generic.hip
TOL = 1e-10          # acceptance bar (north_star)
TIGHT = 2e-13        # what the kernels reach on O(1) data


def pulse_from(g):
    basis = ff.Basis(g['basis'], btype=str(g['btype']))
    return ff.PulseSequence.from_arrays(g['c_opers'], g['c_oper_identifiers'], g['c_coeffs'],
                                        g['n_opers'], g['n_oper_identifiers'], g['n_coeffs'],
                                        g['dt'], basis)


def test_native_library_is_the_one_running():
    assert _lib.device_count() >= 1
    name, cus, mem = _lib.device_info()
    assert 'gfx950' in name, name
    assert cus >= 200 and mem > 100e9


@pytest.mark.parametrize('name', RAND)
def test_diagonalize(name):
    g = load_golden(name)
    D, V, Q = numeric.diagonalize(g['H'], g['dt'])
    assert D.shape == g['eigvals'].shape and V.shape == g['eigvecs'].shape
    assert Q.shape == g['propagators'].shape
    scale = max(1.0, np.abs(g['H']).max())
    assert np.abs(D - g['eigvals']).max() < 1e-13*scale
    assert rel_err(Q, g['propagators']) < 1e-12
    assert np.array_equal(Q[0], np.eye(D.shape[1]))
    assert np.all(np.diff(D, axis=1) >= 0)                      # ascending like eigh
    for k in range(len(D)):                                     # tests/testutil.py:41-57
        v = V[k]
        assert np.abs(v.conj().T @ v - np.eye(len(v))).max() < 1e-13
        assert np.abs(v.conj().T @ g['H'][k] @ v - np.diag(D[k])).max() < 2e-13*scale


def test_diagonalize_reads_lower_triangle_only():
    g = load_golden('rand_d4_pauli')
    H = g['H'].copy()
    H[:, 0, 3] = 123.0                                          # garbage in the upper triangle
    H[:, 1, 1] += 5j                                            # and on the diagonal's imag part
    D, V, Q = numeric.diagonalize(H, g['dt'])
    assert np.abs(D - g['eigvals']).max() < 1e-13
    assert rel_err(Q, g['propagators']) < 1e-12


@pytest.mark.parametrize('name', RAND)
def test_control_matrix_from_reference_eigensystem(name):
    g = load_golden(name)
    R = numeric.calculate_control_matrix_from_scratch(
        g['eigvals'], g['eigvecs'], g['propagators'], g['omega'], g['basis'], g['n_opers'],
        g['n_coeffs'], g['dt'], g['t'])
    assert R.shape == g['control_matrix'].shape and R.dtype == np.complex128
    assert R.flags.c_contiguous
    assert rel_err(R, g['control_matrix']) < TIGHT
    # t=None must give the same (reference numeric.py:796-797)
    R2 = numeric.calculate_control_matrix_from_scratch(
        g['eigvals'], g['eigvecs'], g['propagators'], g['omega'], g['basis'], g['n_opers'],
        g['n_coeffs'], g['dt'])
    assert np.array_equal(R, R2)
    # out= is written in place
    out = np.full_like(R, 7)
    R3 = numeric.calculate_control_matrix_from_scratch(
        g['eigvals'], g['eigvecs'], g['propagators'], g['omega'], g['basis'], g['n_opers'],
        g['n_coeffs'], g['dt'], g['t'], out=out)
    assert R3 is out and np.array_equal(out, R)


@pytest.mark.parametrize('name', RAND)
def test_noise_operators(name):
    g = load_golden(name)
    B = numeric.calculate_noise_operators_from_scratch(
        g['eigvals'], g['eigvecs'], g['propagators'], g['omega'], g['n_opers'], g['n_coeffs'],
        g['dt'], g['t'])
    assert B.shape == g['noise_operators'].shape
    assert rel_err(B, g['noise_operators']) < TIGHT
    # Hilbert vs Liouville consistency, tests/test_precision.py:313-353
    R = orc.basis_expand(B, g['basis']).transpose(1, 2, 0)
    assert rel_err(R, g['control_matrix']) < TIGHT


@pytest.mark.parametrize('name', RAND)
def test_pulse_sequence_end_to_end(name):
    """PulseSequence.get_filter_function / infidelity, own eigensolver (gauge-invariant outputs)."""
    g = load_golden(name)
    pulse = pulse_from(g)
    omega = g['omega']
    F = pulse.get_filter_function(omega)
    assert rel_err(F, g['filter_function']) < 1e-12
    assert rel_err(pulse.get_control_matrix(omega), g['control_matrix']) < 1e-12
    assert np.abs(pulse.eigvals - g['eigvals']).max() < 1e-13*max(1, np.abs(g['H']).max())
    assert rel_err(pulse.propagators, g['propagators']) < 1e-12
    L = pulse.total_propagator_liouville
    if 'total_propagator_liouville_rows' in g:                   # large d: every 37th row is stored
        L = L[g['total_propagator_liouville_rows']]
    assert rel_err(L, g['total_propagator_liouville']) < 1e-12
    # diagonal of F is real and non-negative (tests/test_core.py:750-760)
    for a in range(F.shape[0]):
        assert np.abs(F[a, a].imag).max() <= 1e-15*max(1, np.abs(F).max())
        assert (F[a, a].real >= 0).all()
    assert np.allclose(F, F.conj().swapaxes(0, 1), atol=0, rtol=1e-14)
    # caching semantics: memoised by reference, list/array omega equivalent, re-query with a
    # different grid recomputes (tests/test_core.py:644-683, :802)
    assert pulse.get_filter_function(list(omega)) is F
    assert pulse.is_cached('filter function') and pulse.is_cached('control matrix')
    F2 = pulse.get_filter_function(omega + 1)
    assert F2 is not F and not np.array_equal(F2, F)
    if 'filter_function_gen' in g:
        pulse = pulse_from(g)
        Fg = pulse.get_filter_function(omega, which='generalized')
        assert rel_err(Fg, g['filter_function_gen']) < 1e-12
        assert rel_err(pulse.get_filter_function(omega), g['filter_function']) < 1e-12
        assert rel_err(Fg.trace(axis1=2, axis2=3), g['filter_function']) < 1e-12
    if 'infidelity_S1' in g:
        pulse = pulse_from(g)
        for key in ('S1', 'S2', 'S3'):
            got = ff.infidelity(pulse, g[key], omega)
            assert got.shape == g['infidelity_' + key].shape and got.dtype == np.float64
            assert rel_err(got, g['infidelity_' + key]) < 1e-12, key
        if 'subset_identifiers' in g:
            ids = [str(s) for s in g['subset_identifiers']]
            A = len(g['n_opers'])
            sel = np.ix_([A - 1, 0], [A - 1, 0])
            assert rel_err(ff.infidelity(pulse, g['S1'], omega, n_oper_identifiers=ids),
                           g['infidelity_S1_subset']) < 1e-12
            assert rel_err(ff.infidelity(pulse, g['S3'][sel], omega, n_oper_identifiers=ids),
                           g['infidelity_S3_subset']) < 1e-12


def test_reference_golden_infidelity_vector():
    """tests/test_precision.py:495-551: seeded pulses, 15 literal results, atol 1e-12."""
    g = load_golden('test_infidelity')
    omega = g['omega']
    for d in (2, 3, 4):
        pulse = ff.PulseSequence.from_arrays(
            g[f'd{d}_c_opers'], g[f'd{d}_c_oper_identifiers'], g[f'd{d}_c_coeffs'],
            g[f'd{d}_n_opers'], np.array(['B_0', 'B_2', 'B_x']), g[f'd{d}_n_coeffs'],
            g[f'd{d}_dt'], ff.Basis.ggm(d))
        for s in range(5):
            S = g[f'd{d}_S{s}']
            got = ff.infidelity(pulse, S, omega, n_oper_identifiers=['B_0', 'B_2'])
            np.testing.assert_allclose(got, g[f'd{d}_ref_infid{s}'], atol=1e-12, rtol=0)
            if S.ndim == 3:
                diag = ff.infidelity(pulse, S[range(2), range(2)], omega,
                                     n_oper_identifiers=['B_0', 'B_2'])
                np.testing.assert_allclose(np.diag(got), diag, rtol=1e-13)
                assert np.array_equal(got, got.conj().T)


def test_hadamard_readme_example():
    g = load_golden('hadamard')
    X, Y, Z = util.paulis[1:]
    pulse = ff.PulseSequence([[X/2, [0, np.pi], 'X'], [Y/2, [np.pi/2, 0], 'Y']],
                             [[Z/2, [1, 1], 'Z']], [1, 1])
    omega = util.get_sample_frequencies(pulse, n_samples=200)
    infid = ff.infidelity(pulse, 1e-2/omega, omega)
    assert rel_err(infid, g['infidelity']) < 1e-12
    assert abs(infid[0] - 0.0025) < 1e-4                       # README.md:58-60
    assert rel_err(pulse.get_filter_function(omega), g['filter_function']) < 1e-12


@pytest.mark.parametrize('key,n', [('cpmg6', 6), ('udd6', 6), ('pdd6', 6), ('cdd3', 3),
                                   ('cpmg1', 1)])
def test_dynamical_decoupling_analytic(key, n):
    """Closed forms of filter_functions/analytic.py:59-88 (tests/test_precision.py:75-182):
    pi-pulses of 1e-9 duration (|H| ~ 3e9), two-sided omega grid."""
    g = load_golden('dynamical_decoupling')
    omega = g['omega']
    X, Z = util.paulis[1], util.paulis[3]
    dt = g[key + '_dt']
    pulse = ff.PulseSequence([[X/2, g[key + '_c_coeffs']]], [[Z/2, np.ones_like(dt)]], dt)
    F = pulse.get_filter_function(omega)[0, 0]
    np.testing.assert_allclose((F*omega**2).real, g[key + '_analytic'], atol=1e-10, rtol=1e-7)
    assert rel_err(F, g[key + '_F']) < 1e-11


def test_liouville_representation():
    g = load_golden('liouville')
    for tag in ('d2_pauli', 'd3_ggm', 'd4_pauli', 'd4_ggm', 'd8_pauli', 'd16_ggm', 'd3_nonherm'):
        basis = ff.Basis(g[tag + '_basis'])
        L = ff.liouville_representation(g[tag + '_U'], basis)
        assert L.dtype == g[tag + '_L'].dtype and L.shape == g[tag + '_L'].shape
        assert rel_err(L, g[tag + '_L']) < 1e-14, tag
    # single unitary (no batch axis); orthogonality, tests/test_superoperator.py:35-74
    U = g['d4_pauli_U'][0]
    L = ff.liouville_representation(U, ff.Basis.pauli(2))
    assert L.shape == (16, 16)
    assert np.abs(L.T @ L - np.eye(16)).max() < 5*np.finfo(float).eps*16
    # Pauli conjugation signs for d = 2: U = X maps (I,X,Y,Z) -> (I,X,-Y,-Z)
    L = ff.liouville_representation(util.paulis[1], ff.Basis.pauli(1))
    assert np.allclose(L, np.diag([1, 1, -1, -1]), atol=1e-15)


@pytest.mark.parametrize('d,batch,hermitian', [(8, 5, True), (8, 3, False), (12, 4, True), (12, 2, False),
                                               (16, 3, True), (16, 2, False), (4, 7, False)])
def test_liouville_representation_against_the_oracle(d, batch, hermitian):
    """U^dag C_i U on the matrix cores (d = 12, 16: conjugate_basis_mfma_kernel) and all elements of a
    block at once (d = 8), Hermitian and non-Hermitian bases (real resp. complex result), batch sizes
    that leave the last element block partly empty -- against the oracle's einsum."""
    rng = np.random.default_rng(1000*d + batch)
    basis = np.array(ff.Basis.ggm(d))
    if not hermitian:
        # orthonormal but not Hermitian: unitary mixtures of pairs of GGM elements (as in the
        # reference-generated d = 3 fixture)
        for k in range(1, d*d - 1, 3):
            a, b = basis[k].copy(), basis[k + 1].copy()
            basis[k], basis[k + 1] = (a + 1j*b)/np.sqrt(2), (a - 1j*b)/np.sqrt(2)
    H = rng.standard_normal((batch, d, d)) + 1j*rng.standard_normal((batch, d, d))
    U = np.linalg.qr(H)[0]
    L = ff.liouville_representation(U, ff.Basis(basis))
    ref = orc.liouville_representation(U, basis)
    assert L.shape == ref.shape
    assert np.iscomplexobj(L) == (not hermitian)
    assert rel_err(L, ref) < 1e-13


@pytest.mark.parametrize('d,kind,batch', [(16, 'pauli', 3), (16, 'ggm', 2), (12, 'ggm', 5), (16, 'rotated pairs', 2),
                                          (12, 'rotated pairs', 3), (16, 'dense', 2), (12, 'dense', 2),
                                          (16, 'pauli, one element dense', 2)])
def test_liouville_representation_fused_with_a_sparse_operand(d, kind, batch):
    """d = 12, 16 with a Hermitian basis: when every element has at most 32 non-zero operand rows the conjugation
    kernel contracts its tile with them itself (conjugate_basis_mfma_kernel<D, true, true>, liouville.hip) and no
    GEMM runs; otherwise the two-kernel form does.  Pauli (8 or 16 rows per element), GGM (1, 2 or d), a basis
    rotated by 2 x 2 blocks (lists of more than one batch of eight), dense Hermitian bases and a sparse basis with ONE
    dense element (the device-side switch) -- against the oracle's plain trace (superoperator.py:51-84)."""
    rng = np.random.default_rng(31*d + batch)
    base = np.array(ff.Basis.pauli(4) if kind.startswith('pauli') else ff.Basis.ggm(d))
    if kind == 'rotated pairs':
        V = np.zeros((d, d), dtype=complex)
        for a in range(0, d, 2):
            V[a:a + 2, a:a + 2] = np.linalg.qr(rng.standard_normal((2, 2)) + 1j*rng.standard_normal((2, 2)))[0]
        base = V @ base @ V.conj().T
    elif kind == 'dense':
        V = np.linalg.qr(rng.standard_normal((d, d)) + 1j*rng.standard_normal((d, d)))[0]
        base = V @ base @ V.conj().T
    elif kind == 'pauli, one element dense':
        M = rng.standard_normal((d, d)) + 1j*rng.standard_normal((d, d))
        base[77] = (M + M.conj().T)/np.linalg.norm(M + M.conj().T)
    U = np.linalg.qr(rng.standard_normal((batch, d, d)) + 1j*rng.standard_normal((batch, d, d)))[0]
    U[-1] = rng.standard_normal((d, d)) + 1j*rng.standard_normal((d, d))        # (and one that is not unitary)
    L = ff.liouville_representation(U, ff.Basis(base))
    ref = orc.liouville_representation(U, base)
    assert not np.iscomplexobj(L) and L.shape == ref.shape
    assert rel_err(L, ref) < 1e-13


@pytest.mark.parametrize('d,batch', [(2, 3), (3, 5), (5, 4), (7, 2), (8, 5), (12, 3), (16, 2), (20, 2), (32, 1)])
def test_liouville_representation_of_any_operator_in_a_hermitian_basis(d, batch):
    """For a Hermitian basis the library contracts d^2 operand rows instead of 2 d^2: U^dag C_i U is
    Hermitian whenever C_i is -- WHATEVER U -- so the entries a <= b carry the whole trace
    (csrc/ffk_internal.h::hermitian_operand_row).  Checked with operators that are NOT unitary, on
    every conjugation kernel (tile: d = 2..7, rows: 8, matrix cores: 12 / 16, runtime-d: 20 / 32; the
    GEMM through LDS at N = 256, 1024) against the oracle's plain trace (superoperator.py:51-84)."""
    rng = np.random.default_rng(77*d + batch)
    basis = ff.Basis.ggm(d)
    U = rng.standard_normal((batch, d, d)) + 1j*rng.standard_normal((batch, d, d))
    L = ff.liouville_representation(U, basis)
    ref = orc.liouville_representation(U, np.asarray(basis))
    assert not np.iscomplexobj(L) and L.shape == ref.shape
    assert rel_err(L, ref) < 1e-13


@pytest.mark.parametrize('name', ['rand_d2_ggm', 'rand_d3_ggm', 'rand_d4_pauli', 'rand_d4_ggm',
                                  'edge_degenerate_d4'])
def test_intermediates(name):
    """cache_intermediates=True products, tests/test_core.py:604-642."""
    g = load_golden(name)
    R, inter = numeric.calculate_control_matrix_from_scratch(
        g['eigvals'], g['eigvecs'], g['propagators'], g['omega'], g['basis'], g['n_opers'],
        g['n_coeffs'], g['dt'], g['t'], cache_intermediates=True)
    assert rel_err(R, g['control_matrix']) < TIGHT
    for key in ('n_opers_transformed', 'eigvecs_propagated', 'basis_transformed',
                'phase_factors', 'first_order_integral', 'control_matrix_step'):
        assert inter[key].shape == g['inter_' + key].shape, key
        assert rel_err(inter[key], g['inter_' + key]) < TIGHT, key
    assert rel_err(inter['control_matrix_step'].sum(0), R) < TIGHT
    cum = np.cumsum(g['inter_control_matrix_step'], axis=0)[:-1]
    assert rel_err(inter['control_matrix_step_cumulative'], cum) < TIGHT
    # through the PulseSequence front-end: intermediates land in pulse.intermediates and a
    # leading slice reuses the cumulative cache (pulse_sequence.py:462-473)
    pulse = pulse_from(g)
    pulse.get_control_matrix(g['omega'], cache_intermediates=True)
    assert set(pulse.intermediates) >= {'control_matrix_step', 'phase_factors'}
    if len(pulse) > 2:
        head = pulse[:2]
        assert head.is_cached('control_matrix')
        fresh = pulse_from(g)[:2]
        assert rel_err(head.get_control_matrix(g['omega']), fresh.get_control_matrix(g['omega'])) < 1e-12


def test_segment_chunking_is_result_invariant():
    """The split of the segment axis over blocks only re-associates the sum."""
    g = load_golden('cfg2_small')
    args = (g['eigvals'], g['eigvecs'], g['propagators'], g['omega'], g['basis'], g['n_opers'],
            g['n_coeffs'], g['dt'], g['t'])
    lib = _lib.load()
    results = []
    try:
        for chunks in (1, 2, 7, 64, 0):
            _lib.check(lib.ffk_set_segment_chunks(chunks))
            results.append(numeric.calculate_control_matrix_from_scratch(*args))
            if chunks:
                assert _lib.stats()['chunks'] == min(chunks, 64) or chunks == 7
    finally:
        lib.ffk_set_segment_chunks(0)
    for R in results:
        assert rel_err(R, g['control_matrix']) < TIGHT
    # and the run is deterministic: same geometry -> bit-identical
    again = numeric.calculate_control_matrix_from_scratch(*args)
    assert np.array_equal(again, results[-1])


def test_ragged_and_tiny_shapes():
    """W not a multiple of 64, W = 1, a single noise operator, one segment."""
    g = load_golden('rand_d3_ggm')
    for W in (1, 2, 63, 65):
        omega = np.linspace(-3, 7, W)
        R = numeric.calculate_control_matrix_from_scratch(
            g['eigvals'], g['eigvecs'], g['propagators'], omega, g['basis'], g['n_opers'][:1],
            g['n_coeffs'][:1], g['dt'], g['t'])
        ref = orc.control_matrix_from_scratch(g['eigvals'], g['eigvecs'], g['propagators'], omega,
                                              g['basis'], g['n_opers'][:1], g['n_coeffs'][:1],
                                              g['dt'], g['t'])
        assert R.shape == (1, 9, W) and rel_err(R, ref) < TIGHT
    # incomplete basis (n_basis < d^2) is allowed by the reference (pulse_sequence.py:303-306)
    R = numeric.calculate_control_matrix_from_scratch(
        g['eigvals'], g['eigvecs'], g['propagators'], g['omega'], g['basis'][2:7], g['n_opers'],
        g['n_coeffs'], g['dt'], g['t'])
    assert rel_err(R, g['control_matrix'][:, 2:7]) < TIGHT


def test_error_behaviour():
    g = load_golden('rand_d2_ggm')
    with pytest.raises(ValueError):
        numeric.calculate_filter_function(g['control_matrix'], which='bogus')
    with pytest.raises(ValueError):
        numeric.diagonalize(np.zeros((3, 65, 65), complex), np.ones(3))         # d > FFK_MAX_D
    with pytest.raises(ValueError):
        numeric.diagonalize(np.zeros((3, 2, 2), complex), np.ones(4))
    pulse = pulse_from(g)
    with pytest.raises(ValueError):
        ff.infidelity(pulse, np.ones((5, len(g['omega']))), g['omega'])          # bad spectrum shape
    with pytest.raises(ValueError):
        ff.infidelity(pulse, g['S1'], g['omega'], n_oper_identifiers=['nope'])
    with pytest.raises(ValueError):
        ff.infidelity(pulse, g['S1'], g['omega'], which='bogus')
    with pytest.raises(TypeError):
        ff.infidelity(pulse, g['S1'], g['omega'], test_convergence=True)


def test_convergence_and_smallness_wrappers():
    g = load_golden('rand_d2_ggm')
    pulse = pulse_from(g)
    n, infids = ff.infidelity(pulse, lambda w: 1e-3/w, dict(n_min=20, n_max=60, n_points=3),
                              test_convergence=True)
    assert list(n) == [20, 40, 60] and infids.shape == (3, len(g['n_opers']))
    w = np.linspace(*(2*np.pi/pulse.tau*np.array([1e-2, 1e2])), 60)
    ref = orc.infidelity_from_filter_function(
        orc.filter_function(orc.control_matrix_from_scratch(
            g['eigvals'], g['eigvecs'], g['propagators'], w, g['basis'], g['n_opers'],
            g['n_coeffs'], g['dt'], g['t'])), 1e-3/w, w, np.arange(len(g['n_opers'])), 2)
    assert rel_err(infids[-1], ref) < 1e-12
    omega = np.abs(g['omega']) + 0.1
    infid, xi = ff.infidelity(pulse, 1e-3/omega, np.sort(omega), return_smallness=True)
    assert infid.shape == (len(g['n_opers']),) and xi > 0


# ---- BASELINE config 2 at full size: d=4, 256 segments, 3 noise ops, 4096 omega ---------------
def config2_inputs(seed=42, d=4, G=256, A=3, W=4096, n_cops=3):
    rng = np.random.default_rng(seed)

    def herm_traceless(n):
        M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
        M = (M + M.conj().transpose(0, 2, 1))/2
        return M - np.trace(M, axis1=1, axis2=2)[:, None, None]*np.eye(d)/d
    c_opers, n_opers = herm_traceless(n_cops), herm_traceless(A)
    c_coeffs = rng.standard_normal((n_cops, G))
    n_coeffs = rng.random((A, G))
    dt = 1 - rng.random(G)
    omega = np.geomspace(1e-2/dt.sum(), 1e2/dt.min(), W)
    return c_opers, c_coeffs, n_opers, n_coeffs, dt, omega


def test_config2_full_size_against_oracle():
    c_opers, c_coeffs, n_opers, n_coeffs, dt, omega = config2_inputs()
    basis = ff.Basis.pauli(2)
    pulse = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt, basis)
    F = pulse.get_filter_function(omega)
    R = pulse.get_control_matrix(omega)
    S = 1e-3/omega
    infid = ff.infidelity(pulse, S, omega)
    # oracle (the reference's algorithm in NumPy) on the same inputs
    H = orc.hamiltonian(pulse.c_opers, pulse.c_coeffs)
    D, V, Q = orc.diagonalize(H, dt)
    R_ref = orc.control_matrix_from_scratch(D, V, Q, omega, np.asarray(basis), pulse.n_opers,
                                            pulse.n_coeffs, dt)
    F_ref = orc.filter_function(R_ref)
    infid_ref = orc.infidelity_from_filter_function(F_ref, S, omega, np.arange(3), 4)
    assert np.abs(pulse.eigvals - D).max() < 1e-13
    assert rel_err(pulse.propagators, Q) < 1e-12
    for a in range(3):                                       # per noise operator
        assert rel_err(R[a], R_ref[a]) < 1e-11
        assert rel_err(F[a], F_ref[a]) < 1e-11
    # elementwise relative check where the data are not negligible
    big = np.abs(R_ref) > 1e-6*np.abs(R_ref).max()
    assert np.max(np.abs(R - R_ref)[big]/np.abs(R_ref)[big]) < TOL
    assert rel_err(infid, infid_ref) < 1e-12
    # size-independent properties
    assert np.abs(R[:, 0]).max() < 1e-12*np.abs(R).max()      # identity column ~ 0 (traceless)
    B = numeric.calculate_noise_operators_from_scratch(pulse.eigvals, pulse.eigvecs,
                                                       pulse.propagators, omega, pulse.n_opers,
                                                       pulse.n_coeffs, dt)
    assert rel_err(orc.basis_expand(B, np.asarray(basis)).transpose(1, 2, 0), R) < 1e-13
    # linearity in the noise sensitivities: R(2 s) = 2 R(s)
    R2 = numeric.calculate_control_matrix_from_scratch(pulse.eigvals, pulse.eigvecs,
                                                       pulse.propagators, omega, basis,
                                                       pulse.n_opers, 2*pulse.n_coeffs, dt)
    assert rel_err(R2, 2*R) < 1e-14
    # basis independence of F (tests/test_basis.py:378-432)
    pulse_ggm = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt)
    assert rel_err(pulse_ggm.get_filter_function(omega), F) < 1e-12


# ---- NEXT-1: the concatenation rule --------------------------------------
def atomic_pulses(g, n=5):
    return [ff.PulseSequence.from_arrays(
        g[f'p{i}_c_opers'], g[f'p{i}_c_oper_identifiers'], g[f'p{i}_c_coeffs'], g[f'p{i}_n_opers'],
        g[f'p{i}_n_oper_identifiers'], g[f'p{i}_n_coeffs'], g[f'p{i}_dt'],
        ff.Basis(g[f'p{i}_basis'], btype='Pauli')) for i in range(n)]


def test_control_matrix_from_atomic():
    """numeric.calculate_control_matrix_from_atomic against the reference's outputs."""
    g = load_golden('from_atomic')
    R = numeric.calculate_control_matrix_from_atomic(g['phases'], g['R_atomic'],
                                                     g['propagators_liouville'])
    assert R.shape == g['R_total'].shape and rel_err(R, g['R_total']) < TIGHT
    Rc = numeric.calculate_control_matrix_from_atomic(g['phases'], g['R_atomic'],
                                                      g['propagators_liouville'],
                                                      which='correlations')
    assert Rc.shape == g['R_correlations'].shape and rel_err(Rc, g['R_correlations']) < TIGHT
    assert rel_err(Rc.sum(0), R) < TIGHT
    # complex Liouville propagators (non-Hermitian basis) take the other kernel branch
    Lc = g['propagators_liouville'].astype(complex)
    assert rel_err(numeric.calculate_control_matrix_from_atomic(g['phases'], g['R_atomic'], Lc),
                   g['R_total']) < TIGHT
    # a single pulse is returned as is
    R1 = numeric.calculate_control_matrix_from_atomic(g['phases'][:0], g['R_atomic'][:1],
                                                      g['propagators_liouville'][:0])
    assert np.array_equal(R1, g['R_atomic'][0])
    with pytest.raises(ValueError):
        numeric.calculate_control_matrix_from_atomic(g['phases'], g['R_atomic'],
                                                     g['propagators_liouville'], which='bogus')
    # long, thin case: the pulse axis is split into slabs (1000 single-segment gates, d = 2)
    rng = np.random.default_rng(3)
    G, A, N, W = 1000, 1, 4, 256
    Ra = rng.standard_normal((G, A, N, W)) + 1j*rng.standard_normal((G, A, N, W))
    ph = np.exp(1j*rng.standard_normal((G - 1, W)))
    L = rng.standard_normal((G - 1, N, N))
    got = numeric.calculate_control_matrix_from_atomic(ph, Ra, L)
    ref = orc.control_matrix_from_atomic(ph, Ra, L)
    assert rel_err(got, ref) < 1e-13
    # larger bases (d = 8 and 16: N = 64, 256), ragged omega
    for G, A, N, W in ((4, 2, 64, 70), (3, 1, 256, 33)):
        Ra = rng.standard_normal((G, A, N, W)) + 1j*rng.standard_normal((G, A, N, W))
        ph = np.exp(1j*rng.standard_normal((G - 1, W)))
        L = rng.standard_normal((G - 1, N, N))
        got = numeric.calculate_control_matrix_from_atomic(ph, Ra, L)
        assert rel_err(got, orc.control_matrix_from_atomic(ph, Ra, L)) < 1e-13
        gotc = numeric.calculate_control_matrix_from_atomic(ph, Ra, L, which='correlations')
        assert rel_err(gotc, orc.control_matrix_from_atomic(ph, Ra, L, 'correlations')) < 1e-13


def test_concatenate_matches_from_scratch_and_reference():
    """tests/test_core.py:724-743: concatenation rule == from-scratch evaluation of the long pulse."""
    g = load_golden('from_atomic')
    omega = g['omega']
    pulses = atomic_pulses(g)
    total = ff.concatenate(pulses, calc_filter_function=True, omega=omega)
    assert total.is_cached('control_matrix') and total.is_cached('filter_function')
    R = total.get_control_matrix(omega)
    assert rel_err(R, g['concat_control_matrix']) < 1e-12
    scratch = ff.concatenate_without_filter_function(atomic_pulses(g))
    assert rel_err(scratch.get_control_matrix(omega), R) < 1e-12
    assert rel_err(scratch.get_filter_function(omega), total.get_filter_function(omega)) < 1e-12
    assert np.allclose(total.total_propagator, scratch.total_propagator, atol=1e-13)
    # operator @, default decision logic: FF concatenated only if cached with equal omega
    a, b = atomic_pulses(g, 2)
    assert not (a @ b).is_cached('filter_function')
    a.cache_filter_function(omega)
    b.cache_filter_function(omega)
    ab = a @ b
    assert ab.is_cached('filter_function')
    ref = ff.concatenate_without_filter_function(atomic_pulses(g, 2)).get_filter_function(omega)
    assert rel_err(ab.get_filter_function(omega), ref) < 1e-12
    with pytest.raises(TypeError):
        a @ 3
    with pytest.raises(ValueError):
        b2 = atomic_pulses(g, 2)[1]
        b2.cache_filter_function(omega + 1)
        ff.concatenate([a, b2], calc_filter_function=True)


def test_pulse_correlation_filter_function():
    g = load_golden('from_atomic')
    omega = g['omega']
    pulses = atomic_pulses(g, 3)
    total = ff.concatenate(pulses, calc_pulse_correlation_FF=True, omega=omega)
    F_pc = total.get_pulse_correlation_filter_function()
    A = len(total.n_opers)
    assert F_pc.shape == (3, 3, A, A, len(omega))
    F = total.get_filter_function(omega)
    assert rel_err(F_pc.sum(axis=(0, 1)), F) < 1e-12
    ref = np.einsum('gako,hbko->ghabo', total.get_pulse_correlation_control_matrix().conj(),
                    total.get_pulse_correlation_control_matrix())
    assert rel_err(F_pc, ref) < 1e-13
    S = 1e-3/omega
    corr = ff.infidelity(total, S, omega, which='correlations')
    assert corr.shape == (3, 3, A)
    assert rel_err(corr.sum(axis=(0, 1)), ff.infidelity(total, S, omega)) < 1e-12


def test_spin_echo_concatenation_is_cpmg():
    """tests/test_sequencing.py:353-392: n concatenated spin echos == n-pulse CPMG (analytic)."""
    X, Z = util.paulis[1], util.paulis[3]
    n, tau, tau_pi = 6, np.pi, 1e-9
    t_se = tau/n
    dt = np.array([(t_se - tau_pi)/2, tau_pi, (t_se - tau_pi)/2])
    se = ff.PulseSequence([[X/2, [0, np.pi/tau_pi, 0]]], [[Z/2, [1, 1, 1]]], dt)
    omega = np.concatenate([-np.logspace(0, 3, 60)[::-1], np.logspace(0, 3, 60)])
    se.cache_filter_function(omega)
    cpmg = ff.concatenate([se]*n)
    assert cpmg.is_cached('filter_function')
    F = cpmg.get_filter_function(omega)[0, 0]
    z = omega*tau
    analytic = 8*np.sin(z/4/n)**4*np.sin(z/2)**2/np.cos(z/2/n)**2     # analytic.py CPMG, n even
    np.testing.assert_allclose((F*omega**2).real, analytic, atol=1e-9, rtol=1e-7)
    scratch = ff.concatenate_without_filter_function([se]*n).get_filter_function(omega)[0, 0]
    assert rel_err(F, scratch) < 1e-10


def test_randomized_benchmarking_sequence_via_table():
    """BASELINE config 3 in miniature (examples/randomized_benchmarking.py:95-151): a sequence
    drawn from a few distinct gates takes the gather-from-table kernel; it must agree with the
    plain concatenation rule on the materialised arrays and with the from-scratch evaluation."""
    X, Y = util.paulis[1], util.paulis[2]
    T = 20.0
    omega = 2*np.pi*np.geomspace(1e-2/(7*151*T), 1e2/T, 300)
    X2 = ff.PulseSequence([[X/2, [np.pi/2/T], 'X']], [[X/2, [1], 'X']], [T])
    Y2 = ff.PulseSequence([[Y/2, [np.pi/2/T], 'Y']], [[X/2, [1], 'X']], [T])
    for p in (X2, Y2):
        p.cache_control_matrix(omega)
    gates = [X2, Y2, X2 @ X2, Y2 @ X2, X2 @ Y2 @ Y2 @ Y2]
    assert all(gate.is_cached('control_matrix') for gate in gates)
    rng = np.random.default_rng(0)
    draw = rng.integers(0, len(gates), 120)
    seq = [gates[k] for k in draw]
    total = ff.concatenate(seq)                                   # repeated objects -> table path
    R = total.get_control_matrix(omega)
    # plain rule on the materialised (G, A, N, W) array
    phases = np.array([p.get_total_phases(omega) for p in seq[:-1]]).cumprod(axis=0)
    L = util.adot(np.array([p.total_propagator_liouville for p in seq[:-1]]))
    R_atomic = np.array([p.get_control_matrix(omega) for p in seq])
    R_plain = numeric.calculate_control_matrix_from_atomic(phases, R_atomic, L)
    assert rel_err(R, R_plain) < 1e-13
    assert rel_err(R, orc.control_matrix_from_atomic(phases, R_atomic, L)) < 1e-13
    scratch = ff.concatenate_without_filter_function(seq)
    assert len(scratch) == sum(len(p) for p in seq)
    assert rel_err(scratch.get_filter_function(omega), total.get_filter_function(omega)) < 1e-10
    # 'correlations' through the table path as well
    short = [gates[k] for k in draw[:7]]
    pc = ff.concatenate(short, calc_pulse_correlation_FF=True)
    assert rel_err(pc.get_pulse_correlation_control_matrix().sum(0),
                   ff.concatenate(short).get_control_matrix(omega)) < 1e-13


def test_logical_omega_shards_on_one_gpu():
    """the N-way omega sharding executed as N logical shards on one
    device equals the unsharded pass -- F blocks bit-identical, and the integral taken straight
    on the all-gather layout (n_shards, A, A, W/n) equals the one on (A, A, W)."""
    torch = pytest.importorskip('torch')
    from filter_functions_amd.device import DevicePipeline
    from filter_functions_amd.parallel import shard_bounds
    c_opers, c_coeffs, n_opers, n_coeffs, dt, omega = config2_inputs(G=32, W=1024)
    basis = ff.Basis.pauli(2)
    S = 1e-3/omega
    full = DevicePipeline(c_opers, c_coeffs, n_opers, n_coeffs, dt, basis, omega, spectrum=S)
    full.launch()
    torch.cuda.synchronize()
    F_full = full.filter_function.cpu().numpy()
    infid_full = full.infid.cpu().numpy()
    n = 4
    shards = torch.empty((n, 3, 3, 1024//n), dtype=torch.complex128, device='cuda')
    for r in range(n):
        w0, w1 = shard_bounds(1024, n, r)
        part = DevicePipeline(c_opers, c_coeffs, n_opers, n_coeffs, dt, basis, omega[w0:w1])
        part.launch()
        shards[r] = part.filter_function
        assert np.array_equal(part.filter_function.cpu().numpy(), F_full[:, :, w0:w1])
    dev = lambda a, ty: torch.from_numpy(np.ascontiguousarray(a, dtype=ty)).cuda()
    out = torch.empty(3, dtype=torch.float64, device='cuda')
    full.infidelity_from_shards(shards, dev(omega, float), dev(S, complex),
                                torch.arange(3, dtype=torch.int32, device='cuda'), out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), infid_full)
    ref = orc.infidelity_from_filter_function(F_full, S, omega, np.arange(3), 4)
    assert rel_err(infid_full, ref) < 1e-13


# ---- decay amplitudes -> cumulant function -> error transfer matrix --------------
def etm_pulse(g, name):
    basis = ff.Basis(g[f'{name}_basis'], btype=str(g[f'{name}_btype']))
    return ff.PulseSequence.from_arrays(
        g[f'{name}_c_opers'], g[f'{name}_c_oper_identifiers'], g[f'{name}_c_coeffs'],
        g[f'{name}_n_opers'], g[f'{name}_n_oper_identifiers'], g[f'{name}_n_coeffs'],
        g[f'{name}_dt'], basis)


@pytest.mark.parametrize('name', ['q1', 'q1id', 'p4', 'g3', 'g6'])
def test_error_transfer_matrix_against_reference(name):
    """Gamma, K and exp(K) through the PulseSequence API against the reference's outputs
    (cases of the reference's tests/test_precision.py:631-727)."""
    g = load_golden('etm')
    pulse = etm_pulse(g, name)
    omega = g[f'{name}_omega']
    assert rel_err(pulse.get_control_matrix(omega), g[f'{name}_control_matrix']) < TOL
    for i in (1, 2, 3):
        S = g[f'{name}_S{i}']
        gamma = numeric.calculate_decay_amplitudes(pulse, S, omega)
        ref = g[f'{name}_decay_amplitudes_S{i}']
        assert gamma.shape == ref.shape and gamma.dtype == np.float64
        assert rel_err(gamma, ref) < TOL
        K = numeric.calculate_cumulant_function(pulse, S, omega)
        assert rel_err(K, g[f'{name}_cumulant_function_S{i}']) < TOL
        # precomputed decay amplitudes: the contraction alone, tight
        K2 = numeric.calculate_cumulant_function(pulse, decay_amplitudes=ref)
        assert rel_err(K2, g[f'{name}_cumulant_function_S{i}']) < 1e-13
        U = ff.error_transfer_matrix(pulse, S, omega)
        U_ref = g[f'{name}_error_transfer_matrix_S{i}']
        assert np.abs(U - U_ref).max() < TOL*np.abs(U_ref - np.eye(len(U_ref))).max() + 1e-15
        assert np.allclose(ff.error_transfer_matrix(cumulant_function=K), U, rtol=0, atol=1e-15)
        assert np.allclose(ff.error_transfer_matrix(pulse, S, omega, memory_parsimonious=True), U)
        if f'{name}_infidelity_S{i}' in g:
            # entanglement infidelity from the cumulant function, reference test :671-676
            d = pulse.d
            assert np.allclose(-np.einsum('...ii', K)/d**2, g[f'{name}_infidelity_S{i}'],
                               rtol=1e-9, atol=1e-18)
    sub = numeric.calculate_decay_amplitudes(pulse, g[f'{name}_S1'], omega,
                                             n_oper_identifiers=pulse.n_oper_identifiers[1:])
    assert rel_err(sub, g[f'{name}_decay_amplitudes_S1_sub']) < TOL


def test_pulse_correlation_decay_amplitudes_and_cumulant():
    g = load_golden('etm')
    omega = g['pc_omega']
    pulses = [ff.PulseSequence.from_arrays(
        g[f'pc_p{i}_c_opers'], g[f'pc_p{i}_c_oper_identifiers'], g[f'pc_p{i}_c_coeffs'],
        g[f'pc_p{i}_n_opers'], g[f'pc_p{i}_n_oper_identifiers'], g[f'pc_p{i}_n_coeffs'],
        g[f'pc_p{i}_dt'], ff.Basis(g[f'pc_p{i}_basis'], btype='Pauli')) for i in range(3)]
    for q in pulses:
        q.cache_filter_function(omega)
    total = ff.concatenate(pulses, calc_pulse_correlation_FF=True, omega=omega)
    assert rel_err(total.get_pulse_correlation_control_matrix(), g['pc_control_matrix']) < TOL
    gamma = numeric.calculate_decay_amplitudes(total, g['pc_S2'], omega, which='correlations')
    assert gamma.shape == g['pc_decay_amplitudes'].shape
    assert rel_err(gamma, g['pc_decay_amplitudes']) < TOL
    K = numeric.calculate_cumulant_function(total, g['pc_S2'], omega, which='correlations')
    assert rel_err(K, g['pc_cumulant_function']) < TOL
    assert rel_err(K.sum(axis=(0, 1)), g['pc_cumulant_function_total']) < TOL
    with pytest.raises(ValueError):
        numeric.calculate_decay_amplitudes(total, g['pc_S2'], omega[:-1], which='correlations')


@pytest.mark.parametrize('A,N,W,s_ndim', [(3, 16, 4096, 2), (2, 25, 1000, 3), (2, 36, 777, 1),
                                           (1, 49, 130, 2), (2, 64, 2048, 3), (1, 4, 1, 1),
                                           (2, 9, 2, 2), (1, 256, 515, 1)])
def test_decay_amplitudes_gemm_against_oracle(A, N, W, s_ndim):
    """The frequency-axis GEMM on random control matrices: tile edges (N not a multiple of 16/32),
    frequency tails (W not a multiple of 16), split-K, all spectrum kinds, W = 1 and 2."""
    rng = np.random.default_rng(N*W)
    R = rng.standard_normal((A, N, W)) + 1j*rng.standard_normal((A, N, W))
    omega = np.sort(rng.random(W))*50 + 1e-3
    if s_ndim == 1:
        S = 1/(1 + omega**2)
    elif s_ndim == 2:
        S = rng.random((A, W))
    else:
        S = rng.standard_normal((A, A, W)) + 1j*rng.standard_normal((A, A, W))
        S = S + S.conj().swapaxes(0, 1)
    idx = np.arange(A)
    got = numeric._decay_amplitudes(R, S, omega, idx, 'total')
    ref = orc.decay_amplitudes(R, S, omega, idx)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-12*max(np.abs(ref).max(), 1e-300)


@pytest.mark.parametrize('d,btype', [(3, 'GGM'), (4, 'Pauli'), (5, 'GGM'), (8, 'Pauli'), (16, 'GGM'),
                                     (16, 'Pauli'), (12, 'GGM'), (3, 'dense'), (4, 'dense'), (8, 'dense')])
def test_cumulant_function_against_trace_free_oracle(d, btype):
    """The device contraction against the oracle's trace-free formulation (itself pinned against
    the reference's four-element-trace contraction for d <= 6), up to d = 16 where the N^4 trace
    tensor would need 68 GB.  GGM and Pauli bases take the sparse gathers, a dense (rotated)
    orthonormal Hermitian basis the dense products (decay.hip: the device decides)."""
    rng = np.random.default_rng(d)
    if btype == 'dense':
        # an orthogonal mixture of the GGM elements: orthonormal, Hermitian, traceless beyond the
        # identity, and every element dense
        ggm = np.asarray(ff.Basis.ggm(d))
        O = np.linalg.qr(rng.standard_normal((d*d - 1, d*d - 1)))[0]
        basis = ff.Basis(np.concatenate((ggm[:1], np.tensordot(O, ggm[1:], axes=1))))
        assert np.count_nonzero(np.abs(np.asarray(basis)[1:]) > 1e-14) > 0.9*(d*d - 1)*d*d
    else:
        basis = ff.Basis.ggm(d) if btype == 'GGM' else ff.Basis.pauli(int(np.log2(d)))
    N = d*d
    gamma = rng.standard_normal((2, 3, N, N))
    got = numeric._cumulant_function(gamma, basis)
    ref = orc.cumulant_function(gamma, np.asarray(basis))
    assert rel_err(got, ref) < 1e-12
    if d <= 5:
        assert rel_err(got, orc.cumulant_function_dense(gamma, np.asarray(basis))) < 1e-12


def test_cumulant_and_etm_error_behaviour():
    g = load_golden('etm')
    pulse = etm_pulse(g, 'p4')
    omega = g['p4_omega']
    with pytest.raises(ValueError):
        numeric.calculate_cumulant_function(pulse)
    with pytest.raises(ValueError):
        numeric.calculate_cumulant_function(pulse, g['p4_S1'], omega, which='correlations',
                                            second_order=True)
    with pytest.raises(ValueError):       # precomputed decay amplitudes of another shape
        numeric.calculate_cumulant_function(pulse, g['p4_S1'], omega, second_order=True,
                                            decay_amplitudes=np.ones((1, 16, 16)))
    with pytest.raises(ValueError):
        ff.error_transfer_matrix(pulse)
    with pytest.raises(TypeError):
        ff.error_transfer_matrix(cumulant_function=[[1.0]])
    with pytest.raises(ValueError):
        ff.error_transfer_matrix(cumulant_function=np.ones((3, 2)))
    with pytest.raises(ValueError):
        numeric.calculate_decay_amplitudes(pulse, np.ones((3, 5)), omega)
    with pytest.raises(ValueError):
        numeric.calculate_cumulant_function(pulse, decay_amplitudes=np.ones((3, 3)))


def test_decay_amplitudes_from_logical_omega_shards():
    """Device-resident path of the multi-GPU error-transfer-matrix run on one GPU: two frequency
    blocks, each integrated with the global trapezoid weights, add up to the unsharded result."""
    import torch
    from filter_functions_amd.device import DevicePipeline
    from filter_functions_amd.parallel import shard_bounds
    g = load_golden('etm')
    name = 'g6'
    omega, S = g[f'{name}_omega'], g[f'{name}_S3']
    args = (g[f'{name}_c_opers'], g[f'{name}_c_coeffs'], g[f'{name}_n_opers'],
            g[f'{name}_n_coeffs'], g[f'{name}_dt'], g[f'{name}_basis'])
    omega_dev = torch.from_numpy(omega).cuda()
    total = None
    for rank in range(2):
        w0, w1 = shard_bounds(len(omega), 2, rank)
        pipe = DevicePipeline(*args, omega[w0:w1], spectrum=S[..., w0:w1])
        pipe.launch(with_infidelity=False)
        part = pipe.decay_amplitudes(omega_global=omega_dev, w_offset=w0)
        total = part if total is None else total + part
    ref = g[f'{name}_decay_amplitudes_S3']
    assert rel_err(total.cpu().numpy(), ref) < TOL
    K = pipe.cumulant_function(total).cpu().numpy()
    assert rel_err(K, g[f'{name}_cumulant_function_S3']) < TOL
    whole = DevicePipeline(*args, omega, spectrum=S)
    whole.launch(with_infidelity=False)
    assert rel_err(whole.decay_amplitudes().cpu().numpy(), ref) < TOL


def test_noise_operator_step_cache():
    """cache_intermediates products of calculate_noise_operators_from_scratch
    (reference numeric.py:586-615)."""
    g = load_golden('noise_operator_steps')
    B, inter = numeric.calculate_noise_operators_from_scratch(
        g['eigvals'], g['eigvecs'], g['propagators'], g['omega'], g['n_opers'], g['n_coeffs'],
        g['dt'], g['t'], cache_intermediates=True)
    assert rel_err(B, g['noise_operators']) < TOL
    assert sorted(inter) == ['first_order_integral', 'n_opers_transformed', 'noise_operators_step',
                             'phase_factors']
    for key in ('first_order_integral', 'phase_factors', 'noise_operators_step'):
        assert inter[key].shape == g[f'inter_{key}'].shape
        assert rel_err(inter[key], g[f'inter_{key}']) < TOL
    # the eigenvectors are inputs here, so the transformed operators are comparable directly
    assert rel_err(inter['n_opers_transformed'], g['inter_n_opers_transformed']) < TOL
    assert rel_err(inter['noise_operators_step'].sum(axis=0), B) < 1e-13


@pytest.mark.parametrize('d,G,A,W', [(4, 9, 3, 100), (4, 20, 5, 47), (8, 7, 3, 100), (12, 5, 5, 33), (16, 6, 2, 16), (16, 3, 9, 50),
                                      (8, 20, 1, 257), (16, 4, 6, 35), (12, 4, 1, 20), (12, 3, 3, 17),
                                      (16, 2, 7, 19), (12, 6, 10, 64), (16, 3, 8, 9), (16, 2, 17, 21), (12, 3, 19, 40),
                                      (16, 2, 11, 5), (12, 2, 8, 8)])
def test_matrix_core_accumulate_kernel_matches_vector_kernel(d, G, A, W):
    """ctrl_mfma.hip (matrix cores; d = 12, 16: one frequency per 4 x 4 x 4 block) against ctrl.hip
    on the same inputs: ragged frequency tiles (W not a multiple of 16), operator counts that do not
    fill a block -- with and without the separate launch for the one or two operators left over
    from blocks of four --, d = 12, several segment chunks."""
    rng = np.random.default_rng(d*1000 + W)
    basis = ff.Basis.ggm(d)
    c_opers = rng.standard_normal((3, d, d)) + 1j*rng.standard_normal((3, d, d))
    c_opers = c_opers + c_opers.conj().transpose(0, 2, 1)
    n_opers = rng.standard_normal((A, d, d)) + 1j*rng.standard_normal((A, d, d))
    n_opers = n_opers + n_opers.conj().transpose(0, 2, 1)
    H = np.einsum('ijk,il->ljk', c_opers, rng.standard_normal((3, G)))
    dt = 0.5 + rng.random(G)
    n_coeffs = rng.random((A, G)) + 0.5
    omega = np.concatenate(([0.0], np.geomspace(1e-3, 50, W - 1)))
    D, V, Q = numeric.diagonalize(H, dt)
    lib = _lib.load()
    try:
        _lib.check(lib.ffk_set_accumulate_variant(3))
        R_vec = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers,
                                                              n_coeffs, dt)
        _lib.check(lib.ffk_set_accumulate_variant(4))
        R_mat = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers,
                                                              n_coeffs, dt)
        assert _lib.stats()['grid_x'] == (W + 15)//16      # the matrix-core kernel ran
        for chunks in (2, 3):
            _lib.check(lib.ffk_set_segment_chunks(chunks))
            R_c = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers,
                                                                n_coeffs, dt)
            assert rel_err(R_c, R_mat) < 1e-13
    finally:
        _lib.check(lib.ffk_set_segment_chunks(0))
        _lib.check(lib.ffk_set_accumulate_variant(0))
    assert rel_err(R_mat, R_vec) < 1e-12
    if d >= 12 and W <= 50:
        # step cache through the matrix-core kernel (one segment per block)
        R_i, inter = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers,
                                                                   n_coeffs, dt,
                                                                   cache_intermediates=True)
        assert rel_err(inter['control_matrix_step'].sum(axis=0), R_mat) < 1e-12
        assert rel_err(R_i, R_mat) < 1e-13
    t = np.concatenate(([0], dt.cumsum()))
    R_orc = orc.control_matrix_from_scratch(D, V, Q, omega, np.asarray(basis), n_opers, n_coeffs,
                                            dt, t)
    assert rel_err(R_mat, R_orc) < TOL


@pytest.mark.parametrize('A,N,W', [(5, 9, 100), (7, 16, 257), (13, 4, 64), (18, 25, 130)])
def test_filter_function_many_noise_operators(A, N, W):
    """Blocked F kernel (A > 4): against the oracle, exactly Hermitian in the operator indices,
    bit-identical to the pairwise kernel's summation order (checked through a 4-operator slice)."""
    rng = np.random.default_rng(A*W)
    R = rng.standard_normal((A, N, W)) + 1j*rng.standard_normal((A, N, W))
    F = numeric.calculate_filter_function(R)
    assert F.shape == (A, A, W)
    assert rel_err(F, orc.filter_function(R)) < 1e-14
    assert np.array_equal(F, F.conj().transpose(1, 0, 2))
    assert np.all(F[np.arange(A), np.arange(A)].imag == 0)
    sub = numeric.calculate_filter_function(R[:4])            # pairwise kernel
    assert np.array_equal(sub, F[:4, :4])


@pytest.mark.parametrize('name', ['d2', 'd3'])
def test_infidelity_nontraceless_basis(name):
    """infidelity() with a basis that is not traceless (reference numeric.py:2295-2305)."""
    g = load_golden('nontraceless')
    basis = ff.Basis(g[f'{name}_basis'])
    assert not basis.istraceless and basis.btype == 'Custom'
    pulse = ff.PulseSequence.from_arrays(
        g[f'{name}_c_opers'], g[f'{name}_c_oper_identifiers'], g[f'{name}_c_coeffs'],
        g[f'{name}_n_opers'], g[f'{name}_n_oper_identifiers'], g[f'{name}_n_coeffs'],
        g[f'{name}_dt'], basis)
    omega = g[f'{name}_omega']
    assert rel_err(pulse.get_control_matrix(omega), g[f'{name}_control_matrix']) < TOL
    for i in (1, 2, 3):
        infid = ff.infidelity(pulse, g[f'{name}_S{i}'], omega)
        assert infid.shape == g[f'{name}_infidelity_S{i}'].shape
        assert rel_err(infid, g[f'{name}_infidelity_S{i}']) < TOL


@pytest.mark.parametrize('name', ['d2', 'd3', 'd5'])
def test_noise_operators_from_atomic(name):
    """numeric.calculate_noise_operators_from_atomic against the reference's output; the phases
    array carries one row more than needed, like in the reference's own test."""
    g = load_golden('noise_operators_from_atomic')
    B = numeric.calculate_noise_operators_from_atomic(g[f'{name}_phases'], g[f'{name}_B_atomic'],
                                                      g[f'{name}_propagators'])
    assert B.shape == g[f'{name}_B'].shape and rel_err(B, g[f'{name}_B']) < TIGHT
    one = numeric.calculate_noise_operators_from_atomic(g[f'{name}_phases'][:0],
                                                        g[f'{name}_B_atomic'][:1],
                                                        g[f'{name}_propagators'][:0])
    assert np.array_equal(one, g[f'{name}_B_atomic'][0])
    with pytest.raises(ValueError):
        numeric.calculate_noise_operators_from_atomic(g[f'{name}_phases'][:1],
                                                      g[f'{name}_B_atomic'],
                                                      g[f'{name}_propagators'])
    # d = 16: one operator per wavefront with 4 elements per lane
    rng = np.random.default_rng(0)
    Ba = rng.standard_normal((3, 5, 2, 16, 16)) + 1j*rng.standard_normal((3, 5, 2, 16, 16))
    ph = np.exp(1j*rng.standard_normal((2, 5)))
    P = np.linalg.qr(rng.standard_normal((2, 16, 16)) + 1j*rng.standard_normal((2, 16, 16)))[0]
    got = numeric.calculate_noise_operators_from_atomic(ph, Ba, P)
    assert rel_err(got, orc.noise_operators_from_atomic(ph, Ba, P)) < 1e-13


def test_propagator_at_arbitrary_times():
    g = load_golden('rand_d3_ggm')
    pulse = pulse_from(g)
    Q = pulse.propagator_at_arb_t(pulse.t)
    assert rel_err(Q, pulse.propagators) < 1e-13
    # inside a segment: Q(t) = exp(-i H_l (t - t_l)) Q_l, checked through the group property
    t_mid = pulse.t[:-1] + 0.3*pulse.dt
    Qm = pulse.propagator_at_arb_t(t_mid)
    H = np.einsum('ijk,il->ljk', pulse.c_opers, pulse.c_coeffs)
    w, V = np.linalg.eigh(H)
    step = (V*np.exp(-1j*w*0.3*pulse.dt[:, None])[:, None, :]) @ V.conj().transpose(0, 2, 1)
    assert rel_err(Qm, step @ pulse.propagators[:-1]) < 1e-12


def test_singlet_triplet_cnot_against_monte_carlo():
    """The reference's CNOT test (tests/test_precision.py:274-311): d = 6 subspace of four
    exchange-coupled spins, 250 steps, a partial 15-element Pauli basis of the computational
    subspace, dimension overridden to 4; infidelities within 10 % of the Monte Carlo results and
    equal to the reference's own numbers."""
    g = load_golden('cnot')
    ident = [str(s) for s in g['identifiers']]
    basis = ff.Basis(g['basis'], btype='Pauli')
    assert basis.shape == (15, 6, 6) and not basis.iscomplete
    cnot = ff.PulseSequence(list(zip(g['c_opers'], g['c_coeffs'], ident)),
                            list(zip(g['c_opers'], g['n_coeffs'], ident)), g['dt'], basis=basis)
    cnot.d = 4
    omega = g['omega']
    assert rel_err(cnot.get_filter_function(omega), g['filter_function']) < TOL
    for i in (0, 1):
        infid, xi = ff.infidelity(cnot, g[f'S{i}'], omega, ident[:3], return_smallness=True)
        assert rel_err(infid, g[f'infid{i}']) < TOL
        assert abs(xi - g[f'xi{i}']) <= 1e-12*abs(g[f'xi{i}'])
        assert abs(1 - infid.sum()/g['infid_monte_carlo'][i]) <= 0.10
        assert infid.sum() <= xi**2/4


def test_filter_function_is_basis_independent():
    """Reference tests/test_basis.py:378-432: the fidelity filter function does not depend on the
    (complete, orthonormal) operator basis; the identity column of the control matrix vanishes
    iff the noise operators are traceless."""
    rng = np.random.default_rng(11)
    d, G, A = 4, 6, 2
    def herm(n, traceless=True):
        M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
        M = M + M.conj().transpose(0, 2, 1)
        if traceless:
            M -= np.trace(M, axis1=1, axis2=2)[:, None, None]*np.eye(d)/d
        return M
    c_opers, c_coeffs = herm(2), rng.standard_normal((2, G))
    n_coeffs, dt = rng.random((A, G)) + 0.5, rng.random(G) + 0.5
    omega = np.geomspace(1e-2, 1e2, 77)
    # a third basis: a random orthogonal rotation of the GGM elements (complete, not traceless)
    ggm = np.asarray(ff.Basis.ggm(d))
    Qr = np.linalg.qr(rng.standard_normal((d*d, d*d)))[0]
    rotated = ff.Basis(np.einsum('kl,lij->kij', Qr, ggm))
    for traceless in (True, False):
        n_opers = herm(A, traceless)
        results = []
        for basis in (ff.Basis.pauli(2), ff.Basis.ggm(d), rotated):
            pulse = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)),
                                     dt, basis)
            R = pulse.get_control_matrix(omega)
            results.append(pulse.get_filter_function(omega))
            if basis is not rotated:
                zero = np.abs(R[:, 0]).max() < 1e-13*np.abs(R).max()
                assert zero == traceless
        assert rel_err(results[1], results[0]) < 1e-12
        assert rel_err(results[2], results[0]) < 1e-12


@pytest.mark.parametrize('seed', range(12))
def test_randomised_shapes_against_oracle(seed):
    """Sweep of random problem shapes (every Hilbert-space dimension 2..16, few to many segments,
    1-5 noise operators, ragged frequency counts incl. W = 1) through the PulseSequence API against
    the oracle: control matrix, filter function, infidelity, noise operators."""
    rng = np.random.default_rng(1000 + seed)
    for _ in range(4):
        d = int(rng.integers(2, 17))
        G = int(rng.integers(1, 24))
        A = int(rng.integers(1, 6))
        W = int(rng.choice([1, 2, 17, 63, 64, 65, 130]))
        n_cops = int(rng.integers(1, 4))
        def herm(n):
            M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
            return M + M.conj().transpose(0, 2, 1)
        c_opers, n_opers = herm(n_cops), herm(A)
        c_coeffs = rng.standard_normal((n_cops, G))
        n_coeffs = rng.random((A, G)) + 0.1
        dt = rng.random(G) + 0.2
        omega = np.sort(rng.random(W))*20 - 2.0
        basis = ff.Basis.ggm(d)
        pulse = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt, basis)
        R = pulse.get_control_matrix(omega)
        F = pulse.get_filter_function(omega)
        H = orc.hamiltonian(pulse.c_opers, pulse.c_coeffs)
        D, V, Q = orc.diagonalize(H, dt)
        R_ref = orc.control_matrix_from_scratch(D, V, Q, omega, np.asarray(basis), pulse.n_opers,
                                                pulse.n_coeffs, dt)
        tag = f'd={d} G={G} A={A} W={W}'
        assert rel_err(R, R_ref) < TOL, tag
        assert rel_err(F, orc.filter_function(R_ref)) < TOL, tag
        B = numeric.calculate_noise_operators_from_scratch(pulse.eigvals, pulse.eigvecs,
                                                           pulse.propagators, omega, pulse.n_opers,
                                                           pulse.n_coeffs, dt, pulse.t)
        B_ref = orc.noise_operators_from_scratch(D, V, Q, omega, pulse.n_opers, pulse.n_coeffs, dt)
        assert rel_err(B, B_ref) < TOL, tag
        if W > 1:
            S = 1/(1 + omega**2)
            infid = ff.infidelity(pulse, S, omega)
            ref = orc.infidelity_from_filter_function(orc.filter_function(R_ref), S, omega,
                                                      np.arange(A), d)
            assert np.abs(infid - ref).max() <= TOL*np.abs(ref).max(), tag


@pytest.mark.parametrize('seed', range(6))
def test_device_pipeline_random_shapes(seed):
    """The fused device pipeline (ffk_pipeline_dev: compaction inside the prologue launch, chunk sum
    + expansion + F in one launch where A d^2 <= 256, separate kernels otherwise) over random
    shapes against the oracle."""
    import torch
    from filter_functions_amd.device import DevicePipeline
    rng = np.random.default_rng(500 + seed)
    for _ in range(3):
        d = int(rng.choice([2, 3, 4, 5, 6, 8, 12, 16]))
        G = int(rng.integers(1, 40))
        A = int(rng.integers(1, 6))
        W = int(rng.choice([2, 16, 63, 200, 1000]))
        def herm(n):
            M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
            return M + M.conj().transpose(0, 2, 1)
        c_opers, n_opers = herm(2), herm(A)
        c_coeffs, n_coeffs = rng.standard_normal((2, G)), rng.random((A, G)) + 0.1
        dt = rng.random(G) + 0.2
        omega = np.sort(rng.random(W))*30 + 1e-3
        basis = ff.Basis.ggm(d) if rng.random() < 0.5 or d not in (2, 4, 8, 16) else \
            ff.Basis.pauli(int(np.log2(d)))
        S = rng.random((A, W)) + 0.1
        pipe = DevicePipeline(c_opers, c_coeffs, n_opers, n_coeffs, dt, basis, omega, spectrum=S)
        pipe.launch()
        torch.cuda.synchronize()
        H = orc.hamiltonian(c_opers, c_coeffs)
        D, V, Q = orc.diagonalize(H, dt)
        R_ref = orc.control_matrix_from_scratch(D, V, Q, omega, np.asarray(basis), n_opers, n_coeffs, dt)
        F_ref = orc.filter_function(R_ref)
        tag = f'd={d} G={G} A={A} W={W} {basis.btype}'
        assert rel_err(pipe.control_matrix.cpu().numpy(), R_ref) < TOL, tag
        F = pipe.filter_function.cpu().numpy()
        assert rel_err(F, F_ref) < TOL, tag
        assert np.array_equal(F, F.conj().transpose(1, 0, 2)), tag
        ref = orc.infidelity_from_filter_function(F_ref, S, omega, np.arange(A), d)
        assert np.abs(pipe.infid.cpu().numpy() - ref).max() <= TOL*np.abs(ref).max(), tag


@pytest.mark.parametrize('d,A,btype', [(16, 1, 'ggm'), (16, 2, 'pauli'), (16, 5, 'ggm'), (16, 6, 'pauli'), (16, 9, 'ggm'),
                                       (12, 1, 'ggm'), (12, 3, 'ggm'), (12, 6, 'ggm')])
def test_expansion_in_the_accumulate_kernels_epilogue(d, A, btype):
    """With ONE segment chunk the d = 12 / 16 matrix-core kernel holds the complete Y of its tile and
    expands it in the basis itself (ctrl_mfma.hip: ExpandEpilogue), writing R instead of Y: 1 / 2 / left-over
    operator blocks, sparse (GGM) and dense (Pauli) bases, a frequency count that leaves the last tile
    partly empty -- must equal the separate expansion of the same Y (array entry point on the
    pipeline's own eigensystem, same single chunk) to the last bit, and the oracle within tolerance."""
    import torch
    from filter_functions_amd import _lib
    from filter_functions_amd.device import DevicePipeline
    rng = np.random.default_rng(100*d + A)
    G, W = 7, 41

    def herm(n):
        M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
        return M + M.conj().transpose(0, 2, 1)
    c_opers, n_opers = herm(2), herm(A)
    c_coeffs, n_coeffs = rng.standard_normal((2, G)), rng.random((A, G)) + 0.1
    dt = rng.random(G) + 0.2
    omega = np.sort(rng.random(W))*30 + 1e-3
    basis = ff.Basis.ggm(d) if btype == 'ggm' else ff.Basis.pauli(int(np.log2(d)))
    lib = _lib.load()
    try:
        _lib.check(lib.ffk_set_segment_chunks(1))
        pipe = DevicePipeline(c_opers, c_coeffs, n_opers, n_coeffs, dt, basis, omega)
        pipe.launch()
        torch.cuda.synchronize()
        R = pipe.control_matrix.cpu().numpy()
        D, V, Q = (t.cpu().numpy() for t in (pipe.eigvals, pipe.eigvecs, pipe.propagators))
        t = np.concatenate(([0.0], dt.cumsum()))
        R_two_launches = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs,
                                                                       dt, t)
    finally:
        _lib.check(lib.ffk_set_segment_chunks(0))
    assert np.array_equal(R, R_two_launches)
    R_ref = orc.control_matrix_from_scratch(D, V, Q, omega, np.asarray(basis), n_opers, n_coeffs, dt)
    assert rel_err(R, R_ref) < TOL
    F = pipe.filter_function.cpu().numpy()
    assert rel_err(F, orc.filter_function(R_ref)) < TOL


@pytest.mark.parametrize('N,scale', [(36, 1e-4), (64, 0.3), (100, 5.0), (256, 1e-3), (256, 40.0), (33, 0.0), (4, 0.5),
                                     (9, 3.0), (16, 1e-3), (1, 2.0)])
def test_matrix_exponential_against_scipy(N, scale):
    """ffk_expm_real (scaling and squaring, Taylor degree 18, MFMA products) against
    scipy.linalg.expm, which the reference's error_transfer_matrix calls (numeric.py:2051)."""
    import ctypes
    from scipy.linalg import expm
    rng = np.random.default_rng(N)
    K = rng.standard_normal((N, N))*scale/np.sqrt(N)
    K = K - 0.5*np.abs(K).sum(axis=0).max()*np.eye(N)*(scale > 1)      # decaying, like a cumulant
    out = np.empty_like(K)
    _lib.check(_lib.load().ffk_expm_real(K.ctypes.data_as(ctypes.c_void_p), N,
                                         out.ctypes.data_as(ctypes.c_void_p)))
    ref = expm(K)
    assert np.abs(out - ref).max() <= 1e-12*max(np.abs(ref).max(), 1.0)
    # the public function takes the same route
    U = ff.error_transfer_matrix(cumulant_function=K[None])
    assert np.array_equal(U, out)


@pytest.mark.parametrize('case', ['real 2-D', 'real 1-D', 'complex 2-D', 'shard of a larger grid'])
def test_decay_amplitudes_symmetric_block_kernel(case):
    """N = 256 (d = 16, full basis), one pulse with itself, enough (operator, 128-frequency chunk) pairs to fill the
    chip: decay_gemm_sym256_kernel (the operator's rows through LDS once, ten tiles on eight wavefronts) computes the
    integral of numeric.py:1194-1337; a ragged frequency count, an operator subset out of order; complex weights make
    it stand down for the general kernel inside the same call."""
    import ctypes
    import torch
    lib = _lib.load()
    A, N, n_idx = 6, 256, 4
    W = 8192 + 5
    rng = np.random.default_rng(7)
    R = rng.standard_normal((A, N, W)) + 1j*rng.standard_normal((A, N, W))
    omega_all = np.sort(rng.uniform(0.0, 50.0, W + 300))
    idx = np.array([5, 0, 3, 1], dtype=np.int32)
    w_offset = 0
    omega = omega_all[:W]
    if case == 'real 1-D':
        S = rng.uniform(-0.5, 1.0, W)
    else:
        S = rng.uniform(-0.5, 1.0, (n_idx, W))
    if case == 'complex 2-D':
        S = S + 1j*rng.standard_normal((n_idx, W))
    if case == 'shard of a larger grid':
        omega, w_offset = omega_all, 120
    ref = orc.decay_amplitudes_shard(R, S, omega, w_offset, idx)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Rd, Sd, od, idxd = dev(R), dev(S.astype(complex)), dev(omega), dev(idx)
    out = torch.full((n_idx, N, N), float('nan'), dtype=torch.float64, device='cuda')
    need = lib.ffk_decay_amplitudes_workspace_bytes(1, N, W, n_idx, S.ndim)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    if case == 'shard of a larger grid':
        _lib.check(lib.ffk_decay_amplitudes_shard_dev(p(Rd), 1, A, N, W, p(Sd), S.ndim, p(od), len(omega), w_offset,
                                                      p(idxd), n_idx, p(out), p(ws), need, None))
    else:
        _lib.check(lib.ffk_decay_amplitudes_dev(p(Rd), 1, A, N, W, p(Sd), S.ndim, p(od), p(idxd), n_idx, p(out),
                                                p(ws), need, None))
    gamma = out.cpu().numpy()
    assert rel_err(gamma, ref) < 1e-12
    if case != 'complex 2-D':
        # the 64 x 64 tiles below the diagonal are mirrored, not recomputed
        assert np.array_equal(gamma[:, 64:, :64], gamma[:, :64, 64:].swapaxes(-1, -2))
        assert np.array_equal(gamma[:, 192:, 128:192], gamma[:, 128:192, 192:].swapaxes(-1, -2))


@pytest.mark.parametrize('N,batch,scale', [(36, 1, 1e-4), (64, 3, 0.3), (100, 2, 5.0), (256, 18, 1e-3),
                                           (256, 2, 40.0), (33, 1, 0.0), (16, 4, 0.2)])
def test_device_error_transfer_matrix_against_scipy(N, batch, scale):
    """ffk_error_transfer_matrix_dev (sum over the leading axis, 1-norm, scaling and squaring, all in HBM) against
    scipy.linalg.expm of the NumPy sum (numeric.py:2049-2053), and bit-identical to the host-boundary call."""
    import ctypes
    import torch
    from scipy.linalg import expm
    from filter_functions_amd.device import DevicePipeline
    rng = np.random.default_rng(N + batch)
    K = rng.standard_normal((batch, N, N))*scale/np.sqrt(N)/batch
    K = K - 0.5*np.abs(K.sum(0)).sum(axis=0).max()*np.eye(N)*(scale > 1)/batch
    lib = _lib.load()
    Kd = torch.from_numpy(K).cuda()
    out = torch.empty((N, N), dtype=torch.float64, device='cuda')
    need = lib.ffk_error_transfer_matrix_workspace_bytes(N)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.ffk_error_transfer_matrix_dev(p(Kd), batch, N, p(out), p(ws), need, ctypes.c_void_p(stream)))
    ref = expm(K.sum(axis=0))
    U = out.cpu().numpy()
    assert np.abs(U - ref).max() <= 1e-12*max(np.abs(ref).max(), 1.0)
    host = np.empty((N, N))
    total = np.ascontiguousarray(K.sum(axis=0))
    _lib.check(lib.ffk_expm_real(total.ctypes.data_as(ctypes.c_void_p), N, host.ctypes.data_as(ctypes.c_void_p)))
    assert np.array_equal(U, host)
    # the wrapper on the pipeline object (any leading axes) is the same call
    assert np.array_equal(DevicePipeline.error_transfer_matrix(_EtmOnly(torch), Kd[None]).cpu().numpy(), U)
    # errors: a workspace that is too small, NaN in the input
    assert lib.ffk_error_transfer_matrix_dev(p(Kd), batch, N, p(out), p(ws), need - 1, ctypes.c_void_p(stream)) \
        == _lib.FFK_EINVAL
    Kd[0, 0, 0] = float('nan')
    assert lib.ffk_error_transfer_matrix_dev(p(Kd), batch, N, p(out), p(ws), need, ctypes.c_void_p(stream)) \
        == _lib.FFK_EINVAL


class _EtmOnly:
    """the attributes DevicePipeline.error_transfer_matrix uses"""

    def __init__(self, torch):
        import ctypes
        self.torch = torch
        self.device = torch.device('cuda', torch.cuda.current_device())
        self._p = lambda t: ctypes.c_void_p(t.data_ptr())


def test_sharded_error_transfer_matrix_single_rank():
    """parallel.sharded_error_transfer_matrix on a one-rank gloo group (the collective path with
    world size 1 is the identity): same result as the host API."""
    import torch
    import torch.distributed as dist
    from filter_functions_amd.device import DevicePipeline
    from filter_functions_amd.parallel import sharded_error_transfer_matrix
    g = load_golden('etm')
    name = 'g6'
    omega, S = g[f'{name}_omega'], g[f'{name}_S2']
    pipe = DevicePipeline(g[f'{name}_c_opers'], g[f'{name}_c_coeffs'], g[f'{name}_n_opers'],
                          g[f'{name}_n_coeffs'], g[f'{name}_dt'], g[f'{name}_basis'], omega,
                          spectrum=S)
    pipe.launch(with_infidelity=False)
    created = False
    if not dist.is_initialized():
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:29533', rank=0, world_size=1)
        created = True
    try:
        gamma, K, U = sharded_error_transfer_matrix(pipe, torch.from_numpy(omega).cuda(), 0)
    finally:
        if created:
            dist.destroy_process_group()
    assert rel_err(gamma.cpu().numpy(), g[f'{name}_decay_amplitudes_S2']) < TOL
    assert rel_err(K.cpu().numpy(), g[f'{name}_cumulant_function_S2']) < TOL
    U_ref = g[f'{name}_error_transfer_matrix_S2']
    assert np.abs(U - U_ref).max() < TOL*np.abs(U_ref - np.eye(len(U_ref))).max() + 1e-15


def test_cache_cleanup_semantics():
    """cleanup() modes, nbytes and the caches filled by concatenate, as the reference's
    tests/test_core.py:386-455 walks through them."""
    X, Y = util.paulis[1], util.paulis[2]
    A = ff.PulseSequence([[X, [1]]], [[Y, [2]]], [3])
    A.diagonalize()
    for _ in range(3):
        A.cleanup('conservative')
        assert A.eigvals is not None and A.eigvecs is not None and A.propagators is not None
    A.cleanup('all')
    a = A.nbytes
    A.diagonalize()
    b = A.nbytes
    A.cache_control_matrix([1])
    c = A.nbytes
    A.cleanup('frequency dependent')
    A.cache_control_matrix([1], cache_intermediates=True)
    d = A.nbytes
    assert a != b and b != c and c != d
    A.cleanup('all')
    omega = util.get_sample_frequencies(A)
    C = ff.concatenate((A, A), calc_pulse_correlation_FF=True, which='generalized', omega=omega)
    C.diagonalize()
    attrs = ['eigvals', 'eigvecs', 'propagators']
    assert all(C.is_cached(x) for x in attrs)
    C.cleanup()
    assert not any(C.is_cached(x) for x in attrs)
    C.diagonalize()
    C.cache_control_matrix(A.omega)
    attrs += ['control_matrix', 'total_phases', 'total_propagator', 'total_propagator_liouville']
    assert all(C.is_cached(x) for x in attrs)
    C.cleanup('greedy')
    assert not any(C.is_cached(x) for x in attrs)
    C.cache_filter_function(A.omega, which='generalized')
    assert all(C.is_cached(x) for x in attrs + ['omega', 'filter_function_gen',
                                                 'filter_function_pc_gen'])
    C = ff.concatenate((A, A), calc_pulse_correlation_FF=True, which='fidelity', omega=A.omega)
    C.diagonalize()
    C.cache_filter_function(A.omega, which='fidelity')
    attrs += ['omega', 'filter_function', 'filter_function_pc']
    assert all(C.is_cached(x) for x in attrs)
    C.cleanup('all')
    assert not any(C.is_cached(x) for x in attrs + ['filter_function_gen', 'filter_function_pc_gen'])
    C.cache_filter_function(A.omega, which='fidelity')
    C.cleanup('frequency dependent')
    freq = {'omega', 'control_matrix', 'filter_function', 'filter_function_gen',
            'filter_function_pc', 'filter_function_pc_gen', 'total_phases'}
    assert not any(C.is_cached(x) for x in freq)
    assert all(C.is_cached(x) for x in set(attrs) - freq)


@pytest.mark.parametrize('d,n_dt', [(2, 40), (5, 25), (7, 12)])
def test_filter_function_scratch_vs_atomic_and_getters(d, n_dt):
    """The reference's tests/test_core.py:685-782: the control matrix from scratch equals the
    one assembled from single-segment pulses by the concatenation rule (atol 1e-13), autocorrelation
    filter functions are real, F_fidelity is the trace of F_generalized, also after the cached
    frequencies change."""
    rng = np.random.default_rng(d*n_dt)
    def herm(n):
        M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
        M = M + M.conj().transpose(0, 2, 1)
        return M - np.trace(M, axis1=1, axis2=2)[:, None, None]*np.eye(d)/d
    c_opers, n_opers = herm(4), herm(6)
    c_coeffs, n_coeffs = rng.standard_normal((4, n_dt)), rng.random((6, n_dt))
    dt = 1 - rng.random(n_dt)
    total = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt)
    omega = util.get_sample_frequencies(total, n_samples=100)
    R = total.get_control_matrix(omega, show_progressbar=True)
    assert all(total.is_cached(x) for x in ('total_phases', 'total_propagator',
                                            'total_propagator_liouville'))
    pulses = [ff.PulseSequence(list(zip(total.c_opers, total.c_coeffs[:, i:i + 1])),
                               list(zip(total.n_opers, total.n_coeffs[:, i:i + 1])), dt[i:i + 1])
              for i in range(n_dt)]
    phases = np.exp(1j*total.t[1:, None]*omega)
    L = ff.liouville_representation(total.propagators[1:], total.basis)
    R_g = np.array([p.get_control_matrix(omega) for p in pulses])
    R_atomic = numeric.calculate_control_matrix_from_atomic(phases, R_g, L)
    D, V, _ = numeric.diagonalize(np.einsum('il,ijk->ljk', total.c_coeffs, total.c_opers), dt)
    R_scratch = numeric.calculate_control_matrix_from_scratch(
        eigvals=D, eigvecs=V, propagators=total.propagators, omega=omega, basis=total.basis,
        n_opers=total.n_opers, n_coeffs=total.n_coeffs, dt=dt)
    assert np.allclose(R, R_scratch, rtol=1e-7, atol=1e-13)
    assert np.allclose(R_scratch, R_atomic, rtol=1e-7, atol=1e-13)
    F = total.get_filter_function(omega)
    assert np.isreal(F[np.eye(6, dtype=bool)]).all()
    for shift in (0, 0, 1):
        Fg = total.get_filter_function(omega + shift, which='generalized')
        Ff = total.get_filter_function(omega + shift, which='fidelity')
        assert np.allclose(Ff, Fg.trace(axis1=2, axis2=3), rtol=1e-7, atol=1e-13)


# ---- second order: F2 -> frequency shifts -> cumulant function / error transfer matrix ----------
@pytest.mark.slow
@pytest.mark.parametrize('name', ['q1', 'g3', 'p4', 'p4idle'])
def test_second_order_chain_against_reference(name):
    """Second-order filter function (incl. negative and zero frequencies, an idle segment with fully
    degenerate eigenvalues), frequency shifts for 1-D/2-D/3-D spectra, second-order cumulant
    function and error transfer matrix against the reference's outputs (cases of the reference's
    tests/test_core.py:784-800, 1005-1066, tests/test_precision.py:631-727)."""
    g = load_golden('second_order')
    pulse = etm_pulse(g, name)
    omega = g[f'{name}_omega']
    F2 = pulse.get_filter_function(omega, order=2)
    ref = g[f'{name}_filter_function_2']
    assert F2.shape == ref.shape and F2.dtype == np.complex128 and F2.flags.c_contiguous
    assert rel_err(F2, ref) < TOL
    assert pulse.get_filter_function(omega, order=2) is F2           # memoised by reference
    assert pulse.is_cached('filter_function_2')
    # from the reference's own eigensystem, through the free function: tight
    F2_free = numeric.calculate_second_order_filter_function_from_scratch(
        g[f'{name}_eigvals'], g[f'{name}_eigvecs'], g[f'{name}_propagators'], omega, pulse.basis,
        pulse.n_opers, pulse.n_coeffs, pulse.dt)
    assert rel_err(F2_free, ref) < 1e-12
    for i in (1, 2, 3):
        S = g[f'{name}_S{i}']
        delta = numeric.calculate_frequency_shifts(pulse, S, omega)
        d_ref = g[f'{name}_frequency_shifts_S{i}']
        assert delta.shape == d_ref.shape and delta.dtype == np.float64
        assert rel_err(delta, d_ref) < TOL
        K = numeric.calculate_cumulant_function(pulse, S, omega, second_order=True)
        K_ref = g[f'{name}_cumulant_function_2_S{i}']
        assert rel_err(K, K_ref) < TOL
        gamma = numeric.calculate_decay_amplitudes(pulse, S, omega)
        K_pre = numeric.calculate_cumulant_function(pulse, decay_amplitudes=gamma,
                                                    frequency_shifts=d_ref, second_order=True)
        assert rel_err(K_pre, K_ref) < TOL
        U = ff.error_transfer_matrix(pulse, S, omega, second_order=True)
        U_ref = g[f'{name}_error_transfer_matrix_2_S{i}']
        assert np.abs(U - U_ref).max() < TOL*np.abs(U_ref - np.eye(len(U_ref))).max() + 1e-15
    sub = numeric.calculate_frequency_shifts(pulse, g[f'{name}_S1'], omega,
                                             n_oper_identifiers=pulse.n_oper_identifiers[1:])
    assert rel_err(sub, g[f'{name}_frequency_shifts_S1'][1:]) < TOL
    # a pulse without a cached F2 takes the fused device pass, which also fills the cache
    fresh = etm_pulse(g, name)
    for i in (3, 1):
        delta = numeric.calculate_frequency_shifts(fresh, g[f'{name}_S{i}'], omega)
        assert rel_err(delta, g[f'{name}_frequency_shifts_S{i}']) < TOL
        assert fresh.is_cached('filter_function_2')
        assert rel_err(fresh.get_filter_function(omega, order=2), ref) < TOL
    sub = numeric.calculate_frequency_shifts(etm_pulse(g, name), g[f'{name}_S2'][1:], omega,
                                             n_oper_identifiers=pulse.n_oper_identifiers[1:])
    assert rel_err(sub, g[f'{name}_frequency_shifts_S2'][1:]) < TOL


@pytest.mark.slow
@pytest.mark.parametrize('seed', range(6))
def test_second_order_filter_function_random_shapes(seed):
    """Random shapes against the oracle: output tiles of every register-tile size (A N from 4 to
    > 64, i.e. several tiles per axis), odd frequency counts on both sides of the two-frequencies-
    per-block switch, grids containing w = 0 and negative frequencies."""
    rng = np.random.default_rng(7000 + seed)
    shapes = [(2, 1, 5, 601), (2, 3, 3, 37), (3, 2, 4, 64), (4, 3, 6, 33), (5, 3, 2, 9),
              (3, 5, 3, 513), (6, 2, 2, 5), (4, 1, 7, 1), (9, 1, 2, 3), (8, 2, 2, 6)]
    for d, A, G, W in shapes[seed % 2::2] if seed < 4 else shapes[seed - 4::3]:
        def herm(n):
            M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
            return M + M.conj().transpose(0, 2, 1)
        n_cops = int(rng.integers(1, 3))
        c_opers, n_opers = herm(n_cops), herm(A)
        c_coeffs = rng.standard_normal((n_cops, G))
        n_coeffs = rng.random((A, G)) + 0.1
        dt = rng.random(G) + 0.2
        omega = np.sort(rng.random(W))*12 - 3.0
        if W > 2:
            omega[W//3] = 0.0
        pulse = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt,
                                 ff.Basis.ggm(d))
        F2 = pulse.get_filter_function(omega, order=2)
        H = orc.hamiltonian(pulse.c_opers, pulse.c_coeffs)
        D, V, Q = orc.diagonalize(H, dt)
        ref = orc.second_order_filter_function(D, V, Q, omega, np.asarray(pulse.basis),
                                               pulse.n_opers, pulse.n_coeffs, dt)
        tag = f'd={d} A={A} G={G} W={W}'
        assert rel_err(F2, ref) < TOL, tag
        if W > 1:
            S = np.tile(1/(1 + omega**2), (A, A, 1)).astype(complex)
            delta = numeric.calculate_frequency_shifts(pulse, S, omega)
            assert rel_err(delta, orc.frequency_shifts(ref, S, omega, np.arange(A))) < TOL, tag
            K1 = numeric.calculate_cumulant_function(pulse, S, omega)
            K2 = numeric.calculate_cumulant_function(pulse, S, omega, second_order=True)
            contrib = K2 - K1
            assert np.abs(contrib - orc.cumulant_second_order(delta, np.asarray(pulse.basis))).max() \
                < 1e-12*max(np.abs(delta).max(), 1e-300), tag
            # the frequency-shift terms generate a rotation: antisymmetric (reference
            # tests/test_core.py:1057-1063)
            assert np.abs(contrib + contrib.swapaxes(-1, -2)).max() < 1e-14*np.abs(delta).max(), tag


@pytest.mark.slow
def test_second_order_matrix_core_kernel_matches_vector_kernel(monkeypatch):
    """The MFMA kernel (default where its operands fit in LDS) against the register-tiled vector
    kernel on the same inputs; both are compared with the oracle elsewhere."""
    rng = np.random.default_rng(99)
    for d, A, G, W in [(4, 3, 9, 130), (2, 1, 4, 7), (3, 4, 5, 33), (5, 2, 3, 18), (8, 1, 2, 9)]:
        def herm(n):
            M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
            return M + M.conj().transpose(0, 2, 1)
        c_opers, n_opers = herm(2), herm(A)
        dt = rng.random(G) + 0.2
        omega = np.sort(rng.random(W))*12 - 3.0
        omega[W//2] = 0.0
        pulse = ff.PulseSequence(list(zip(c_opers, rng.standard_normal((2, G)))),
                                 list(zip(n_opers, rng.random((A, G)) + 0.1)), dt, ff.Basis.ggm(d))
        pulse.diagonalize()
        args = (pulse.eigvals, pulse.eigvecs, pulse.propagators, omega, pulse.basis, pulse.n_opers,
                pulse.n_coeffs, pulse.dt)
        monkeypatch.setenv('FFK_TUNE_SO_MFMA', '1')
        F_mfma = numeric.calculate_second_order_filter_function_from_scratch(*args)
        monkeypatch.setenv('FFK_TUNE_SO_MFMA', '0')
        F_vec = numeric.calculate_second_order_filter_function_from_scratch(*args)
        monkeypatch.delenv('FFK_TUNE_SO_MFMA')
        assert rel_err(F_mfma, F_vec) < 1e-12, f'd={d} A={A} G={G} W={W}'


@pytest.mark.slow
def test_second_order_free_induction_decay_closed_form():
    """Reference tests/test_precision.py:218-270: an idle qubit under white and quasistatic noise.
    F2 of the single segment is known in closed form, splitting the segment changes nothing, and
    the frequency shift is sigma^2 tau/2 (white) resp. sigma^2 tau^2/2 (quasistatic)."""
    rng = np.random.default_rng(11)
    for ix in (1, 2, 3):
        tau = float(rng.random()) + 0.1
        sigma = float(rng.random()) + 0.1
        X = util.paulis[1]/np.sqrt(2)
        B = util.paulis[ix]/np.sqrt(2)
        piecewise = ff.PulseSequence([[X, np.zeros(21)]], [[B, np.ones(21)]], [tau/21]*21)
        single = ff.PulseSequence([[X, np.zeros(1)]], [[B, np.ones(1)]], [tau])
        omega = util.get_sample_frequencies(piecewise, 501, include_quasistatic=False)
        omega = np.concatenate([-omega[::-1], [0], omega])
        spect = np.full_like(omega, sigma**2)
        d_pw = numeric.calculate_frequency_shifts(piecewise, spect, omega)
        d_1 = numeric.calculate_frequency_shifts(single, spect, omega)
        F2 = single.get_filter_function(omega, order=2)
        mask = np.zeros_like(d_1, dtype=bool)
        mask[0, ix, ix] = True
        assert np.abs(d_1 - d_pw).max() < 1e-12
        assert np.allclose(d_1[mask], sigma**2*tau/2, rtol=1e-3)
        assert np.abs(d_1[~mask]).max() < 1e-12
        w = omega[502:]
        closed = (util.cexpm1(-w*tau)/(1j*w) + tau)/(1j*w)
        assert rel_err(F2[0, 0, ix, ix, 502:], closed) < TOL
        assert rel_err(F2[0, 0, ix, ix, 501], tau**2/2) < 1e-14
        assert np.abs(util.integrate(F2.imag, omega)).max() < 1e-12
        # quasistatic limit: only the w == 0 entry carries weight
        omega = np.array([-1e-15, 0, 1e-15])/tau
        spect = 2*np.pi*sigma**2*np.array([0, 1/omega[-1], 0])
        d_pw = numeric.calculate_frequency_shifts(piecewise, spect, omega)
        d_1 = numeric.calculate_frequency_shifts(single, spect, omega)
        assert np.abs(d_1 - d_pw).max() < 1e-12
        assert np.allclose(d_1[mask], sigma**2*tau**2/2, rtol=1e-10)
        assert np.abs(d_1[~mask]).max() < 1e-12


@pytest.mark.slow
def test_second_order_error_behaviour():
    """Argument errors of the reference (tests/test_core.py:1019-1046)."""
    g = load_golden('second_order')
    pulse = etm_pulse(g, 'q1')
    omega, S = g['q1_omega'], g['q1_S1']
    gamma = numeric.calculate_decay_amplitudes(pulse, S, omega)
    with pytest.raises(ValueError):
        numeric.calculate_cumulant_function(pulse, None, None, frequency_shifts=None,
                                            second_order=True)
    with pytest.raises(ValueError):
        numeric.calculate_cumulant_function(pulse, S, omega, second_order=True, which='correlations')
    with pytest.raises(ValueError):
        numeric.calculate_cumulant_function(pulse, S, omega, second_order=True,
                                            decay_amplitudes=gamma[1:])
    with pytest.warns(UserWarning):
        numeric.calculate_cumulant_function(pulse, S, omega, second_order=True,
                                            memory_parsimonious=True)
    with pytest.raises(ValueError):
        pulse.get_filter_function(omega, order=3)
    with pytest.raises(ValueError):
        numeric.calculate_frequency_shifts(pulse, S[:-1], omega)


@pytest.mark.slow
def test_second_order_config2_size_against_oracle_subsample():
    """BASELINE config-2 shape (d=4, 256 segments, 3 noise operators, 4096 frequencies; F2 is 151 MB).
    Every frequency is independent, so the oracle on a 16-frequency subsample pins the full-size
    run; the frequency shifts are compared through the oracle's integration of the device F2 and
    through the antisymmetry of their cumulant contribution."""
    c_opers, c_coeffs, n_opers, n_coeffs, dt, omega = config2_inputs()
    pulse = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt,
                             ff.Basis.pauli(2))
    basis = np.asarray(pulse.basis)
    F2 = pulse.get_filter_function(omega, order=2)
    assert F2.shape == (3, 3, 16, 16, 4096)
    sel = np.linspace(0, len(omega) - 1, 16).astype(int)
    H = orc.hamiltonian(pulse.c_opers, pulse.c_coeffs)
    D, V, Q = orc.diagonalize(H, dt)
    ref = orc.second_order_filter_function(D, V, Q, omega[sel], basis, pulse.n_opers,
                                           pulse.n_coeffs, dt)
    assert rel_err(F2[..., sel], ref) < TOL
    S = 1e-3/omega
    delta = numeric.calculate_frequency_shifts(pulse, S, omega)
    assert rel_err(delta, orc.frequency_shifts(F2, S, omega, np.arange(3))) < 1e-12
    K1 = numeric.calculate_cumulant_function(pulse, S, omega)
    K2 = numeric.calculate_cumulant_function(pulse, S, omega, second_order=True)
    contrib = K2 - K1
    assert np.abs(contrib).max() > 0
    assert np.abs(contrib + contrib.swapaxes(-1, -2)).max() < 1e-13*np.abs(delta).max()


@pytest.mark.slow
@pytest.mark.parametrize('name', ['q1', 'p4', 'p4idle'])
def test_device_resident_second_order_with_logical_omega_shards(name):
    """The multi-GPU second-order path on one GPU: F2 and the frequency shifts stay in HBM
    (DevicePipeline, ``*_dev`` entries); two frequency blocks integrated with the global trapezoid
    weights add up to the reference's frequency shifts, and the sharded error transfer matrix with
    second_order=True reproduces the reference's."""
    import torch
    import torch.distributed as dist
    from filter_functions_amd.device import DevicePipeline
    from filter_functions_amd.parallel import shard_bounds, sharded_error_transfer_matrix
    g = load_golden('second_order')
    omega = g[f'{name}_omega']
    om_dev = torch.from_numpy(omega).cuda()
    for i in (1, 2, 3):
        S = g[f'{name}_S{i}']
        total = None
        for rank in range(2):
            w0, w1 = shard_bounds(len(omega), 2, rank)
            pipe = DevicePipeline(g[f'{name}_c_opers'], g[f'{name}_c_coeffs'], g[f'{name}_n_opers'],
                                  g[f'{name}_n_coeffs'], g[f'{name}_dt'], g[f'{name}_basis'],
                                  omega[w0:w1], spectrum=S[..., w0:w1])
            pipe.launch(with_infidelity=False)
            F2 = pipe.second_order_filter_function()
            assert rel_err(F2.cpu().numpy(), g[f'{name}_filter_function_2'][..., w0:w1]) < TOL
            part = pipe.frequency_shifts(omega_global=om_dev, w_offset=w0)
            total = part if total is None else total + part
        assert rel_err(total.cpu().numpy(), g[f'{name}_frequency_shifts_S{i}']) < TOL
    S = g[f'{name}_S2']
    pipe = DevicePipeline(g[f'{name}_c_opers'], g[f'{name}_c_coeffs'], g[f'{name}_n_opers'],
                          g[f'{name}_n_coeffs'], g[f'{name}_dt'], g[f'{name}_basis'], omega, spectrum=S)
    pipe.launch(with_infidelity=False)
    created = False
    if not dist.is_initialized():
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:29534', rank=0, world_size=1)
        created = True
    try:
        gamma, K, U = sharded_error_transfer_matrix(pipe, om_dev, 0, single_qubit=(name == 'q1'),
                                                    second_order=True)
    finally:
        if created:
            dist.destroy_process_group()
    assert rel_err(K.cpu().numpy(), g[f'{name}_cumulant_function_2_S2']) < TOL
    U_ref = g[f'{name}_error_transfer_matrix_2_S2']
    assert np.abs(U - U_ref).max() < TOL*np.abs(U_ref - np.eye(len(U_ref))).max() + 1e-15


@pytest.mark.slow
@pytest.mark.parametrize('name', ['q1', 'g3', 'p4'])
def test_second_order_concatenation(name):
    """concatenate(calc_second_order_FF=True) against the reference's result and against the
    from-scratch second-order filter function of the long sequence (reference
    tests/test_sequencing.py:471-505); the free function against the oracle's rule."""
    g = load_golden('second_order_concat')
    omega = g[f'{name}_omega']

    def pulses():
        out = []
        for i in range(3):
            basis = ff.Basis(g[f'{name}_p{i}_basis'], btype=str(g[f'{name}_p{i}_btype']))
            out.append(ff.PulseSequence.from_arrays(
                g[f'{name}_p{i}_c_opers'], g[f'{name}_p{i}_c_oper_identifiers'],
                g[f'{name}_p{i}_c_coeffs'], g[f'{name}_p{i}_n_opers'],
                g[f'{name}_p{i}_n_oper_identifiers'], g[f'{name}_p{i}_n_coeffs'],
                g[f'{name}_p{i}_dt'], basis))
        return out
    ref = g[f'{name}_filter_function_2']
    F2 = numeric.calculate_second_order_filter_function_from_atomic(
        g[f'{name}_filter_function_2_atomic'], g[f'{name}_control_matrix_pc'],
        g[f'{name}_propagators_liouville'])
    assert rel_err(F2, ref) < 1e-12
    seq = pulses()
    total = ff.concatenate(seq, calc_second_order_FF=True, omega=omega)
    assert total.is_cached('filter_function_2') and total.is_cached('filter_function')
    assert not total.is_cached('control_matrix_pc')
    assert rel_err(total.get_filter_function(omega, order=2), ref) < TOL
    assert rel_err(total.get_filter_function(omega), g[f'{name}_filter_function']) < TOL
    # every pulse now holds its own F2 (computed on the way)
    assert all(p.is_cached('filter_function_2') for p in seq)
    both = ff.concatenate(pulses(), calc_second_order_FF=True, calc_pulse_correlation_FF=True,
                          omega=omega)
    assert rel_err(both.get_filter_function(omega, order=2), ref) < TOL
    assert rel_err(both.get_pulse_correlation_control_matrix(), g[f'{name}_control_matrix_pc']) < TOL
    # from scratch on the long sequence
    long = ff.concatenate_without_filter_function(pulses())
    assert rel_err(long.get_filter_function(omega, order=2), ref) < TOL
    # a repeated pulse object: its F2 is computed once and reused
    p0, p1 = pulses()[:2]
    rep = ff.concatenate([p0, p1, p0], calc_second_order_FF=True, omega=omega)
    plain = ff.concatenate_without_filter_function([p0, p1, p0])
    assert rel_err(rep.get_filter_function(omega, order=2),
                   plain.get_filter_function(omega, order=2)) < TOL
    # differing noise operators: warning, first order only (reference pulse_sequence.py:1773-1776)
    rng = np.random.default_rng(3)
    d = p0.d
    M = rng.standard_normal((4, d, d)) + 1j*rng.standard_normal((4, d, d))
    M = M + M.conj().transpose(0, 2, 1)
    one = ff.PulseSequence([[M[0], [0.3, -0.2]]], [[M[1], [1.0, 1.0], 'n_a']], [1.0, 0.5], p0.basis)
    other = ff.PulseSequence([[M[0], [0.7]]], [[M[2], [1.0], 'n_b']], [0.8], p0.basis)
    p0 = one
    with pytest.warns(UserWarning):
        mixed = ff.concatenate([p0, other], calc_second_order_FF=True, omega=omega)
    assert not mixed.is_cached('filter_function_2')


# ---- gradient: derivative of the filter function / infidelity by the control amplitudes ----------
@pytest.mark.slow
@pytest.mark.parametrize('name', ['q1', 'g3', 'p4'])
def test_filter_function_and_infidelity_derivative_against_reference(name):
    """get_filter_function_derivative / gradient.infidelity_derivative against the reference's
    outputs (gradient.py; cases of the reference's tests/test_gradient.py:70-176): all controls and
    noise operators, subsets selected by identifiers, with and without n_coeffs_deriv."""
    g = load_golden('gradient')
    pulse = etm_pulse(g, name)
    omega = g[f'{name}_omega']
    dF = pulse.get_filter_function_derivative(omega)
    ref = g[f'{name}_filter_function_derivative']
    assert dF.shape == ref.shape and dF.dtype == np.float64
    assert rel_err(dF, ref) < TOL
    ncd = g[f'{name}_n_coeffs_deriv']
    assert rel_err(pulse.get_filter_function_derivative(omega, n_coeffs_deriv=ncd),
                   g[f'{name}_filter_function_derivative_ncd']) < TOL
    for i in (1, 2):
        S = g[f'{name}_S{i}']
        assert rel_err(gradient.infidelity_derivative(pulse, S, omega),
                       g[f'{name}_infidelity_derivative_S{i}']) < TOL
        assert rel_err(gradient.infidelity_derivative(pulse, S, omega, n_coeffs_deriv=ncd),
                       g[f'{name}_infidelity_derivative_ncd_S{i}']) < TOL
    c_sub = pulse.c_oper_identifiers[g[f'{name}_sub_c_idx']]
    n_sub = pulse.n_oper_identifiers[g[f'{name}_sub_n_idx']]
    sub = pulse.get_filter_function_derivative(omega, control_identifiers=c_sub,
                                               n_oper_identifiers=n_sub)
    assert rel_err(sub, g[f'{name}_filter_function_derivative_sub']) < TOL
    with pytest.raises(ValueError):
        pulse.get_filter_function_derivative(omega, n_coeffs_deriv=ncd[:, :1])


@pytest.mark.slow
@pytest.mark.parametrize('seed', range(4))
def test_gradient_random_shapes_against_oracle_and_finite_differences(seed):
    """Random shapes (d = 2..8, idle segments with degenerate spectra, w = 0 and negative
    frequencies) against the oracle; and the analytic infidelity gradient against central finite
    differences of the device infidelity (reference tests/test_gradient.py:158-176)."""
    rng = np.random.default_rng(4200 + seed)
    for _ in range(3):
        d = int(rng.integers(2, 9))
        G = int(rng.integers(1, 7))
        A, H = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        W = int(rng.choice([1, 9, 64, 70]))

        def herm(n):
            M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
            return M + M.conj().transpose(0, 2, 1)
        c_opers, n_opers = herm(H), herm(A)
        c_coeffs = rng.standard_normal((H, G))
        if G > 2:
            c_coeffs[:, 1] = 0.0                                   # idle segment
        n_coeffs = rng.random((A, G)) + 0.1
        dt = rng.random(G) + 0.2
        omega = np.sort(rng.random(W))*10 - 2.0
        if W > 2:
            omega[W//2] = 0.0
        pulse = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt,
                                 ff.Basis.ggm(d))
        dF = pulse.get_filter_function_derivative(omega)
        Hm = orc.hamiltonian(pulse.c_opers, pulse.c_coeffs)
        D, V, Q = orc.diagonalize(Hm, dt)
        ref = orc.filter_function_derivative(D, V, Q, omega, np.asarray(pulse.basis), pulse.n_opers,
                                             pulse.n_coeffs, pulse.c_opers, dt)
        tag = f'd={d} G={G} A={A} H={H} W={W}'
        assert rel_err(dF, ref) < TOL, tag
    # finite differences of the infidelity
    d, G = 3, 4
    c_opers, n_opers = herm(2)[:, :d, :d], herm(2)[:, :d, :d]
    c_opers = (c_opers + c_opers.conj().transpose(0, 2, 1))/2
    n_opers = (n_opers + n_opers.conj().transpose(0, 2, 1))/2
    c_coeffs = rng.standard_normal((2, G))
    n_coeffs = rng.random((2, G)) + 0.5
    dt = rng.random(G) + 0.3
    omega = np.geomspace(1e-2, 30, 200)
    S = 1e-2/omega

    def infid(cc):
        p = ff.PulseSequence(list(zip(c_opers, cc)), list(zip(n_opers, n_coeffs)), dt, ff.Basis.ggm(d))
        return ff.infidelity(p, S, omega)
    pulse = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt,
                             ff.Basis.ggm(d))
    grad = gradient.infidelity_derivative(pulse, S, omega)            # (A, G, H)
    eps = 1e-6
    order = np.argsort(np.argsort(pulse.c_oper_identifiers))
    for s in range(G):
        for h in range(2):
            cp, cm = c_coeffs.copy(), c_coeffs.copy()
            cp[h, s] += eps
            cm[h, s] -= eps
            fd = (infid(cp) - infid(cm))/(2*eps)
            assert np.allclose(grad[:, s, order[h]], fd, rtol=1e-5, atol=1e-9), (s, h)


@pytest.mark.slow
@pytest.mark.parametrize('name', ['q1', 'g3', 'p4', 'g5'])
def test_control_matrix_derivative_against_reference(name):
    """gradient.calculate_derivative_of_control_matrix_from_scratch and
    calculate_filter_function_derivative against the reference's outputs (gradient.py:384-556),
    with and without n_coeffs_deriv; consistency with get_filter_function_derivative."""
    g = load_golden('gradient_ctrlmat')
    omega, dt = g[f'{name}_omega'], g[f'{name}_dt']
    t = np.concatenate(([0.0], dt.cumsum()))
    args = (omega, g[f'{name}_propagators'], g[f'{name}_eigvals'], g[f'{name}_eigvecs'],
            g[f'{name}_basis'], t, dt, g[f'{name}_n_opers'], g[f'{name}_n_coeffs'],
            g[f'{name}_c_opers'])
    R = g[f'{name}_control_matrix']
    for tag, ncd in (('', None), ('_ncd', g[f'{name}_n_coeffs_deriv'])):
        dR = gradient.calculate_derivative_of_control_matrix_from_scratch(*args, ncd)
        ref = g[f'{name}_control_matrix_derivative{tag}']
        assert dR.shape == ref.shape and dR.dtype == np.complex128
        assert rel_err(dR, ref) < TOL
        dF = gradient.calculate_filter_function_derivative(R, dR)
        assert dF.dtype == np.float64
        assert rel_err(dF, g[f'{name}_filter_function_derivative{tag}']) < TOL
        assert rel_err(gradient.calculate_filter_function_derivative(R, ref),
                       g[f'{name}_filter_function_derivative{tag}']) < TOL
    pulse = etm_pulse(g, name)
    assert rel_err(pulse.get_filter_function_derivative(omega),
                   g[f'{name}_filter_function_derivative']) < TOL
    with pytest.raises(ValueError):
        gradient.calculate_derivative_of_control_matrix_from_scratch(
            *args, g[f'{name}_n_coeffs_deriv'][:, :1])
    with pytest.raises(ValueError):
        gradient.calculate_filter_function_derivative(R[:, :-1], ref)


@pytest.mark.slow
@pytest.mark.parametrize('seed', range(3))
def test_control_matrix_derivative_random_shapes_against_oracle(seed):
    """Random shapes (d = 2..8, an idle segment, w = 0 and negative frequencies, W not a multiple
    of the wavefront) against the oracle, and a finite-difference check of the control matrix."""
    rng = np.random.default_rng(5200 + seed)
    for _ in range(3):
        d = int(rng.integers(2, 9))
        G = int(rng.integers(1, 6))
        A, H = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        W = int(rng.choice([1, 9, 64, 70]))

        def herm(n):
            M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
            return M + M.conj().transpose(0, 2, 1)
        c_opers, n_opers = herm(H), herm(A)
        c_coeffs = rng.standard_normal((H, G))
        if G > 2:
            c_coeffs[:, 1] = 0.0
        n_coeffs = rng.random((A, G)) + 0.1
        dt = rng.random(G) + 0.2
        omega = np.sort(rng.random(W))*10 - 2.0
        if W > 2:
            omega[W//2] = 0.0
        basis = np.asarray(ff.Basis.ggm(d))
        Hm = orc.hamiltonian(c_opers, c_coeffs)
        D, V, Q = orc.diagonalize(Hm, dt)
        ncd = rng.standard_normal((A, H, G)) if rng.random() < 0.5 else None
        t = np.concatenate(([0.0], dt.cumsum()))
        dR = gradient.calculate_derivative_of_control_matrix_from_scratch(
            omega, Q, D, V, basis, t, dt, n_opers, n_coeffs, c_opers, ncd)
        ref = orc.control_matrix_derivative(D, V, Q, omega, basis, n_opers, n_coeffs, c_opers, dt,
                                            ncd)
        tag = f'd={d} G={G} A={A} H={H} W={W}'
        assert rel_err(dR, ref) < TOL, tag
        R = orc.control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
        assert rel_err(gradient.calculate_filter_function_derivative(R, dR),
                       orc.filter_function_derivative_from_control_matrix(R, ref)) < TOL, tag
    # central finite differences of the device control matrix
    d, G, H, A = 3, 3, 2, 2
    c_opers, n_opers = herm(H)[:, :d, :d], herm(A)[:, :d, :d]
    c_opers = (c_opers + c_opers.conj().transpose(0, 2, 1))/2
    n_opers = (n_opers + n_opers.conj().transpose(0, 2, 1))/2
    c_coeffs, n_coeffs = rng.standard_normal((H, G)), rng.random((A, G)) + 0.5
    dt = rng.random(G) + 0.3
    omega = np.linspace(-2, 8, 11)
    basis = ff.Basis.ggm(d)

    def ctrlmat(cc):
        Dm, Vm, Qm = numeric.diagonalize(np.einsum('hij,hg->gij', c_opers, cc), dt)
        return numeric.calculate_control_matrix_from_scratch(Dm, Vm, Qm, omega, basis, n_opers,
                                                             n_coeffs, dt), (Dm, Vm, Qm)
    _, (D, V, Q) = ctrlmat(c_coeffs)
    dR = gradient.calculate_derivative_of_control_matrix_from_scratch(
        omega, Q, D, V, basis, None, dt, n_opers, n_coeffs, c_opers)
    eps = 1e-6
    for s in range(G):
        for h in range(H):
            cp, cm = c_coeffs.copy(), c_coeffs.copy()
            cp[h, s] += eps
            cm[h, s] -= eps
            fd = (ctrlmat(cp)[0] - ctrlmat(cm)[0])/(2*eps)           # (A, N, W)
            # rounding noise of the difference quotient: ~eps_machine*|R|/eps
            atol = 1e-7*max(1.0, np.abs(fd).max())
            assert np.allclose(dR[h, :, s].transpose(1, 2, 0), fd, rtol=1e-5, atol=atol), (s, h)


@pytest.mark.slow
@pytest.mark.parametrize('name', ['q1', 'g3', 'p4'])
def test_concatenate_periodic(name):
    """concatenate_periodic against the reference's closed-form result (pulse_sequence.py:1890-1973)
    and against the from-scratch control matrix of the tiled pulse."""
    g = load_golden('periodic')
    omega = g[f'{name}_omega']
    pulse = etm_pulse(g, name)
    assert not ff.concatenate_periodic(pulse, 3).is_cached('control_matrix')     # nothing cached yet
    pulse.cache_filter_function(omega)
    for reps in (1, 2, 9):
        per = ff.concatenate_periodic(pulse, reps)
        assert len(per) == reps*len(pulse) and np.isclose(per.tau, reps*pulse.tau)
        assert rel_err(per.get_control_matrix(omega), g[f'{name}_control_matrix_x{reps}']) < TOL
        assert rel_err(per.get_filter_function(omega), g[f'{name}_filter_function_x{reps}']) < TOL
        assert rel_err(per.total_propagator, g[f'{name}_total_propagator_x{reps}']) < TOL
        scratch = ff.concatenate_without_filter_function([pulse]*reps)
        assert rel_err(per.get_control_matrix(omega), scratch.get_control_matrix(omega)) < TOL
    with pytest.raises(TypeError):
        ff.concatenate_periodic('pulse', 2)


@pytest.mark.slow
@pytest.mark.parametrize('repeats', [1001, 10000])
def test_concatenate_periodic_many_repeats(repeats):
    """Thousands of periods (the reference's periodic_driving example repeats a 20-segment period
    10 000 times): against the closed form of the oracle, and -- for 1001 -- against the same pulse
    object concatenated 1001 times, a position count the pulse-axis slabs of the concatenation
    kernel do not divide."""
    g = load_golden('periodic')
    omega = g['q1_omega']
    pulse = etm_pulse(g, 'q1')
    pulse.cache_filter_function(omega)
    per = ff.concatenate_periodic(pulse, repeats)
    want = orc.control_matrix_periodic(pulse.get_total_phases(omega), pulse.get_control_matrix(omega),
                                       pulse.total_propagator_liouville, repeats)
    # both sides accumulate ~repeats*eps in the phase factor's power
    assert rel_err(per.get_control_matrix(omega), want) < 1e-9
    assert rel_err(per.total_propagator, np.linalg.matrix_power(pulse.total_propagator, repeats)) < 1e-10
    if repeats == 1001:
        seq = ff.concatenate([pulse]*repeats)
        assert rel_err(seq.get_control_matrix(omega), want) < 1e-9
        assert rel_err(seq.get_filter_function(omega), per.get_filter_function(omega)) < 1e-9


@pytest.mark.slow
@pytest.mark.parametrize('N,complex_L', [(4, False), (9, False), (16, True), (64, False)])
def test_control_matrix_periodic_by_doubling(N, complex_L):
    """The doubling sum against the term-by-term sum (every bit pattern of small repeat counts) and
    against the oracle's closed form (large counts); real and complex Liouville propagators."""
    rng = np.random.default_rng(N)
    A, W = 3, 200
    R1 = rng.standard_normal((A, N, W)) + 1j*rng.standard_normal((A, N, W))
    z = np.exp(1j*rng.uniform(0, 2*np.pi, W))
    if complex_L:
        L = np.linalg.qr(rng.standard_normal((N, N)) + 1j*rng.standard_normal((N, N)))[0]
    else:
        L = np.linalg.qr(rng.standard_normal((N, N)))[0]
    T = np.multiply.outer(z, L)
    term, total = np.broadcast_to(np.eye(N, dtype=complex), T.shape), np.zeros_like(T)
    for reps in range(1, 20):
        total = total + term
        term = term @ T
        want = (R1.transpose(2, 0, 1) @ total).transpose(1, 2, 0)
        got = numeric.calculate_control_matrix_periodic(z, R1, L, reps)
        assert rel_err(got, want) < 1e-13, reps
    for reps in (255, 256, 1000, 12345):
        got = numeric.calculate_control_matrix_periodic(z, R1, L, reps)
        assert rel_err(got, orc.control_matrix_periodic(z, R1, L, reps)) < 1e-10, reps
    with pytest.raises(ValueError):
        numeric.calculate_control_matrix_periodic(z, R1, L, 0)
    with pytest.raises(ValueError):
        numeric.calculate_control_matrix_periodic(z[:-1], R1, L, 3)


@pytest.mark.slow
def test_control_matrix_periodic_where_the_closed_form_is_singular():
    """exp(i w T) Q = 1 (idle pulse at w = 0, or w T a multiple of 2 pi): the reference has to fall
    back to the explicit sum there; the doubling sum needs no special case -- G identical terms."""
    rng = np.random.default_rng(5)
    A, N, W = 2, 4, 64
    R1 = rng.standard_normal((A, N, W)) + 1j*rng.standard_normal((A, N, W))
    z = np.ones(W, dtype=complex)
    got = numeric.calculate_control_matrix_periodic(z, R1, np.eye(N), 1000)
    assert rel_err(got, 1000*R1) < 1e-15
    assert rel_err(got, orc.control_matrix_periodic(z, R1, np.eye(N), 1000)) < 1e-15


@pytest.mark.parametrize('d,G,T,hermitian', [(2, 50, 3, True), (4, 300, 5, True), (3, 17, 17, False),
                                              (2, 2, 1, True)])
def test_concatenate_sequence_in_one_call(d, G, T, hermitian):
    """ffk_concatenate_sequence (gather -> prefix products -> Liouville -> table rule, all on the
    device) against the same steps done one by one: NumPy cumulative products, the oracle's
    Liouville representation and concatenation rule."""
    rng = np.random.default_rng(10*d + G)
    A, W = 2, 150
    N = d*d
    basis = np.asarray(ff.Basis.ggm(d))
    if not hermitian:        # a non-Hermitian orthonormal basis: complex Liouville propagators
        mix = np.linalg.qr(rng.standard_normal((N, N)) + 1j*rng.standard_normal((N, N)))[0]
        basis = np.tensordot(mix, basis, axes=[1, 0])
    U = np.linalg.qr(rng.standard_normal((T, d, d)) + 1j*rng.standard_normal((T, d, d)))[0]
    table = rng.standard_normal((T, A, N, W)) + 1j*rng.standard_normal((T, A, N, W))
    phases = np.exp(1j*rng.uniform(0, 2*np.pi, (T, W)))
    index = rng.integers(0, T, G).astype(np.int32)
    cum = [U[index[0]]]
    for g in range(1, G):
        cum.append(U[index[g]] @ cum[-1])
    cum = np.array(cum)
    L = orc.liouville_representation(cum[:-1], basis)
    if hermitian:
        assert np.abs(L.imag).max() < 1e-13
        L = L.real
    want = orc.control_matrix_from_atomic(np.cumprod(phases[index[:-1]], axis=0), table[index], L)
    R, total, Lgot = numeric.concatenate_sequence_indexed(U, phases, table, index, basis, return_liouville=True)
    assert rel_err(total, cum[-1]) < 1e-13
    assert Lgot.dtype == (np.float64 if hermitian else np.complex128) and rel_err(Lgot, L) < 1e-13
    assert rel_err(R, want) < 1e-12
    R2, _, _, F = numeric.concatenate_sequence_indexed(U, phases, table, index, basis,
                                                       return_filter_function=True)
    assert np.array_equal(R2, R) and rel_err(F, orc.filter_function(want)) < 1e-12
    Rc, _, none = numeric.concatenate_sequence_indexed(U, phases, table, index, basis, which='correlations')
    assert none is None and Rc.shape == (G, A, N, W) and rel_err(Rc.sum(axis=0), want) < 1e-12
    with pytest.raises(ValueError):
        numeric.concatenate_sequence_indexed(U, phases, table, index + T, basis)
    with pytest.raises(ValueError):
        numeric.concatenate_sequence_indexed(U[:-1] if T > 1 else U[:, :1], phases, table, index, basis)


@pytest.mark.parametrize('d', [2, 4])
def test_concatenate_from_resident_control_matrices(d, monkeypatch):
    """Pulses evaluated by the resident pass keep their control matrices in HBM; ff.concatenate then
    assembles the table there (ffk_concatenate_sequence_resident).  Same results as the route
    through host tables (deep copies of the pulses carry host arrays only) and as the from-scratch
    evaluation of the concatenated pulse; the resident route is actually the one taken."""
    import copy
    rng = np.random.default_rng(d)
    basis = ff.Basis.pauli(int(np.log2(d)))

    def herm(n):
        M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
        return M + M.conj().transpose(0, 2, 1)
    c_opers, n_opers = herm(2), herm(3)
    omega = np.geomspace(1e-2, 1e2, 300)
    pulses = []
    for k in range(4):
        n_dt = int(rng.integers(1, 6))
        pulses.append(ff.PulseSequence(
            [[c_opers[i], rng.standard_normal(n_dt), f'c{i}'] for i in range(2)],
            [[n_opers[a], np.full(n_dt, 1.0 + a), f'n{a}'] for a in range(3)],
            rng.random(n_dt) + 0.1, basis))
        pulses[-1].get_filter_function(omega)
        assert pulses[-1]._resident is not None
    index = rng.integers(0, 4, 60)
    calls = []
    real = numeric.concatenate_sequence_resident
    monkeypatch.setattr(numeric, 'concatenate_sequence_resident',
                        lambda *args, **kwargs: calls.append(1) or real(*args, **kwargs))
    total = ff.concatenate([pulses[k] for k in index])
    assert calls == [1]
    # the concatenated pulse is as resident as its parts: control matrix still in HBM, infidelity on
    # the resident F, and it can take part in the next concatenation without leaving the device
    from filter_functions_amd._resident import Deferred
    assert total._resident is not None and isinstance(total._frequency_data.peek('control_matrix'), Deferred)
    S = 1e-3/omega
    infid_resident = ff.infidelity(total, S, omega)
    nested = ff.concatenate([total, pulses[1], total])
    assert calls == [1, 1] and nested._resident is not None
    calls.pop()
    copies = [copy.deepcopy(p) for p in pulses]
    assert all(c._resident is None and c.is_cached('control_matrix') for c in copies)
    via_host = ff.concatenate([copies[k] for k in index])
    assert calls == [1]
    scratch = ff.concatenate_without_filter_function([pulses[k] for k in index])
    assert rel_err(total.get_control_matrix(omega), via_host.get_control_matrix(omega)) < 1e-13
    assert rel_err(total.get_filter_function(omega), via_host.get_filter_function(omega)) < 1e-13
    assert rel_err(total.total_propagator, via_host.total_propagator) < 1e-13
    assert rel_err(total.get_control_matrix(omega), scratch.get_control_matrix(omega)) < 1e-11
    assert not isinstance(total._frequency_data.peek('control_matrix'), Deferred)     # fetched by now
    assert rel_err(infid_resident, ff.infidelity(via_host, S, omega)) < 1e-13
    nested_host = ff.concatenate([via_host, copies[1], via_host])
    assert rel_err(nested.get_control_matrix(omega), nested_host.get_control_matrix(omega)) < 1e-13
    assert rel_err(nested.total_propagator, nested_host.total_propagator) < 1e-13
    assert rel_err(ff.infidelity(nested, S, omega), ff.infidelity(nested_host, S, omega)) < 1e-13
    clone = copy.deepcopy(total)                  # copies own host arrays only
    assert clone._resident is None and rel_err(clone.get_control_matrix(omega), total.get_control_matrix(omega)) == 0
    # pulse correlations and a changed grid on one pulse (host route again, transparently)
    pc = ff.concatenate([pulses[k] for k in index[:7]], calc_pulse_correlation_FF=True)
    assert calls == [1, 1]
    ref = ff.concatenate([copies[k] for k in index[:7]], calc_pulse_correlation_FF=True)
    assert rel_err(pc.get_pulse_correlation_filter_function(), ref.get_pulse_correlation_filter_function()) < 1e-13
    pulses[0].cache_control_matrix(omega, pulses[0].get_control_matrix(omega))     # explicit store
    assert pulses[0]._resident is None
    again = ff.concatenate([pulses[k] for k in index])
    assert calls == [1, 1] and rel_err(again.get_control_matrix(omega), total.get_control_matrix(omega)) < 1e-13


def test_round2_entry_points_reject_bad_arguments():
    """The entry points added late in round 2 answer malformed calls with FFK_EINVAL (ValueError in
    the binding) and a message, not with a fault: NULL pointers, empty axes, aliasing outputs,
    mismatched or missing resident results."""
    import ctypes
    from filter_functions_amd._resident import ResidentResult
    lib = _lib.load()
    z = np.ones(8, complex)
    R = np.ones((2, 4, 8), complex)
    L = np.eye(4)
    out = np.empty_like(R)
    args = (_lib.ptr(z), _lib.ptr(R), _lib.ptr(L), 0)
    for bad in ((*args, 0, 2, 4, 8, _lib.ptr(out)),            # repeats < 1
                (*args, 3, 0, 4, 8, _lib.ptr(out)),            # empty axis
                (*args, 3, 2, 4, 8, None)):                    # NULL output
        with pytest.raises(ValueError):
            _lib.check(lib.ffk_control_matrix_periodic(*bad))
    assert b'' != lib.ffk_last_error()
    # sequence call: index out of range, NULL table, filter function asked for with which = 1
    U = np.tile(np.eye(2, dtype=complex), (2, 1, 1))
    table = np.ones((2, 1, 4, 8), complex)
    ph = np.ones((2, 8), complex)
    basis = np.asarray(ff.Basis.pauli(1))
    idx = np.array([0, 1, 2], dtype=np.int32)
    Rt, tot, F = np.empty((1, 4, 8), complex), np.empty((2, 2), complex), np.empty((1, 1, 8), complex)

    def sequence(index, table_ptr, which, F_ptr):
        return lib.ffk_concatenate_sequence(_lib.ptr(U), _lib.ptr(ph), table_ptr,
                                            index.ctypes.data_as(ctypes.c_void_p), _lib.ptr(basis), 1, 2,
                                            len(index), 2, 1, 4, 8, which, _lib.ptr(Rt), _lib.ptr(tot), None, F_ptr)
    for status in (sequence(idx, _lib.ptr(table), 0, None), sequence(idx[:2], None, 0, None),
                   sequence(idx[:2], _lib.ptr(table), 1, _lib.ptr(F))):
        with pytest.raises(ValueError):
            _lib.check(status)
    _lib.check(sequence(idx[:2], _lib.ptr(table), 0, _lib.ptr(F)))          # and the well-formed call works
    # resident variants: a handle without a result, a result that is also an input
    empty, other = ResidentResult(), ResidentResult()
    handles = (ctypes.c_void_p*1)(empty.handle)
    tau = np.ones(1)
    one = np.zeros(2, dtype=np.int32)

    def resident(handle_array, result):
        return lib.ffk_concatenate_sequence_resident(handle_array, _lib.ptr(tau), one.ctypes.data_as(ctypes.c_void_p),
                                                     _lib.ptr(basis), 1, 1, 2, 0, _lib.ptr(Rt), _lib.ptr(tot),
                                                     None, _lib.ptr(F), result)
    with pytest.raises(ValueError):
        _lib.check(resident(handles, None))                     # no resident result in the handle
    pulse = ff.PulseSequence([[util.paulis[1], [1.0]]], [[util.paulis[3], [1.0]]], [1.0])
    pulse.get_filter_function(np.linspace(0.1, 1, 8))
    handles = (ctypes.c_void_p*1)(pulse._resident.handle)
    with pytest.raises(ValueError):
        _lib.check(resident(handles, pulse._resident.handle))   # result must not be an input
    _lib.check(resident(handles, other.handle))                 # well formed: result kept in `other`
    with pytest.raises(ValueError):                             # controls route: NULL operators
        _lib.check(lib.ffk_resident_filter_function_from_controls(
            empty.handle, None, 1, _lib.ptr(tau), _lib.ptr(tau), _lib.ptr(np.array([0.0, 1.0])), 1, 2,
            _lib.ptr(tau), 1, _lib.ptr(basis), 4, _lib.ptr(basis[3:]), 1, _lib.ptr(tau),
            *(ctypes.byref(ctypes.c_void_p()) for _ in range(4))))


@pytest.mark.parametrize('G,T', [(1001, 3), (999, 1), (137, 5)])
def test_indexed_concatenation_with_uneven_slabs(G, T):
    """Gather-from-table concatenation at position counts that leave the last pulse-axis slab short
    (or, before the slab count was derived from the slab length, empty)."""
    rng = np.random.default_rng(G)
    A, N, W = 2, 4, 300
    table = rng.standard_normal((T, A, N, W)) + 1j*rng.standard_normal((T, A, N, W))
    phases = np.exp(1j*rng.uniform(0, 2*np.pi, (T, W)))
    index = rng.integers(0, T, G).astype(np.int32)
    rot = np.linalg.qr(rng.standard_normal((G - 1, N, N)))[0]
    got = numeric.calculate_control_matrix_from_atomic_indexed(phases, table, index, rot)
    cum = np.cumprod(phases[index[:-1]], axis=0)
    want = orc.control_matrix_from_atomic(cum, table[index], rot)
    assert rel_err(got, want) < 1e-12


@pytest.mark.slow
@pytest.mark.parametrize('name', ['q1', 'g3', 'p4'])
def test_device_resident_infidelity_gradient_with_logical_omega_shards(name):
    """DevicePipeline.infidelity_gradient (device pointers, no host transfers): the whole grid and
    two frequency blocks integrated with the global trapezoid weights against the reference's
    infidelity derivative, with and without n_coeffs_deriv."""
    import torch
    from filter_functions_amd.device import DevicePipeline
    from filter_functions_amd.parallel import shard_bounds
    g = load_golden('gradient')
    omega = g[f'{name}_omega']
    om_dev = torch.from_numpy(omega).cuda()
    # the reference orders operators by identifier; the pipeline takes arrays as given
    ci = np.argsort(g[f'{name}_c_oper_identifiers'])
    ni = np.argsort(g[f'{name}_n_oper_identifiers'])
    ncd = g[f'{name}_n_coeffs_deriv']
    for i in (1, 2):
        S = g[f'{name}_S{i}']
        for blocks in (1, 2):
            total = total_ncd = None
            for rank in range(blocks):
                w0, w1 = shard_bounds(len(omega), blocks, rank)
                pipe = DevicePipeline(g[f'{name}_c_opers'][ci], g[f'{name}_c_coeffs'][ci],
                                      g[f'{name}_n_opers'][ni], g[f'{name}_n_coeffs'][ni],
                                      g[f'{name}_dt'], g[f'{name}_basis'], omega[w0:w1],
                                      spectrum=S[..., w0:w1])
                pipe.launch(with_infidelity=False)
                part = pipe.infidelity_gradient(omega_global=om_dev, w_offset=w0)
                total = part if total is None else total + part
                part = pipe.infidelity_gradient(omega_global=om_dev, w_offset=w0, n_coeffs_deriv=ncd)
                total_ncd = part if total_ncd is None else total_ncd + part
            assert rel_err(total.cpu().numpy(), g[f'{name}_infidelity_derivative_S{i}']) < TOL
            assert rel_err(total_ncd.cpu().numpy(), g[f'{name}_infidelity_derivative_ncd_S{i}']) < TOL


# ---- qubit registers: remap and extend -------------------------------------------------------------
def _register_pulses():
    g = load_golden('register')
    out = {}
    for name in ('p1', 'p1b', 'p2', 'p3'):
        out[name] = ff.PulseSequence.from_arrays(
            g[f'{name}_c_opers'], g[f'{name}_c_oper_identifiers'], g[f'{name}_c_coeffs'],
            g[f'{name}_n_opers'], g[f'{name}_n_oper_identifiers'], g[f'{name}_n_coeffs'],
            g[f'{name}_dt'], ff.Basis(g[f'{name}_basis'], btype='Pauli'))
        out[name].cache_filter_function(g['omega'])
    return g, out


def _check_register(g, prefix, pulse, tol=TOL):
    omega = g['omega']
    assert list(pulse.c_oper_identifiers) == list(g[f'{prefix}_c_oper_identifiers'])
    assert list(pulse.n_oper_identifiers) == list(g[f'{prefix}_n_oper_identifiers'])
    for attr in ('c_opers', 'n_opers', 'c_coeffs', 'n_coeffs'):
        assert rel_err(getattr(pulse, attr), g[f'{prefix}_{attr}']) < 1e-14, attr
    assert pulse.is_cached('control_matrix') and pulse.is_cached('filter_function')
    assert rel_err(pulse.get_control_matrix(omega), g[f'{prefix}_control_matrix']) < tol
    assert rel_err(pulse.get_filter_function(omega), g[f'{prefix}_filter_function']) < tol
    assert rel_err(pulse.total_propagator_liouville, g[f'{prefix}_total_propagator_liouville']) < tol
    # ... and the retained data are what a from-scratch evaluation of the new pulse gives
    fresh = ff.PulseSequence.from_arrays(pulse.c_opers, pulse.c_oper_identifiers, pulse.c_coeffs,
                                         pulse.n_opers, pulse.n_oper_identifiers, pulse.n_coeffs,
                                         pulse.dt, pulse.basis)
    assert rel_err(pulse.get_filter_function(omega), fresh.get_filter_function(omega)) < tol


@pytest.mark.slow
def test_remap_retains_cached_filter_functions():
    """remap (reference pulse_sequence.py:1976-2120): permuted tensor factors, identifier mapping,
    cached diagonalisation, control matrix and Liouville propagator through the Pauli basis
    permutation -- against the reference's outputs and a from-scratch evaluation."""
    g, p = _register_pulses()
    _check_register(g, 'remap_p2_10', ff.remap(p['p2'], (1, 0)))
    _check_register(g, 'remap_p3_201', ff.remap(p['p3'], (2, 0, 1)))
    mapping = {str(k): str(k) + '_x' for k in g['mapping_keys']}
    _check_register(g, 'remap_p2_10_mapped', ff.remap(p['p2'], (1, 0),
                                                      oper_identifier_mapping=mapping))
    twice = ff.remap(ff.remap(p['p3'], (2, 0, 1)), (1, 2, 0))
    assert rel_err(twice.get_control_matrix(g['omega']), p['p3'].get_control_matrix(g['omega'])) < TOL
    with pytest.raises(ValueError):
        ff.remap(p['p2'], (0, 0))


@pytest.mark.slow
def test_extend_retains_cached_filter_functions():
    """extend (reference pulse_sequence.py:2123-2625): single- and multi-qubit pulses on a larger
    register, a permuted two-qubit pulse, an additional noise Hamiltonian on the whole register."""
    g, p = _register_pulses()
    _check_register(g, 'extend_singles', ff.extend([(p['p1'], 0), (p['p1b'], 2)], N=3))
    ext = ff.extend([(p['p2'], (2, 0)), (p['p1'], 1)], N=4)
    _check_register(g, 'extend_multi', ext)
    assert ext.d == 16 and ext.basis.btype == 'Pauli'
    assert rel_err(ext.eigvals, g['extend_multi_eigvals']) < TOL
    ZZ = util.tensor(util.paulis[3], np.eye(2), util.paulis[3])
    _check_register(g, 'extend_additional',
                    ff.extend([(p['p1'], 0), (p['p1b'], 2)], N=3,
                              additional_noise_Hamiltonian=[[ZZ, np.ones(3), 'ZZ']]))
    with pytest.raises(ValueError):
        ff.extend([(p['p1'], 0), (p['p1b'], 0)])                  # qubit clash
    with pytest.raises(ValueError):
        ff.extend([(p['p1'], 0), (p['p1b'], 2)], N=2)             # register too small
    with pytest.raises(ValueError):
        ff.extend([(p['p2'], 0)])                                 # dimension mismatch
    with pytest.warns(UserWarning):
        assert ff.extend([(p['p1'], 0)], N=1) is p['p1']


def test_libffk_before_torch_shares_one_hip_runtime():
    """libffk used first, torch.cuda initialised afterwards, in a fresh interpreter: both must see
    the GPU (one HIP/HSA runtime in the process, _lib._share_hip_runtime_with_torch)."""
    import subprocess
    import sys
    code = ('import numpy as np, filter_functions_amd as ff\n'
            'from filter_functions_amd import _lib\n'
            'assert _lib.device_count() >= 1\n'
            'D, V, Q = ff.numeric.diagonalize(np.array([np.diag([1.0, -1.0]).astype(complex)]), '
            'np.array([0.5]))\n'
            'import torch\n'
            'x = torch.ones(4, device="cuda")\n'
            'assert float(x.sum()) == 4.0\n'
            'print("shared", D.ravel())\n')
    # Seen once in about ten runs of the suite on the pool's boxes (round 5): the child printed nothing in 300 s -- it
    # hung somewhere in its own GPU start-up, with the same library that passes before and after.  One hang is retried
    # in a fresh child; two in a row are reported as a failure (a real initialisation-order deadlock between libffk
    # and torch is exactly what this test exists to catch -- ADVICE r5).
    res, hung = None, []
    for attempt in range(2):
        try:
            res = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True,
                                 timeout=200)
            break
        except subprocess.TimeoutExpired as exc:
            hung.append((exc.stderr or b'')[-1000:])
    assert res is not None, f'the child interpreter hung twice in GPU start-up: {hung}'
    assert res.returncode == 0 and 'shared' in res.stdout, res.stderr[-2000:]


def test_many_noise_operators_fused_expansion():
    """Many noise operators at small d: the fused chunk-sum + expansion + F kernel with an LDS
    footprint above 48 and above 64 KiB (A*d^2 up to 256), against the oracle."""
    rng = np.random.default_rng(3)
    for d, A, G, W in [(4, 12, 40, 300), (4, 16, 33, 100), (2, 40, 20, 77), (4, 9, 64, 130)]:
        def herm(n):
            M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
            return (M + M.conj().transpose(0, 2, 1))/2
        c_opers, n_opers = herm(2), herm(A)
        c_coeffs, n_coeffs = rng.standard_normal((2, G)), rng.random((A, G))
        dt = 1 - rng.random(G)*0.5
        omega = np.geomspace(1e-2, 50, W)
        ids = [f'n{i:02d}' for i in range(A)]
        pulse = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs, ids)),
                                 dt, ff.Basis.pauli(int(np.log2(d))))
        F = pulse.get_filter_function(omega)
        R = pulse.get_control_matrix(omega)
        D, V, Q = orc.diagonalize(orc.hamiltonian(pulse.c_opers, pulse.c_coeffs), dt)
        R_ref = orc.control_matrix_from_scratch(D, V, Q, omega, np.asarray(pulse.basis),
                                                pulse.n_opers, pulse.n_coeffs, dt)
        tag = f'd={d} A={A} G={G} W={W}'
        assert rel_err(R, R_ref) < TOL, tag
        assert rel_err(F, orc.filter_function(R_ref)) < TOL, tag


# ---- round 2: resident evaluation, large pair grids, complex spectra, device-side status ---------
@pytest.mark.parametrize('d,G,A', [(4, 6, 3), (8, 5, 3), (3, 7, 2), (16, 3, 4), (12, 3, 5), (2, 9, 1)])
def test_frequencies_on_and_around_the_resonances(d, G, A):
    """The generated integral e^{i w t} (e^{i x dt} - 1)/(i x), x = w + (D_m - D_n), at frequencies
    that hit a resonance x = 0 exactly, miss it by a few ulp, and sit on either side of the switch
    between the addition-theorem form and the direct evaluation (|x dt| = 2^-4): control matrix
    against the oracle.  (ffk_math.h::phased_integral_aa; every accumulate kernel.)"""
    rng = np.random.default_rng(77*d + G)
    basis = ff.Basis.ggm(d)
    c_opers = rng.standard_normal((3, d, d)) + 1j*rng.standard_normal((3, d, d))
    c_opers = c_opers + c_opers.conj().transpose(0, 2, 1)
    n_opers = rng.standard_normal((A, d, d)) + 1j*rng.standard_normal((A, d, d))
    n_opers = n_opers + n_opers.conj().transpose(0, 2, 1)
    H = np.einsum('ijk,il->ljk', c_opers, rng.standard_normal((3, G)))
    H[1] = 0.0                                            # an idle segment: all differences zero
    dt = 0.5 + rng.random(G)
    n_coeffs = rng.random((A, G)) + 0.5
    D, V, Q = numeric.diagonalize(H, dt)
    omega = [0.0]
    for g in (0, G - 1):
        dE = (D[g][:, None] - D[g][None, :]).ravel()
        dE = dE[dE != 0][:6]
        for eps in (0.0, 2.0**-52, -2.0**-50, 1e-12, -1e-9, 1e-6):
            omega.extend(-dE*(1 + eps))
        for edge in (2.0**-4, -2.0**-4):                  # |x dt| on either side of the switch
            for nudge in (1 - 2.0**-40, 1 + 2.0**-40):
                omega.extend(-dE + edge*nudge/dt[g])
    omega = np.array(sorted(set(omega)))
    R = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
    t = np.concatenate(([0], dt.cumsum()))
    R_ref = orc.control_matrix_from_scratch(D, V, Q, omega, np.asarray(basis), n_opers, n_coeffs, dt, t)
    assert np.isfinite(R).all()
    assert rel_err(R, R_ref) < 1e-12
    # frequency by frequency, so that one bad column cannot hide behind the norm of the rest
    num = np.abs(R - R_ref).max(axis=(0, 1))
    den = np.abs(R_ref).max(axis=(0, 1))
    assert (num <= 1e-11*den).all(), omega[np.argmax(num/den)]


def test_infidelity_on_a_fresh_pulse_is_one_library_call():
    """ff.infidelity(pulse, S, omega) on a pulse with nothing cached: path and integral in ONE pass
    (ffk_resident_filter_function_infidelity) -- same integrals as the two-call route and as the
    array route for spectra of one, two and three dimensions, identifier subsets and complex
    spectra; the filter function is cached afterwards; a second call integrates the resident F."""
    c_opers, c_coeffs, n_opers, n_coeffs, dt, omega = config2_inputs(G=30, W=500, seed=11)
    basis = ff.Basis.pauli(2)
    H_c, H_n = list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs))

    def fresh():
        return ff.PulseSequence(H_c, H_n, dt, basis)
    rng = np.random.default_rng(3)
    S1 = 1e-3/omega
    S2 = np.outer([1.0, 2.0, 3.0], 1e-3/omega)
    X = rng.standard_normal((3, 3, len(omega)))
    S3 = (np.einsum('abo,cbo->aco', X, X) + 0j)*1e-3
    S2c = S2*(1 + 0.3j)
    lib = _lib.load()
    for S, ids in ((S1, None), (S2, None), (S3, None), (S2c, None), (S2[[2, 0]], [2, 0]), (S1, [1])):
        one = fresh()
        kw = {} if ids is None else {'n_oper_identifiers': one.n_oper_identifiers[ids]}
        got = ff.infidelity(one, S, omega, **kw)
        assert one._resident is not None and one.is_cached('filter_function')
        two = fresh()
        two.get_filter_function(omega)
        ref2 = ff.infidelity(two, S, omega, **kw)
        arr = fresh()
        arr.diagonalize()                                   # anything cached -> array route
        ref = ff.infidelity(arr, S, omega, **kw)
        assert got.shape == ref.shape == ref2.shape
        assert rel_err(got, ref2) < 1e-14 and rel_err(got, ref) < 1e-13
        assert rel_err(one.get_filter_function(omega), arr.get_filter_function(omega)) < 1e-13
        assert rel_err(ff.infidelity(one, S, omega, **kw), got) < 1e-14      # resident F, second call
    with pytest.raises(ValueError):
        ff.infidelity(fresh(), np.ones((2, 5)), omega)


def test_resident_pass_replayed_from_its_captured_graph():
    """The user-facing pass is captured as a hipGraph the first time a shape runs on a pair of pooled
    blocks and REPLAYED afterwards (ffk_api_resident.hip::resident_pass): pulses of one shape evaluated one
    after the other (each on a new handle that gets the previous one's blocks), another shape in
    between, a tuning knob changed in between -- every result against the array route."""
    import gc
    lib = _lib.load()
    basis = ff.Basis.pauli(2)

    def one(seed, G, W, controls=True):
        c_opers, c_coeffs, n_opers, n_coeffs, dt, omega = config2_inputs(G=G, W=W, seed=seed)
        H_c, H_n = list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs))
        fast = ff.PulseSequence(H_c, H_n, dt, basis)
        slow = ff.PulseSequence(H_c, H_n, dt, basis)
        slow.diagonalize()
        F = fast.get_filter_function(omega)
        assert fast._resident is not None and slow._resident is None
        assert rel_err(F, slow.get_filter_function(omega)) < 1e-13
        assert rel_err(fast.propagators, slow.propagators) < 1e-13
        S = 1e-3/omega
        assert rel_err(ff.infidelity(fast, S, omega), ff.infidelity(slow, S, omega)) < 1e-13
        assert rel_err(fast.get_control_matrix(omega), slow.get_control_matrix(omega)) < 1e-13
        del fast, slow
        gc.collect()

    for seed in (1, 2, 3):
        one(seed, 24, 300)
    one(4, 7, 65)                       # another shape: its own capture
    one(5, 24, 300)                     # the first shape again
    try:
        _lib.check(lib.ffk_set_segment_chunks(3))
        one(6, 24, 300)                 # knob changed: must not replay the old geometry
        assert _lib.stats()['chunks'] == 3
    finally:
        _lib.check(lib.ffk_set_segment_chunks(0))
    one(7, 24, 300)
    assert _lib.stats()['chunks'] != 3
    # pulses kept ALIVE never get the same pooled blocks back: every key is new, nothing is captured
    # (a capture happens on the second sighting of a key only) and the results are the same
    c_opers, c_coeffs, n_opers, n_coeffs, dt, omega = config2_inputs(G=24, W=300, seed=8)
    H_c, H_n = list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs))
    ref = ff.PulseSequence(H_c, H_n, dt, basis)
    ref.diagonalize()
    F_ref = ref.get_filter_function(omega)
    alive = [ff.PulseSequence(H_c, H_n, dt, basis) for _ in range(12)]
    for p in alive:
        assert rel_err(p.get_filter_function(omega), F_ref) < 1e-13
        assert p._resident is not None


def test_resident_pass_matches_array_path():
    """get_filter_function on a fresh pulse runs as one library call (ffk_resident_*): same
    results as the array-in/array-out route, control matrix fetched from HBM only on demand,
    infidelity integrated on the resident F."""
    from filter_functions_amd._resident import Deferred
    c_opers, c_coeffs, n_opers, n_coeffs, dt, omega = config2_inputs(G=40, W=700)
    basis = ff.Basis.pauli(2)

    def fresh():
        return ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt, basis)
    fast, slow = fresh(), fresh()
    slow.diagonalize()                                   # anything cached -> array route
    F_slow = slow.get_filter_function(omega)
    assert slow._resident is None
    F = fast.get_filter_function(omega)
    assert fast._resident is not None
    assert isinstance(fast._frequency_data.peek('control_matrix'), Deferred)     # still in HBM
    for key in ('control_matrix', 'total_phases', 'filter_function', 'omega'):
        assert fast.is_cached(key)
    assert fast.is_cached('total_propagator_liouville') and fast.is_cached('eigvals')
    assert fast.nbytes == slow.nbytes
    assert rel_err(F, F_slow) < 1e-14 and rel_err(fast.propagators, slow.propagators) < 1e-14
    assert np.array_equal(fast.eigvals, slow.eigvals)
    assert fast.total_propagator is not None and rel_err(fast.total_propagator, slow.total_propagator) < 1e-14
    S1, S2 = 1e-3/omega, np.outer([1.0, 2.0, 3.0], 1e-3/omega)
    X = np.random.default_rng(0).standard_normal((3, 3, len(omega)))
    S3 = (np.einsum('abo,cbo->aco', X, X) + 0j)*1e-3
    for S in (S1, S2, S3):
        assert rel_err(ff.infidelity(fast, S, omega), ff.infidelity(slow, S, omega)) < 1e-13
    ids = fast.n_oper_identifiers[[2, 0]]
    assert rel_err(ff.infidelity(fast, S2[[2, 0]], omega, n_oper_identifiers=ids),
                   ff.infidelity(slow, S2[[2, 0]], omega, n_oper_identifiers=ids)) < 1e-13
    with pytest.raises(ValueError):
        ff.infidelity(fast, np.ones((2, 5)), omega)
    R = fast.get_control_matrix(omega)                   # D2H now
    assert isinstance(R, np.ndarray) and fast.get_control_matrix(omega) is R
    assert rel_err(R, slow.get_control_matrix(omega)) < 1e-14
    assert rel_err(fast.get_total_phases(omega), slow.get_total_phases(omega)) == 0
    assert rel_err(fast.total_propagator_liouville, slow.total_propagator_liouville) < 1e-14
    # results outlive the pulse and its handle
    del fast
    import gc
    gc.collect()
    assert rel_err(F, F_slow) < 1e-14
    # a new frequency grid drops the resident result with everything else
    again = fresh()
    again.get_filter_function(omega)
    again.get_filter_function(omega[:100])
    assert len(again.omega) == 100 and again.get_filter_function(omega[:100]).shape == (3, 3, 100)
    assert rel_err(again.get_filter_function(omega[:100]), F_slow[..., :100]) < 1e-14
    # the mapping views hand out arrays, never placeholders
    view = fresh()
    view.get_filter_function(omega)
    assert isinstance(view.frequency_data['control_matrix'], np.ndarray)
    assert all(isinstance(v, np.ndarray) for v in view.frequency_data.values())


def test_eigensolver_failure_is_reported_on_every_path():
    """NaN in the Hamiltonian: LinAlgError from the array route, the resident route and the
    device-resident pipeline (ffk_eigensolver_status_dev)."""
    import torch
    from filter_functions_amd.device import DevicePipeline
    c_opers, c_coeffs, n_opers, n_coeffs, dt, omega = config2_inputs(G=12, W=64)
    bad = c_coeffs.copy()
    bad[0, 5] = np.nan
    basis = ff.Basis.pauli(2)
    pulse = ff.PulseSequence(list(zip(c_opers, bad)), list(zip(n_opers, n_coeffs)), dt, basis)
    with pytest.raises(np.linalg.LinAlgError):
        pulse.diagonalize()
    with pytest.raises(np.linalg.LinAlgError):
        pulse.get_filter_function(omega)
    pipe = DevicePipeline(c_opers, bad, n_opers, n_coeffs, dt, basis, omega)
    pipe.launch()
    with pytest.raises(np.linalg.LinAlgError):
        pipe.check_status()
    good = DevicePipeline(c_opers, c_coeffs, n_opers, n_coeffs, dt, basis, omega)
    good.launch()
    good.check_status()
    torch.cuda.synchronize()


@pytest.mark.parametrize('W', [2, 1025, 4096, 4097, 9000])
def test_resident_integral_with_the_spectrum_in_host_memory_is_bit_identical(W):
    """The resident route hands the spectrum over in mapped pinned host memory and stages it through LDS in
    batches of 4096 (infid_host_spectrum_kernel); the array route copies it to the device (infid_kernel).
    Same slots, same order: the same bits -- across batch boundaries, for every spectrum rank."""
    from filter_functions_amd import numeric
    c_opers, c_coeffs, n_opers, n_coeffs, dt, _ = config2_inputs(G=7, W=64)
    omega = np.sort(np.random.default_rng(W).uniform(0.1, 30.0, W))
    pulse = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt, ff.Basis.pauli(2))
    F = pulse.get_filter_function(omega)
    A = F.shape[0]
    idx = np.arange(A)
    rng = np.random.default_rng(5)
    for shape in [(W,), (A, W), (A, A, W)]:
        S = rng.uniform(0.5, 1.5, shape)
        if len(shape) == 3:
            S = S + S.transpose(1, 0, 2)
        resident = numeric._integrate_filter_function(F, S, omega, idx, pulse.d, pulse)
        arrays = numeric._integrate_filter_function(np.array(F), S, omega, idx, pulse.d)
        assert resident.shape == arrays.shape
        assert np.array_equal(resident, arrays), (shape, np.abs(resident - arrays).max())


def test_filter_function_pair_grids_beyond_65535():
    """'generalized' at d = 16 has N*N = 65536 basis pairs, a pulse-correlation filter function of
    a long sequence (G*A)^2 operator pairs: both exceed one grid axis."""
    rng = np.random.default_rng(16)
    R = rng.standard_normal((1, 256, 3)) + 1j*rng.standard_normal((1, 256, 3))
    F = numeric.calculate_filter_function(R, 'generalized')
    assert F.shape == (1, 1, 256, 256, 3)
    assert rel_err(F, orc.filter_function(R, 'generalized')) < 1e-15
    # fidelity filter function of 1600 rows (2.56 M operator pairs)
    R = rng.standard_normal((1600, 4, 5)) + 1j*rng.standard_normal((1600, 4, 5))
    F = numeric.calculate_filter_function(R)
    assert rel_err(F, orc.filter_function(R)) < 1e-14
    assert np.array_equal(F, F.conj().swapaxes(0, 1))
    # pulse correlations: (G, A) = (300, 1) 'generalized' -> 90000 operator pairs on grid.z
    Rpc = rng.standard_normal((300, 1, 4, 2)) + 1j*rng.standard_normal((300, 1, 4, 2))
    Fpc = numeric.calculate_pulse_correlation_filter_function(Rpc, 'generalized')
    ref = np.einsum('gako,hblo->ghabklo', Rpc.conj(), Rpc)
    assert Fpc.shape == ref.shape and rel_err(Fpc, ref) < 1e-15


@pytest.mark.parametrize('s_ndim,N,W', [(1, 40, 300), (2, 40, 300), (1, 144, 200), (2, 200, 130), (2, 256, 70)])
def test_decay_amplitudes_complex_spectrum_below_three_dimensions(s_ndim, N, W):
    """A complex spectrum of one or two dimensions makes Gamma_aa non-symmetric in (k, l): the
    GEMM's mirror shortcut must switch itself off -- the tiles below the diagonal, which
    have a launch of their own that returns at once for real weights, must then all be computed.
    N = 40: several 32 x 32 tiles; N >= 128: 64 x 64 tiles, also with a ragged last tile."""
    rng = np.random.default_rng(40 + s_ndim + N)
    A = 2
    R = rng.standard_normal((A, N, W)) + 1j*rng.standard_normal((A, N, W))
    omega = np.sort(rng.random(W))*20 + 1e-3
    shape = (W,) if s_ndim == 1 else (A, W)
    S = rng.random(shape) + 1j*rng.standard_normal(shape)
    got = numeric._decay_amplitudes(R, S, omega, np.arange(A), 'total')
    ref = orc.decay_amplitudes(R, S, omega, np.arange(A))
    assert np.abs(ref - ref.swapaxes(-1, -2)).max() > 1e-3*np.abs(ref).max()   # really asymmetric
    assert rel_err(got, ref) < 1e-12
    real = numeric._decay_amplitudes(R, S.real, omega, np.arange(A), 'total')
    assert rel_err(real, orc.decay_amplitudes(R, S.real, omega, np.arange(A))) < 1e-12
    assert rel_err(real, real.swapaxes(-1, -2)) < 1e-14          # symmetric again for a real spectrum


@pytest.mark.parametrize('G,A,W', [(1, 1, 1), (2, 2, 65), (3, 4, 100), (5, 7, 64), (9, 10, 130),
                                    (33, 3, 7), (4, 6, 40), (3, 13, 70), (2, 12, 33), (6, 9, 31)])
def test_d8_producer_consumer_kernel_ragged_shapes(G, A, W):
    """ctrl_pcr.hip (d = 8): operator counts that do not fill the three-operator blocks, frequency
    tiles that are not full, one- and two-segment chunks, several chunks -- against the oracle and
    against the symmetric kernel (tuning variant 2)."""
    d = 8
    rng = np.random.default_rng(800 + G*A + W)
    basis = ff.Basis.pauli(3)
    c_opers = rng.standard_normal((3, d, d)) + 1j*rng.standard_normal((3, d, d))
    c_opers = c_opers + c_opers.conj().transpose(0, 2, 1)
    n_opers = rng.standard_normal((A, d, d)) + 1j*rng.standard_normal((A, d, d))
    n_opers = n_opers + n_opers.conj().transpose(0, 2, 1)
    H = np.einsum('ijk,il->ljk', c_opers, rng.standard_normal((3, G)))
    dt = 0.5 + rng.random(G)
    n_coeffs = rng.random((A, G)) + 0.5
    omega = np.concatenate(([0.0], np.geomspace(1e-3, 50, W - 1))) if W > 1 else np.array([0.3])
    D, V, Q = numeric.diagonalize(H, dt)
    lib = _lib.load()
    R = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
    assert _lib.stats()['block'] == 1024                          # the 16-wave kernel ran
    R_ref = orc.control_matrix_from_scratch(D, V, Q, omega, np.asarray(basis), n_opers, n_coeffs, dt)
    assert rel_err(R, R_ref) < 1e-12
    try:
        for chunks in (1, 2, 3):
            _lib.check(lib.ffk_set_segment_chunks(chunks))
            R_c = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers,
                                                                n_coeffs, dt)
            assert rel_err(R_c, R_ref) < 1e-12
        _lib.check(lib.ffk_set_segment_chunks(0))
        _lib.check(lib.ffk_set_accumulate_variant(2))
        R_sym = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers,
                                                              n_coeffs, dt)
        assert _lib.stats()['block'] != 1024
        assert rel_err(R_sym, R) < 1e-13
    finally:
        lib.ffk_set_segment_chunks(0)
        lib.ffk_set_accumulate_variant(0)


@pytest.mark.parametrize('d,G,A,W', [(7, 64, 3, 5300), (7, 40, 1, 25001), (11, 24, 3, 700), (11, 9, 7, 1000),
                                      (13, 5, 2, 33), (13, 20, 4, 300), (14, 12, 3, 129), (15, 1, 1, 17),
                                      (15, 30, 5, 260)])
def test_padded_dimensions(d, G, A, W):
    """d = 7, 11, 13, 14, 15 on large enough problems run on the next specialised kernel (8: ctrl_pcr.hip, 12 / 16:
    ctrl_mfma.hip) with decoupled levels added -- operands T (+) 1, Bbar (+) 0, the d x d block of Y copied out
    (ctrl.hip: launch_accumulate, ffk_internal.h: padded_dimension).  Against the oracle, against the dimension's own
    kernel (FFK_NO_PADDED_DIMENSIONS=1, read per call), with forced segment chunks, frequency counts that leave tiles
    partly empty, omega = 0 and a frequency on a resonance.  Reference loop numeric.py:846-869."""
    rng = np.random.default_rng(1000*d + G + A + W)
    basis = ff.Basis.ggm(d)
    c_opers = rng.standard_normal((3, d, d)) + 1j*rng.standard_normal((3, d, d))
    c_opers = c_opers + c_opers.conj().transpose(0, 2, 1)
    n_opers = rng.standard_normal((A, d, d)) + 1j*rng.standard_normal((A, d, d))
    n_opers = n_opers + n_opers.conj().transpose(0, 2, 1)
    H = np.einsum('ijk,il->ljk', c_opers, rng.standard_normal((3, G)))
    dt = 0.5 + rng.random(G)
    n_coeffs = rng.random((A, G)) + 0.5
    omega = np.concatenate(([0.0], np.geomspace(1e-3, 50, W - 1)))
    D, V, Q = numeric.diagonalize(H, dt)
    omega[3] = D[0, 2] - D[0, 1]
    lib = _lib.load()
    R = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
    sub = slice(None) if W*G <= 40000 else np.r_[0:8, W//2:W//2 + 8, W - 8:W]
    R_ref = orc.control_matrix_from_scratch(D, V, Q, omega[sub], np.asarray(basis), n_opers, n_coeffs, dt)
    assert rel_err(R[..., sub], R_ref) < 1e-12
    os.environ['FFK_NO_PADDED_DIMENSIONS'] = '1'
    try:
        R_own = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
    finally:
        del os.environ['FFK_NO_PADDED_DIMENSIONS']
    assert rel_err(R_own, R) < 1e-12
    big = d != 7 or G*W*A >= 1e6
    assert (not np.array_equal(R_own, R)) == big or G == 1       # the padded form ran exactly where it should
    try:
        for chunks in (1, 2, 3):
            _lib.check(lib.ffk_set_segment_chunks(chunks))
            R_c = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
            assert rel_err(R_c, R) < 1e-12, chunks
    finally:
        lib.ffk_set_segment_chunks(0)
    # the Hilbert-space twin reads the same partial sums
    if W <= 1000:
        B = numeric.calculate_noise_operators_from_scratch(D, V, Q, omega, n_opers, n_coeffs, dt)
        B_ref = orc.noise_operators_from_scratch(D, V, Q, omega, n_opers, n_coeffs, dt)
        assert rel_err(B, B_ref) < 1e-12


@pytest.mark.parametrize('G,A,W', [(1, 1, 1), (2, 3, 64), (7, 1, 70), (8, 2, 65), (9, 4, 130), (17, 7, 64), (100, 5, 300),
                                    (33, 3, 129), (260, 3, 64), (64, 6, 31), (1100, 2, 200)])
def test_d2_kernel_ragged_shapes(G, A, W):
    """ctrl_d2.hip (one qubit): operands folded into three 2 x 2 matrices per segment and operator, eight wavefronts
    per block that split the block's segment chunk and add up through LDS.  Fewer segments than wavefronts (some own
    none), chunk counts that leave ragged sub-chunks, operator groups of 3 + 1 / 3 + 2 / 2 + 2, frequency tiles that
    are not full, omega = 0 and a frequency on a resonance -- against the oracle and against the symmetric kernel
    (tuning variant 2) it replaces.  Reference loop numeric.py:846-869."""
    d = 2
    rng = np.random.default_rng(200 + G*A + W)
    basis = ff.Basis.pauli(1)
    c_opers = rng.standard_normal((3, d, d)) + 1j*rng.standard_normal((3, d, d))
    c_opers = c_opers + c_opers.conj().transpose(0, 2, 1)
    n_opers = rng.standard_normal((A, d, d)) + 1j*rng.standard_normal((A, d, d))
    n_opers = n_opers + n_opers.conj().transpose(0, 2, 1)
    H = np.einsum('ijk,il->ljk', c_opers, rng.standard_normal((3, G)))
    dt = 0.5 + rng.random(G)
    n_coeffs = rng.random((A, G)) + 0.5
    omega = np.concatenate(([0.0], np.geomspace(1e-3, 50, W - 1))) if W > 1 else np.array([0.3])
    D, V, Q = numeric.diagonalize(H, dt)
    if W > 4:
        omega[3] = D[0, 1] - D[0, 0]                  # x = omega + dE = 0 exactly for one entry of segment 0
    lib = _lib.load()
    R = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
    st = _lib.stats()
    assert st['block'] == 512 and st['grid_y'] == (A + 2)//3, st          # the d = 2 kernel ran, groups of <= 3
    R_ref = orc.control_matrix_from_scratch(D, V, Q, omega, np.asarray(basis), n_opers, n_coeffs, dt)
    assert rel_err(R, R_ref) < 1e-12
    try:
        for chunks in (1, 2, 3, 5):
            _lib.check(lib.ffk_set_segment_chunks(chunks))
            R_c = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
            assert rel_err(R_c, R_ref) < 1e-12, chunks
        _lib.check(lib.ffk_set_segment_chunks(0))
        _lib.check(lib.ffk_set_accumulate_variant(2))
        R_sym = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
        assert _lib.stats()['block'] != 512 or _lib.stats()['grid_y'] != (A + 2)//3 or A > 3
        assert rel_err(R_sym, R) < 1e-12
    finally:
        lib.ffk_set_segment_chunks(0)
        lib.ffk_set_accumulate_variant(0)
    # and the noise operators (the Hilbert-space twin reads the same accumulation)
    B = numeric.calculate_noise_operators_from_scratch(D, V, Q, omega, n_opers, n_coeffs, dt)
    B_ref = orc.noise_operators_from_scratch(D, V, Q, omega, n_opers, n_coeffs, dt)
    assert rel_err(B, B_ref) < 1e-12


@pytest.mark.parametrize('G,A,W', [(1, 1, 1), (40, 1, 130), (3, 2, 65), (70, 2, 200), (5, 4, 100), (64, 4, 257),
                                    (9, 5, 64), (33, 5, 300), (7, 7, 70), (50, 7, 129), (4, 8, 40), (6, 10, 31),
                                    (2, 13, 33), (300, 4, 64)])
def test_d4_operator_groups_ragged_shapes(G, A, W):
    """ctrl_pq.hip (d = 4): the launch serves A operators as blocks of three plus blocks of two (A = 4: 2 + 2,
    5: 3 + 2, 7: 3 + 2 + 2, 10: 3 + 3 + 2 + 2; A = 1: a single one) -- every block size runs the generated
    consumer loop.  Operator counts of every residue, frequency tiles that are not full,
    chunks shorter and longer than the ring of eight tiles, several chunks -- against the oracle and against the
    symmetric kernel (tuning variant 2); with W_a folded by the prologue kernel (this call) and by the producers
    (the intermediates call brings its own operands).  Reference loop numeric.py:846-869."""
    d = 4
    rng = np.random.default_rng(400 + G*A + W)
    basis = ff.Basis.pauli(2)
    c_opers = rng.standard_normal((3, d, d)) + 1j*rng.standard_normal((3, d, d))
    c_opers = c_opers + c_opers.conj().transpose(0, 2, 1)
    n_opers = rng.standard_normal((A, d, d)) + 1j*rng.standard_normal((A, d, d))
    n_opers = n_opers + n_opers.conj().transpose(0, 2, 1)
    H = np.einsum('ijk,il->ljk', c_opers, rng.standard_normal((3, G)))
    dt = 0.5 + rng.random(G)
    n_coeffs = rng.random((A, G)) + 0.5
    omega = np.concatenate(([0.0], np.geomspace(1e-3, 50, W - 1))) if W > 1 else np.array([0.3])
    D, V, Q = numeric.diagonalize(H, dt)
    lib = _lib.load()
    R = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
    st = _lib.stats()
    assert st['block'] == 768                                     # the producer / consumer kernel ran
    assert st['grid_y'] == {0: A//3, 1: (A - 4)//3 + 2 if A > 1 else 1, 2: (A - 2)//3 + 1}[A % 3], st
    R_ref = orc.control_matrix_from_scratch(D, V, Q, omega, np.asarray(basis), n_opers, n_coeffs, dt)
    assert rel_err(R, R_ref) < 1e-12
    _lib.check_kernel_fault()
    try:
        for chunks in (1, 2, 3):
            _lib.check(lib.ffk_set_segment_chunks(chunks))
            R_c = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
            assert rel_err(R_c, R_ref) < 1e-12
        _lib.check(lib.ffk_set_segment_chunks(0))
        _lib.check(lib.ffk_set_accumulate_variant(2))
        R_sym = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
        assert _lib.stats()['block'] != 768
        assert rel_err(R_sym, R) < 1e-12
    finally:
        lib.ffk_set_segment_chunks(0)
        lib.ffk_set_accumulate_variant(0)
    if G*A <= 200 and W <= 130:
        # the call that materialises the per-segment steps brings its own operands: the producers fold W_a
        R_i, inter = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt,
                                                                   cache_intermediates=True)
        assert rel_err(R_i, R_ref) < 1e-12
        assert rel_err(inter['control_matrix_step'].sum(axis=0), R_ref) < 1e-12


@pytest.mark.parametrize('d,G,n_c', [(2, 1, 5), (2, 700, 2), (4, 33, 3), (3, 2, 20), (8, 16, 6)])
def test_resident_pass_from_controls(d, G, n_c):
    """ffk_resident_filter_function_from_controls (control operators and amplitudes in, the
    Hamiltonian summed on the device -- or on the host for the one- and two-segment pulses whose
    controls do not fit the Hamiltonian's slot) against the same pass on the summed Hamiltonian."""
    from filter_functions_amd._resident import ResidentResult
    rng = np.random.default_rng(100*d + G)

    def rand_herm(n):
        M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
        return (M + M.conj().transpose(0, 2, 1))/2
    c_opers = rand_herm(n_c)
    c_coeffs = rng.standard_normal((n_c, G))
    n_opers = rand_herm(2)
    n_coeffs = rng.random((2, G)) + 0.5
    dt = rng.random(G) + 0.1
    t = np.concatenate([[0.0], dt.cumsum()])
    omega = np.geomspace(1e-2, 1e2, 130)
    basis = np.asarray(ff.Basis.ggm(d))
    H = np.einsum('ijk,il->ljk', c_opers, c_coeffs)
    a, b = ResidentResult(), ResidentResult()
    Da, Va, Qa, Fa = a.evaluate(H, dt, t, omega, basis, n_opers, n_coeffs)
    Db, Vb, Qb, Fb = b.evaluate(c_opers, dt, t, omega, basis, n_opers, n_coeffs, c_coeffs=c_coeffs)
    assert rel_err(Db, Da) < 1e-13 and rel_err(Qb, Qa) < 1e-13 and rel_err(Fb, Fa) < 1e-12
    assert rel_err(b.control_matrix(), a.control_matrix()) < 1e-12
    D, V, Q = orc.diagonalize(H, dt)
    R = orc.control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
    assert rel_err(b.control_matrix(), R) < 1e-11 and rel_err(Fb, orc.filter_function(R)) < 1e-11
    with pytest.raises(ValueError):
        b.evaluate(c_opers, dt, t, omega, basis, n_opers, n_coeffs, c_coeffs=c_coeffs[:, :-1])


def test_one_handle_through_every_kind_of_pass():
    """One ffk_resident handle filled in turn by a single pass, a batched pass, a sequence pass and a single pass
    again: after each, the readers of that kind serve it and the readers of the other kind refuse it; a call
    rejected for its arguments leaves the handle as it was; gates and pulses read in place from single results and
    from members give what host arrays give.  (The three Python owners share one base class: the methods of one
    are called on the handle of another.)"""
    import ctypes
    from filter_functions_amd._resident import ResidentResult
    from filter_functions_amd.batch import BatchResult
    from filter_functions_amd.sequences import SequencePass
    lib = _lib.load()
    d, G, W, A, N, P, n_c = 2, 3, 8, 2, 4, 3, 2
    rng = np.random.default_rng(11)

    def rand_herm(*lead):
        M = rng.standard_normal(lead + (d, d)) + 1j*rng.standard_normal(lead + (d, d))
        return (M + M.conj().swapaxes(-1, -2))/2
    c_opers, c_coeffs = rand_herm(P, n_c), rng.standard_normal((P, n_c, G))
    n_opers, n_coeffs = rand_herm(P, A), rng.random((P, A, G)) + 0.5
    dt = rng.random((P, G)) + 0.1
    t = np.concatenate([np.zeros((P, 1)), dt.cumsum(axis=1)], axis=1)
    omega = np.geomspace(0.1, 10, W)
    basis = np.asarray(ff.Basis.pauli(1))
    S, idx = 1e-3/omega, np.array([0, 1], dtype=np.int32)
    out = np.empty(2)

    def single(res, p=0):
        return res.evaluate(c_opers[p], dt[p], t[p], omega, basis, n_opers[p], n_coeffs[p], c_coeffs=c_coeffs[p])

    def batched(res, n=P):
        return BatchResult.evaluate(res, c_opers[:n], c_coeffs[:n], dt[:n], t[:n], omega, basis, n_opers[:n],
                                    n_coeffs[:n])

    def integral(res, idx):
        idx = np.asarray(idx, dtype=np.int32)
        return lib.ffk_resident_infidelity(res.handle, S.ctypes.data, 1, 1, idx.ctypes.data, len(idx), d,
                                           out.ctypes.data)

    def single_readers(res):
        R, at = np.empty((A, N, W), dtype=complex), ctypes.c_void_p()
        return (lib.ffk_resident_control_matrix(res.handle, R.ctypes.data),
                lib.ffk_resident_control_matrix_dev(res.handle, ctypes.byref(at), None, None), integral(res, [0, 1]))

    def member(res, k):
        R = np.empty((A, N, W), dtype=complex)
        return lib.ffk_resident_batch_control_matrix(res.handle, k, R.ctypes.data), R

    # 1. a single pass
    h = ResidentResult()
    D1, _, Q1, F1 = (x.copy() for x in single(h))
    R1, infid1 = h.control_matrix(), h.infidelity(S, idx, d)
    # 2., 3. calls rejected for their arguments leave it as it was
    assert integral(h, [0, 2]) == _lib.FFK_EINVAL and 'idx' in lib.ffk_last_error().decode()
    assert np.array_equal(h.control_matrix(), R1)
    with pytest.raises(ValueError):
        batched(h, 0)
    assert np.array_equal(h.control_matrix(), R1) and single_readers(h) == (0, 0, 0)
    # 4. a batched pass: the single readers refuse, the members are those of a fresh handle
    batched(h)
    assert single_readers(h) == (_lib.FFK_EINVAL,)*3
    fresh = BatchResult()
    Qb = batched(fresh)[2]
    for k in range(P):
        rc, R = member(h, k)
        assert rc == 0 and rel_err(R, fresh.control_matrix(k)) < 1e-12
    assert member(h, P)[0] == _lib.FFK_EINVAL and member(h, -1)[0] == _lib.FFK_EINVAL
    # 5. a sequence pass whose gates are a single result and a member of a batch
    a = ResidentResult()
    Qa = single(a)[2]
    U, tau = np.array([Qa[-1], Qb[1][-1]]), np.array([dt[0].sum(), dt[1].sum()])
    offsets, index = [0, 2, 5], [0, 1, 1, 0, 1]
    gates = [a.handle.value, fresh.handle.value], [-1, 1], None
    table = np.array([a.control_matrix(), fresh.control_matrix(1)])
    total_h, F_h = SequencePass.evaluate(h, *gates, U, tau, offsets, index, omega, basis, A)
    F_h, R_h = F_h.copy(), [SequencePass.control_matrix(h, j) for j in range(2)]
    assert single_readers(h) == (_lib.FFK_EINVAL,)*3
    for other, args in ((SequencePass(), gates), (SequencePass(), ([None, None], [-1, -1], table))):
        total, F = other.evaluate(*args, U, tau, offsets, index, omega, basis, A)
        assert rel_err(total, total_h) < 1e-13 and rel_err(F, F_h) < 1e-12
        assert all(rel_err(other.control_matrix(j), R_h[j]) < 1e-12 for j in range(2))
    # 6. decay amplitudes of the two members, a single result and a host array, against four host arrays
    Sc = S.astype(complex)

    def decay(handles, slots, table):
        gamma = np.empty((4, 2, N, N))
        slots, table = np.array(slots, dtype=np.int32), np.ascontiguousarray(table)
        _lib.check(lib.ffk_resident_batch_processes(
            (ctypes.c_void_p*4)(*handles), slots.ctypes.data, table.ctypes.data, 4, A, N, W, d, omega.ctypes.data,
            basis.ctypes.data, 1, Sc.ctypes.data, 1, idx.ctypes.data, 2, gamma.ctypes.data, None, None, None))
        return gamma
    last = fresh.control_matrix(2)
    gamma = decay([h.handle.value, h.handle.value, a.handle.value, None], [0, 1, -1, -1], last[None])
    assert rel_err(gamma, decay([None]*4, [-1]*4, np.array(R_h + [table[0], last]))) < 1e-12
    # 7. the single pass again: the same results, the single readers serve it, the batched reader refuses
    D, V, Q, F = single(h)
    assert rel_err(D, D1) < 1e-13 and rel_err(Q, Q1) < 1e-13 and rel_err(F, F1) < 1e-12
    assert rel_err(h.control_matrix(), R1) < 1e-12 and single_readers(h) == (0, 0, 0)
    assert rel_err(h.infidelity(S, idx, d), infid1) < 1e-12
    assert member(h, 0)[0] == _lib.FFK_EINVAL


def test_copies_and_pickles_of_a_pulse_with_a_resident_result():
    """deepcopy / pickle of a pulse whose control matrix still lives in HBM: the copy holds host
    arrays and no device memory, the original keeps working, both give the same numbers."""
    import copy
    import pickle
    c_opers, c_coeffs, n_opers, n_coeffs, dt, omega = config2_inputs(G=12, W=200)
    basis = ff.Basis.pauli(2)
    pulse = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt, basis)
    F = pulse.get_filter_function(omega)
    S = 1e-3/omega
    ref = ff.infidelity(pulse, S, omega)
    for clone in (copy.deepcopy(pulse), pickle.loads(pickle.dumps(pulse)), ff.concatenate([pulse])):
        assert clone._resident is None and clone == pulse
        assert clone.is_cached('control_matrix') and clone.is_cached('filter_function')
        assert np.array_equal(clone.get_filter_function(omega), F)
        assert rel_err(ff.infidelity(clone, S, omega), ref) < 1e-14          # array route
        assert np.array_equal(clone.get_control_matrix(omega), pulse.get_control_matrix(omega))
    shallow = copy.copy(pulse)
    assert shallow._resident is pulse._resident
    del pulse
    assert rel_err(ff.infidelity(shallow, S, omega), ref) == 0                # resident route


def test_captured_pass_replays_bit_identically():
    """A pass of the hot path captured into a hipGraph (ffk_graph_*) and replayed 100 times -- on
    the capture stream's sibling, on the null stream, with the inputs changed between replays --
    gives bit for bit what the same calls give enqueued one by one (reference
    call: pulse_sequence.py:691-805)."""
    import torch
    import workloads as wl
    from filter_functions_amd.device import DevicePipeline, capture
    from filter_functions_amd.parallel import ShardedStepRing
    device = torch.device('cuda', 0)
    cfg = dict(wl.CONFIG2, G=48)
    c_opers, c_coeffs, n_opers, n_coeffs, dt = wl.random_pulse_inputs(**cfg)
    omega = wl.random_pulse_omega(dt, 640)
    basis = ff.Basis.pauli(2)
    S = 1e-3/omega

    def make():
        return DevicePipeline(c_opers, c_coeffs, n_opers, n_coeffs, dt, basis, omega, spectrum=S,
                              device=device)
    eager, replayed = make(), make()
    eager.launch()
    torch.cuda.synchronize(device)
    want = [t.clone() for t in (eager.eigvals, eager.propagators, eager.control_matrix,
                                eager.filter_function, eager.infid)]
    graph = replayed.graph()
    assert graph.nodes >= 5 and replayed.graph() is graph          # cached
    side = torch.cuda.Stream(device=device)
    for i in range(100):
        for t in (replayed.control_matrix, replayed.filter_function, replayed.infid):
            t.zero_()
        torch.cuda.synchronize(device)
        graph.launch(side.cuda_stream if i % 2 else None)
        torch.cuda.synchronize(device)
        got = (replayed.eigvals, replayed.propagators, replayed.control_matrix,
               replayed.filter_function, replayed.infid)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), f'replay {i} differs'
    # contents may change between replays, addresses may not: another pulse through the same graph
    H2 = eager.H*0.5
    replayed.H.copy_(H2)
    eager.H.copy_(H2)
    eager.launch()
    graph.launch(side.cuda_stream)
    torch.cuda.synchronize(device)
    assert torch.equal(replayed.filter_function, eager.filter_function)
    assert torch.equal(replayed.infid, eager.infid)
    assert not torch.equal(replayed.infid, want[-1])
    replayed.check_status()
    # a failing call inside a capture leaves the stream usable (abort path)
    with pytest.raises(ZeroDivisionError):
        capture(lambda s: 1/0)
    replayed.graph().launch(None)
    torch.cuda.synchronize(device)
    # the ring's one-rank step as a graph (pass + integral) against its eager form, interleaved
    pipes = [make() for _ in range(4)]
    streams = [torch.cuda.Stream(device=device) for _ in range(2)]
    comm = torch.cuda.Stream(device=device)
    ring = ShardedStepRing(pipes, len(omega), omega, S, streams, comm, 1, 0, gather='none',
                           use_graph=True)
    outs = []
    for i in range(24):
        out = ring.step(eager=(i % 5 == 0))
        torch.cuda.synchronize(device)
        outs.append(out.clone())
    assert all(torch.equal(o, outs[0]) for o in outs)           # (step 0 was enqueued call by call)
    assert rel_err(outs[0].cpu().numpy(), want[-1].cpu().numpy()) < TIGHT


@pytest.mark.parametrize('d,n_positions', [(2, 1000), (2, 1025), (3, 600), (4, 300), (4, 200)])
def test_long_resident_concatenations_around_the_one_launch_front(d, n_positions):
    """The one-launch front of a sequence concatenation (sequence_front_kernel: scan over the
    positions in LDS) holds two buffers of one matrix per position: 1024 positions at d = 2, 512 at
    d = 3, 256 at d = 4; beyond that the call must fall back to the gather / scan / Liouville
    launches (round 3: the fuzz sweep found the missing bound as a launch failure).  Either way the
    result equals the route through host tables."""
    import copy
    rng = np.random.default_rng(100*d + n_positions)
    basis = ff.Basis.ggm(d)

    def herm(n):
        M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
        return M + M.conj().transpose(0, 2, 1)
    c_opers, n_opers = herm(2), herm(2)
    omega = np.geomspace(1e-2, 1e1, 130)
    pulses = []
    for k in range(3):
        n_dt = int(rng.integers(1, 4))
        pulses.append(ff.PulseSequence(
            [[c_opers[i], rng.standard_normal(n_dt), f'c{i}'] for i in range(2)],
            [[n_opers[a], np.full(n_dt, 1.0 + a), f'n{a}'] for a in range(2)],
            0.01*rng.random(n_dt) + 0.001, basis))
        pulses[-1].get_filter_function(omega)
        assert pulses[-1]._resident is not None
    index = rng.integers(0, 3, n_positions)
    total = ff.concatenate([pulses[k] for k in index])
    copies = [copy.deepcopy(p) for p in pulses]
    via_host = ff.concatenate([copies[k] for k in index])
    assert rel_err(total.get_filter_function(omega), via_host.get_filter_function(omega)) < 1e-11
    assert rel_err(total.get_control_matrix(omega), via_host.get_control_matrix(omega)) < 1e-11
    assert rel_err(total.total_propagator, via_host.total_propagator) < 1e-11


@pytest.mark.parametrize('n_nops', [1, 3, 4])
def test_block_rule_kernel_with_a_non_hermitian_basis(n_nops):
    """from_atomic_block_kernel<A,4,LCPLX> (one block per 64 frequencies: rule + slab reduction + F)
    with COMPLEX Liouville propagators -- a basis that is not Hermitian -- and 1, 3, 4 noise
    operators, through both routes that reach it (resident control matrices read in place; host
    tables), against the oracle's concatenation rule fed with the same atomic control matrices.
    (For such a basis the rule and the from-scratch evaluation of the long pulse differ in the
    reference itself -- its expansion tr(X C_k) is only a projection for Hermitian C_k -- so the
    from-scratch result is not the yardstick here.)"""
    import copy
    rng = np.random.default_rng(40 + n_nops)
    d = 2
    basis = ff.Basis(np.array([[[0, 1], [0, 0]], [[0, 0], [1, 0]], [[1, 0], [0, 0]], [[0, 0], [0, 1]]],
                              dtype=complex))
    assert not basis.isherm

    def herm(n):
        M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
        return M + M.conj().transpose(0, 2, 1)
    c_opers, n_opers = herm(2), herm(n_nops)
    omega = np.geomspace(1e-2, 1e1, 150)
    pulses = []
    for k in range(3):
        n_dt = int(rng.integers(1, 4))
        pulses.append(ff.PulseSequence(
            [[c_opers[i], rng.standard_normal(n_dt), f'c{i}'] for i in range(2)],
            [[n_opers[a], np.full(n_dt, 1.0 + 0.5*a), f'n{a}'] for a in range(n_nops)],
            0.05*rng.random(n_dt) + 0.01, basis))
        pulses[-1].get_filter_function(omega)
    index = rng.integers(0, 3, 150)
    resident = ff.concatenate([pulses[k] for k in index])
    copies = [copy.deepcopy(p) for p in pulses]
    via_host = ff.concatenate([copies[k] for k in index])
    # the oracle's rule on the same atomic control matrices, cumulative phases and propagators
    R_atomic = np.array([copies[k].get_control_matrix(omega) for k in index])
    phases = np.cumprod([np.exp(1j*omega*copies[k].tau) for k in index[:-1]], axis=0)
    U = np.eye(d, dtype=complex)
    L = []
    for k in index[:-1]:
        U = copies[k].total_propagator @ U
        L.append(orc.liouville_representation(U, np.asarray(basis)))
    R_ref = orc.control_matrix_from_atomic(phases, R_atomic, np.array(L))
    F_ref = orc.filter_function(R_ref)
    assert np.iscomplexobj(np.array(L)) and np.abs(np.array(L).imag).max() > 1e-3
    for got in (resident, via_host):
        assert rel_err(got.get_control_matrix(omega), R_ref) < 1e-11
        assert rel_err(got.get_filter_function(omega), F_ref) < 1e-11


# ---- dimensions above 16: the runtime-d kernels (csrc/generic.hip) ---------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('d,G,A,W,btype', [(24, 3, 2, 9, 'GGM'), (33, 2, 2, 7, 'GGM'), (40, 2, 1, 5, 'GGM'),
                                           (48, 2, 1, 5, 'GGM'), (64, 2, 1, 4, 'Pauli')])
def test_large_d_against_the_oracle(d, G, A, W, btype):
    """Every register-tile size of the generic kernels (d = 17..32, 33..48, 49..64) on seeded random
    pulses, the whole path against the oracle: eigensystem, propagators, control matrix, noise
    operators, filter function, infidelity, Liouville representation (1e-10 relative, north_star)."""
    rng = np.random.default_rng(1000 + d)

    def herm(n):
        M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
        M = (M + M.conj().transpose(0, 2, 1))/2
        return M - np.trace(M, axis1=1, axis2=2)[:, None, None]*np.eye(d)/d
    c_opers, n_opers = herm(2), herm(A)
    c_coeffs, n_coeffs = rng.standard_normal((2, G)), rng.random((A, G))
    dt = 1 - rng.random(G)
    omega = np.concatenate([[-3.0, 0.0, 1e-10], np.geomspace(1e-2/dt.sum(), 1e2/dt.min(), W - 3)])
    basis = ff.Basis.ggm(d) if btype == 'GGM' else ff.Basis.pauli(int(np.log2(d)))
    H = orc.hamiltonian(c_opers, c_coeffs)
    D, V, Q = numeric.diagonalize(H, dt)
    Dr, Vr, Qr = orc.diagonalize(H, dt)
    assert np.abs(D - Dr).max() < 1e-12*np.abs(H).max()*d
    assert rel_err(Q, Qr) < 1e-11
    for k in range(G):
        assert np.abs(V[k].conj().T @ V[k] - np.eye(d)).max() < 1e-12
        assert np.abs(V[k].conj().T @ H[k] @ V[k] - np.diag(D[k])).max() < 1e-11*np.abs(H).max()
    R = numeric.calculate_control_matrix_from_scratch(D, V, Q, omega, basis, n_opers, n_coeffs, dt)
    assert R.shape == (A, d*d, W)
    C = np.asarray(basis)
    # the oracle on every basis element up to d = 40, on every 16th above (its Liouville-space
    # contraction costs d^2 per element: minutes at d = 64); the filter function then through the
    # completeness relation sum_k |R_k|^2 = tr(Y^dag Y)
    sub = np.arange(d*d) if d <= 40 else np.arange(0, d*d, 16)
    R_ref = orc.control_matrix_from_scratch(Dr, Vr, Qr, omega, C[sub], n_opers, n_coeffs, dt)
    assert rel_err(R[:, sub], R_ref) < TOL
    B = numeric.calculate_noise_operators_from_scratch(D, V, Q, omega, n_opers, n_coeffs, dt)
    assert rel_err(np.einsum('oaij,kji->ako', B, C[sub]), R_ref) < TOL
    F = numeric.calculate_filter_function(R)
    F_ref = np.einsum('oaij,obij->abo', B.conj(), B)
    assert rel_err(F, F_ref) < TOL
    if d <= 40:
        assert rel_err(F, orc.filter_function(R_ref)) < TOL
    pulse = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt, basis)
    S = 1e-3/(np.abs(omega) + 1e-2)
    got = ff.infidelity(pulse, S, omega)
    ref = orc.infidelity_from_filter_function(F_ref, S, omega, np.arange(A), d)
    assert rel_err(got, ref) < TOL
    rows = np.arange(0, d*d, max(1, d*d//23))
    L = ff.liouville_representation(Q[-1], basis)
    assert L.shape == (d*d, d*d) and L.dtype == np.float64
    # superoperator.py:51-84 restated for the chosen rows: L[i, j] = tr(U^dag C_i U C_j)
    U = Qr[-1]
    Lr = np.einsum('iab,jba->ij', U.conj().T @ C[rows] @ U, C).real
    assert rel_err(L[rows], Lr) < TOL


@pytest.mark.gpu
def test_large_d_limits_are_reported():
    """Above FFK_MAX_D everything raises; between 17 and 64 the entry points whose kernels are
    compiled per dimension do (and say so), the main path does not."""
    d = 17
    with pytest.raises(ValueError, match='d=65'):
        numeric.diagonalize(np.zeros((2, 65, 65), complex), np.ones(2))
    g = load_golden('rand_d17_ggm')
    with pytest.raises(ValueError, match='cache_intermediates'):
        numeric.calculate_control_matrix_from_scratch(
            g['eigvals'], g['eigvecs'], g['propagators'], g['omega'], g['basis'], g['n_opers'],
            g['n_coeffs'], g['dt'], cache_intermediates=True)
    pulse = pulse_from(g)
    assert pulse.d == d
    with pytest.raises(ValueError):
        pulse.get_filter_function(g['omega'], order=2)


@pytest.mark.gpu
def test_resident_results_are_read_only_views():
    """INTEGRATION.md 'Deviations': F from the one-call routes views pinned memory of the resident
    handle and is read-only (the reference returns a writable array); a copy is an ordinary array and
    integrating it gives the same infidelity."""
    c_opers, c_coeffs, n_opers, n_coeffs, dt, omega = config2_inputs(G=12, W=200, seed=17)
    pulse = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt, ff.Basis.pauli(2))
    F = pulse.get_filter_function(omega)
    assert pulse._resident is not None and not F.flags.writeable
    with pytest.raises(ValueError):
        F *= 2
    G2 = F.copy()
    G2 *= 2
    S = 1e-3/omega
    ref = ff.infidelity(pulse, S, omega)
    assert rel_err(util.integrate(np.einsum('aaw->aw', G2).real*S, omega)/(2*np.pi*4)/2, ref) < 1e-12
    assert not ff.Basis.ggm(3).flags.writeable or True      # (shared default bases: documented, not enforced here)


def test_writable_results_option():
    """``get_filter_function(..., writable=True)``: an owned, writable array as the reference
    returns it (pulse_sequence.py:772-783), memoised by reference, and ``ff.infidelity`` integrates it as the caller
    left it."""
    c_opers, c_coeffs, n_opers, n_coeffs, dt, omega = config2_inputs(G=12, W=200, seed=18)

    def pulse():
        return ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt, ff.Basis.pauli(2))
    S = 1e-3/omega
    p_ro, p_rw = pulse(), pulse()
    F_ro = p_ro.get_filter_function(omega)
    F_rw = p_rw.get_filter_function(omega, writable=True)
    assert F_rw.flags.writeable and F_rw.flags.owndata and F_rw.flags.c_contiguous
    assert np.array_equal(F_ro, F_rw)
    assert p_rw.get_filter_function(omega) is F_rw                      # memoised by reference
    ref = ff.infidelity(p_ro, S, omega)
    assert rel_err(ff.infidelity(p_rw, S, omega), ref) < 1e-13
    F_rw *= 2                                                            # the caller's edit is what gets integrated
    assert rel_err(ff.infidelity(p_rw, S, omega), 2*ref) < 1e-13
    # upgrading an entry that was handed out read-only before
    F2 = p_ro.get_filter_function(omega, writable=True)
    assert F2 is not F_ro and F2.flags.writeable and p_ro.get_filter_function(omega) is F2
    # the module-wide default
    from filter_functions_amd import pulse_sequence as ps
    ps.WRITABLE_RESULTS = True
    try:
        assert pulse().get_filter_function(omega).flags.writeable
    finally:
        ps.WRITABLE_RESULTS = False


_FAULT_SCRIPT = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, {root!r})
import workloads as wl
import filter_functions_amd as ff
from filter_functions_amd import _lib, numeric
from filter_functions_amd.device import DevicePipeline

c_opers, c_coeffs, n_opers, n_coeffs, dt = wl.random_pulse_inputs(**wl.CONFIG2)
omega = wl.random_pulse_omega(dt, 512)
basis = ff.Basis.pauli(2)
seen = []


def expect_fault(name, fn):
    try:
        fn()
    except _lib.FFKKernelFault as exc:
        assert isinstance(exc, RuntimeError) and 'flag wait' in str(exc), exc
        seen.append(name)
    else:
        raise SystemExit(f'{{name}}: no error from a launch whose flag wait ran out')
    word = _lib.ctypes.c_int32(7)
    _lib.check(_lib.load().ffk_kernel_fault_status(_lib.ctypes.byref(word), 0))
    assert word.value == 0, f'{{name}}: the fault word was not cleared by the report'


def pulse():
    return ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt, basis)


# 1. the array call (ffk_control_matrix on host arrays)
p1 = pulse()
p1.diagonalize()
expect_fault('array', lambda: numeric.calculate_control_matrix_from_scratch(
    p1.eigvals, p1.eigvecs, p1.propagators, omega, basis, p1.n_opers, p1.n_coeffs, p1.dt))
# 1b. one, two and five operators: the NC = 1 and NC = 2 blocks' waits (alone, and behind a block of three)
for n_a in (1, 2, 5):
    ops_a = np.concatenate([p1.n_opers, p1.n_opers[::-1]])[:n_a]
    cfs_a = np.concatenate([p1.n_coeffs, p1.n_coeffs[::-1]])[:n_a]
    expect_fault(f'array A={{n_a}}', lambda: numeric.calculate_control_matrix_from_scratch(
        p1.eigvals, p1.eigvecs, p1.propagators, omega, basis, ops_a, cfs_a, p1.dt))
# 2. the resident pass behind PulseSequence.get_filter_function (twice: the second one is the replayed graph)
expect_fault('resident', lambda: pulse().get_filter_function(omega))
expect_fault('resident, second sighting', lambda: pulse().get_filter_function(omega))
expect_fault('resident, replayed', lambda: pulse().get_filter_function(omega))
# 3. the device-pointer pass, call by call and 4. through a captured graph
pipe = DevicePipeline(c_opers, c_coeffs, n_opers, n_coeffs, dt, basis, omega, spectrum=1e-3/omega)
pipe.launch()
expect_fault('_dev', pipe.check_status)
graph = pipe.graph()
_lib.check_kernel_fault()   # (the capture launches nothing: still clean)
graph.launch(None)
expect_fault('captured graph', pipe.check_status)
print('FAULTS SEEN:', ', '.join(seen))
"""


@pytest.mark.gpu
def test_flag_wait_timeout_is_an_error():
    """A flag wait of the d = 4 accumulate kernel that runs out is reported, not returned as numbers
    (VERDICT r4 item 2): a test build of the library whose producers stop publishing tiles
    (-DFFK_PC_FAULT_INJECT, spin limit 64; built by __graft_entry__.build) must raise FFKKernelFault
    (a RuntimeError, C status FFK_EKERNEL) from the array call, the resident pass (enqueued and replayed),
    the device-pointer pass and a captured graph -- and the product build must not.  Reference loop:
    numeric.py:846-869."""
    import os
    import subprocess
    import sys
    root = ROOT
    lib = os.path.join(root, 'build', 'libffk_pcfault.so')
    assert os.path.exists(lib), 'build/libffk_pcfault.so missing: run __graft_entry__.build()'
    env = dict(os.environ, FFK_LIBRARY=lib)
    out = subprocess.run([sys.executable, '-c', _FAULT_SCRIPT.format(root=root)], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert ('FAULTS SEEN: array, array A=1, array A=2, array A=5, resident, resident, second sighting, resident, replayed, '
            '_dev, captured graph') \
        in out.stdout, out.stdout
    # the product build: same calls, no fault, word stays 0
    from filter_functions_amd import _lib
    import workloads as wl
    c_opers, c_coeffs, n_opers, n_coeffs, dt = wl.random_pulse_inputs(**wl.CONFIG2)
    omega = wl.random_pulse_omega(dt, 512)
    pulse = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt,
                             ff.Basis.pauli(2))
    pulse.get_filter_function(omega)
    _lib.check_kernel_fault()


@pytest.mark.gpu
@pytest.mark.parametrize('d,btype', [(17, 'GGM'), (20, 'GGM')])
def test_cumulant_function_and_error_transfer_matrix_above_d16(d, btype):
    """The decay amplitudes -> cumulant function -> error transfer matrix chain above d = 16 (VERDICT r4
    item 9; reference numeric.py:957-1191, 1938-2059 has no dimension limit): the runtime-d control
    matrix feeds the frequency GEMM, the cumulant function's contractions never were compiled per
    dimension.  Against the oracle's matrix form of the cumulant superoperator (pinned to the reference's fixtures
    at d <= 6 in tests/test_oracle_golden.py; the other forms need (d, d, d, d) or N^4 intermediates)."""
    rng = np.random.default_rng(d)
    G, A, W = 5, 2, 40

    def herm(n):
        M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
        M = (M + M.conj().transpose(0, 2, 1))/2
        return M - np.trace(M, axis1=1, axis2=2)[:, None, None]*np.eye(d)/d
    basis = ff.Basis.ggm(d)
    c_opers, n_opers = herm(2), herm(A)
    c_coeffs, n_coeffs = rng.standard_normal((2, G)), rng.random((A, G))
    dt = 1 - 0.5*rng.random(G)
    omega = np.geomspace(1e-2, 30.0, W)
    pulse = ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt, basis)
    S = np.array([1e-3/omega, 2e-3/omega**0.5])
    H = orc.hamiltonian(pulse.c_opers, pulse.c_coeffs)
    D, V, Q = orc.diagonalize(H, dt)
    R_ref = orc.control_matrix_from_scratch(D, V, Q, omega, np.asarray(basis), pulse.n_opers, pulse.n_coeffs, dt)
    gamma_ref = orc.decay_amplitudes(R_ref, S, omega, np.arange(A))
    K_ref = orc.cumulant_function_matrix_form(gamma_ref, np.asarray(basis))
    gamma = numeric.calculate_decay_amplitudes(pulse, S, omega)
    assert rel_err(gamma, gamma_ref) < TOL
    K = numeric.calculate_cumulant_function(pulse, S, omega)
    assert K.shape == K_ref.shape and rel_err(K, K_ref) < TOL
    assert rel_err(numeric.calculate_cumulant_function(pulse, decay_amplitudes=gamma_ref), K_ref) < 1e-12
    U = ff.error_transfer_matrix(pulse, S, omega)
    U_ref = orc.error_transfer_matrix(K_ref)
    assert np.abs(U - U_ref).max() < TOL*np.abs(U_ref - np.eye(len(U_ref))).max() + 1e-15
    # what stays compiled per dimension says so, and says what to call instead
    with pytest.raises(ValueError, match='call them without it'):
        numeric.calculate_control_matrix_from_scratch(pulse.eigvals, pulse.eigvecs, pulse.propagators, omega, basis,
                                                      pulse.n_opers, pulse.n_coeffs, pulse.dt,
                                                      cache_intermediates=True)


# ---------------------------------------------------------------------------------------------
# Host-pointer entry points: every one stages its arrays through the process-wide arena
# ---------------------------------------------------------------------------------------------
def _hostcall_cases(d, G, A, H, W, n_idx=2, T=3, seed=11, basis=None):
    """name -> thunk that runs one host-pointer entry point of libffk on fixed random inputs and returns its outputs.
    The inputs only have the right shapes and dtypes (no kernel's control flow depends on values), which is all that
    staging can get wrong; `slow` marks the entry points of ffk_api_frozen.hip."""
    lib = _lib.load()
    rng = np.random.default_rng(seed)
    p = _lib.ptr
    N = d*d
    basis = np.ascontiguousarray(ff.Basis.ggm(d) if basis is None else basis, dtype=complex)

    def c128(*shape):
        return rng.standard_normal(shape) + 1j*rng.standard_normal(shape)

    def herm(n):
        M = c128(n, d, d)
        return np.ascontiguousarray(M + M.conj().transpose(0, 2, 1))

    def run(fn, outputs, *args):
        _lib.check(fn(*args))
        return outputs

    Hm, n_opers, c_opers = herm(G), herm(A), herm(H)
    dt = rng.random(G) + 0.2
    t = np.concatenate(([0.0], np.cumsum(dt)))
    D = np.ascontiguousarray(rng.standard_normal((G, d)))
    V, Q = c128(G, d, d)/d, c128(G + 1, d, d)/d
    omega = np.sort(rng.random(W))*20 + 1e-2
    n_coeffs, ratio = rng.random((A, G)) + 0.1, rng.random((A, H, G))
    idx = np.arange(n_idx, dtype=np.int32)[::-1].copy()
    spectra = {1: c128(W), 2: c128(n_idx, W), 3: c128(n_idx, n_idx, W)}
    n_out = {1: n_idx, 2: n_idx, 3: n_idx*n_idx}
    R, F, F2 = c128(A, N, W), c128(A, A, W), c128(A, A, N, N, W)
    index = rng.integers(0, T, G).astype(np.int32)
    phases, table, U = c128(T, W), c128(T, A, N, W), c128(T, d, d)/d
    L = np.ascontiguousarray(rng.standard_normal((max(G - 1, 1), N, N))/N)
    pulse_args = (p(D), p(V), p(Q), p(omega), W, p(basis), N, p(n_opers), A, p(n_coeffs), p(dt), p(t), G, d)
    no_basis = pulse_args[:5] + pulse_args[7:]
    grad_args = (*no_basis[:8], p(c_opers), H)
    cases, slow = {}, set()

    def diagonalize():
        o = np.empty((G, d)), np.empty((G, d, d), complex), np.empty((G + 1, d, d), complex)
        return run(lib.ffk_diagonalize, o, p(Hm), p(dt), G, d, *map(p, o))
    cases['diagonalize'] = diagonalize

    def control_matrix(flags):
        o = np.empty((A, N, W), complex), (np.empty((W, A, d, d), complex) if flags else None)
        return run(lib.ffk_control_matrix, o, *pulse_args, flags, *map(p, o))
    cases['control_matrix'] = lambda: control_matrix(0)
    cases['control_matrix+noise_operators'] = lambda: control_matrix(_lib.WANT_NOISE_OPERATORS)

    def intermediates():
        o = [np.empty(s, complex) for s in ((A, G, d, d), (G, d, d), (G, N, d, d), (G, W), (G, W, d, d), (G, A, N, W))]
        return run(lib.ffk_control_matrix_intermediates, o, *pulse_args, *map(p, o))
    cases['control_matrix_intermediates'] = intermediates

    def noise_intermediates():
        o = [np.empty(s, complex) for s in ((A, G, d, d), (G, W), (G, W, d, d), (G, W, A, d, d))]
        return run(lib.ffk_noise_operators_intermediates, o, *no_basis, *map(p, o))
    cases['noise_operators_intermediates'] = noise_intermediates

    def filter_function(which):
        o = [np.empty((A, A, N, N, W) if which else (A, A, W), complex)]
        return run(lib.ffk_filter_function, o, p(R), A, N, W, which, p(o[0]))
    weights = c128(N, N)

    def filter_function_weighted():
        o = [np.empty((A, A, W), complex)]
        return run(lib.ffk_filter_function_weighted, o, p(R), A, N, W, p(weights), 0.5, p(o[0]))
    cases['filter_function_weighted'] = filter_function_weighted

    def infidelity(nd):
        o = [np.empty(n_out[nd])]
        return run(lib.ffk_infidelity, o, p(F), A, W, p(spectra[nd]), nd, p(omega), p(idx), n_idx, d, p(o[0]))

    def liouville():
        o = [np.empty((T, N, N))]
        return run(lib.ffk_liouville, o, p(U), T, d, p(basis), N, 1, p(o[0]))
    cases['liouville'] = liouville

    step_phases, atomic = c128(max(G - 1, 1), W), c128(G, A, N, W)

    def from_atomic(which, g):
        o = [np.empty((g, A, N, W) if which else (A, N, W), complex)]
        return run(lib.ffk_control_matrix_from_atomic, o, p(step_phases) if g > 1 else None, p(atomic),
                   p(L) if g > 1 else None, 0, g, A, N, W, which, p(o[0]))

    def from_atomic_indexed(which):
        o = [np.empty((G, A, N, W) if which else (A, N, W), complex)]
        return run(lib.ffk_control_matrix_from_atomic_indexed, o, p(phases), p(table), p(index), p(L), 0, T, G, A, N,
                   W, which, p(o[0]))

    def concatenate_sequence(which):
        o = [np.empty((G, A, N, W) if which else (A, N, W), complex), np.empty((d, d), complex),
             np.empty((max(G - 1, 1), N, N)), None if which else np.empty((A, A, W), complex)]
        return run(lib.ffk_concatenate_sequence, o, p(U), p(phases), p(table), p(index), p(basis), 1, T, G, d, A, N, W,
                   which, *map(p, o))

    def periodic():
        o = [np.empty((A, N, W), complex)]
        return run(lib.ffk_control_matrix_periodic, o, p(phases), p(R), p(L), 0, 5, A, N, W, p(o[0]))
    cases['control_matrix_periodic'] = periodic
    B_atomic, props = c128(G, W, A, d, d), c128(max(G - 1, 1), d, d)/d

    def noise_operators_from_atomic(g):
        o = [np.empty((W, A, d, d), complex)]
        return run(lib.ffk_noise_operators_from_atomic, o, p(step_phases) if g > 1 else None, p(B_atomic),
                   p(props) if g > 1 else None, g, W, A, d, p(o[0]))
    for g in (G, 1):
        cases[f'control_matrix_from_atomic G={g}'] = lambda g=g: from_atomic(0, g)
        cases[f'noise_operators_from_atomic G={g}'] = lambda g=g: noise_operators_from_atomic(g)

    def decay_amplitudes(nd):
        o = [np.empty((T, T, n_out[nd], N, N))]
        return run(lib.ffk_decay_amplitudes, o, p(table), T, A, N, W, p(spectra[nd]), nd, p(omega), p(idx), n_idx,
                   p(o[0]))
    gamma = np.ascontiguousarray(rng.standard_normal((T, N, N)))

    def cumulant_function():
        o = [np.empty((T, N, N))]
        return run(lib.ffk_cumulant_function, o, p(gamma), T, N, d, p(basis), 0, p(o[0]))
    cases['cumulant_function'] = cumulant_function
    pauli, gamma_1q = np.ascontiguousarray(ff.Basis.pauli(1), dtype=complex), rng.standard_normal((T, 4, 4))

    def cumulant_function_single_qubit():        # a workspace of zero bytes
        o = [np.empty((T, 4, 4))]
        return run(lib.ffk_cumulant_function, o, p(gamma_1q), T, 4, 2, p(pauli), 1, p(o[0]))
    cases['cumulant_function single qubit'] = cumulant_function_single_qubit

    def expm_real():
        o = [np.empty((N, N))]
        return run(lib.ffk_expm_real, o, p(gamma), N, p(o[0]))
    cases['expm_real'] = expm_real

    # ---- ffk_api_frozen.hip
    def second_order():
        o = [np.empty((A, A, N, N, W), complex)]
        return run(lib.ffk_second_order_filter_function, o, *pulse_args, p(o[0]))

    def shifts_from_scratch(nd):
        o = [np.empty((A, A, N, N, W), complex), np.empty((n_out[nd], N, N))]
        return run(lib.ffk_frequency_shifts_from_scratch, o, *pulse_args, p(spectra[nd]), nd, p(idx), n_idx,
                   *map(p, o))
    F_atomic, R_step = c128(G, A, A, N, N, W), c128(G, A, N, W)

    def second_order_from_atomic():
        o = [np.empty((A, A, N, N, W), complex)]
        return run(lib.ffk_second_order_filter_function_from_atomic, o, p(F_atomic), p(R_step), p(L), G, A, N, W,
                   p(o[0]))

    def frequency_shifts(nd):
        o = [np.empty((n_out[nd], N, N))]
        return run(lib.ffk_frequency_shifts, o, p(F2), A, N, W, p(spectra[nd]), nd, p(omega), p(idx), n_idx, p(o[0]))

    def cumulant_second_order():                  # adds to the array it is given
        o = [gamma + 1.0]
        return run(lib.ffk_cumulant_function_second_order, o, p(gamma), T, N, d, p(basis), p(o[0]))
    grad_spectra = {1: c128(W), 2: c128(A, W)}

    def derivative(nd, with_ratio, want_dF=True):
        o = [np.empty((A, G, H, W)) if want_dF else None, np.empty((A, G, H)) if nd else None]
        return run(lib.ffk_filter_function_derivative, o, *grad_args, p(ratio) if with_ratio else None, p(dt), p(t), G,
                   d, p(grad_spectra[nd]) if nd else None, nd, *map(p, o))

    def control_matrix_derivative():
        o = [np.empty((H, W, G, A, N), complex)]
        return run(lib.ffk_control_matrix_derivative, o, *pulse_args[:10], p(c_opers), H, p(ratio), p(dt), p(t), G, d,
                   p(o[0]))
    dR = c128(H, W, G, A, N)

    def derivative_from_control_matrix():
        o = [np.empty((A, G, H, W))]
        return run(lib.ffk_filter_function_derivative_from_control_matrix, o, p(R), p(dR), A, N, W, G, H, p(o[0]))

    for which in (0, 1):
        cases[f'filter_function which={which}'] = lambda w=which: filter_function(w)
        cases[f'control_matrix_from_atomic which={which}'] = lambda w=which: from_atomic(w, G)
        cases[f'control_matrix_from_atomic_indexed which={which}'] = lambda w=which: from_atomic_indexed(w)
        cases[f'concatenate_sequence which={which}'] = lambda w=which: concatenate_sequence(w)
    for nd in (1, 2, 3):
        cases[f'infidelity s_ndim={nd}'] = lambda nd=nd: infidelity(nd)
        cases[f'decay_amplitudes s_ndim={nd}'] = lambda nd=nd: decay_amplitudes(nd)
        cases[f'frequency_shifts_from_scratch s_ndim={nd}'] = lambda nd=nd: shifts_from_scratch(nd)
        cases[f'frequency_shifts s_ndim={nd}'] = lambda nd=nd: frequency_shifts(nd)
    cases.update({
        'second_order_filter_function': second_order, 'second_order_filter_function_from_atomic': second_order_from_atomic,
        'cumulant_function_second_order': cumulant_second_order,
        'filter_function_derivative': lambda: derivative(0, True),
        'infidelity_derivative s_ndim=1': lambda: derivative(1, False),
        'infidelity_derivative s_ndim=2': lambda: derivative(2, True),
        'infidelity_derivative alone': lambda: derivative(2, True, want_dF=False),
        'control_matrix_derivative': control_matrix_derivative,
        'filter_function_derivative_from_control_matrix': derivative_from_control_matrix})
    frozen = ('frequency_shifts', 'second_order', 'cumulant_function_second_order', 'derivative')
    slow = {name for name in cases if any(key in name for key in frozen)}
    if d > 8:
        cases = {k: v for k, v in cases.items() if 'derivative' not in k}       # the gradient kernels: d <= 8
    inputs = dict(D=D, V=V, Q=Q, omega=omega, n_opers=n_opers, n_coeffs=n_coeffs, c_opers=c_opers, ratio=ratio, dt=dt,
                  t=t, basis=basis, idx=idx, spectra=spectra, grad_spectra=grad_spectra)
    return cases, slow, inputs


def _same_bits(got, ref):
    return all((a is None and b is None) or a.tobytes() == b.tobytes() for a, b in zip(got, ref))


_HOSTCALL_SHAPE = dict(d=3, G=4, A=2, H=2, W=33)       # N = 9 (GGM), W no multiple of a wavefront
_hostcall_memo = {}


def _hostcall_reference():
    """The cases at _HOSTCALL_SHAPE and, computed once, the result of each directly after ffk_release_arena()."""
    if not _hostcall_memo:
        cases, slow, inputs = _hostcall_cases(**_HOSTCALL_SHAPE)
        _hostcall_memo.update(cases=cases, slow=slow, inputs=inputs, fresh={})
    return _hostcall_memo


def _fresh_result(name):
    memo = _hostcall_reference()
    if name not in memo['fresh']:
        _lib.check(_lib.load().ffk_release_arena())
        memo['fresh'][name] = [None if o is None else o.copy() for o in memo['cases'][name]()]
    return memo['fresh'][name]


def _grow_arena():
    """A call that leaves the arena far larger than any case at _HOSTCALL_SHAPE needs (7 x 2 MiB)."""
    M = np.zeros((512, 512))
    _lib.check(_lib.load().ffk_expm_real(_lib.ptr(M), 512, _lib.ptr(np.empty_like(M))))


def _check_arena_history(names):
    memo = _hostcall_reference()
    assert names
    for name in names:
        fresh = _fresh_result(name)
        _grow_arena()
        grown = memo['cases'][name]()
        assert all(o is None or np.isfinite(o).all() for o in fresh), name
        assert _same_bits(grown, fresh), f'{name}: the result depends on what the arena held before'


def test_host_pointer_results_do_not_depend_on_the_arenas_history():
    """Each host-pointer entry point of ffk_api.hip and ffk_api_sequence.hip, once on a freshly released arena (the
    reservation is then barely larger than the call's own need, so arrays whose sizes were under-counted overlap)
    and once on an arena that a larger call has grown: bit-identical outputs."""
    memo = _hostcall_reference()
    _check_arena_history([n for n in memo['cases'] if n not in memo['slow']])


@pytest.mark.slow
def test_frozen_host_pointer_results_do_not_depend_on_the_arenas_history():
    """... and those of ffk_api_frozen.hip: second order, frequency shifts, gradients."""
    memo = _hostcall_reference()
    _check_arena_history(sorted(memo['slow']))


def _dev_buffers(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _dptr(tensor):
    return None if tensor is None else tensor.data_ptr()


@pytest.mark.slow
@pytest.mark.parametrize('s_ndim', [1, 2, 3])
def test_host_second_order_call_equals_its_device_pointer_twin(s_ndim):
    """ffk_frequency_shifts_from_scratch against ffk_second_order_filter_function_dev followed by
    ffk_frequency_shifts_shard_dev on the whole grid, each with a workspace of exactly the queried size."""
    import torch
    lib, memo = _lib.load(), _hostcall_reference()
    i, sh = memo['inputs'], _HOSTCALL_SHAPE
    d, G, A, W = sh['d'], sh['G'], sh['A'], sh['W']
    N, n_idx = d*d, len(i['idx'])
    n_out = n_idx*n_idx if s_ndim == 3 else n_idx
    host = _fresh_result(f'frequency_shifts_from_scratch s_ndim={s_ndim}')
    D, V, Q, om, basis, nop, nc, dt, t, S, idx = _dev_buffers(
        i['D'], i['V'], i['Q'], i['omega'], i['basis'], i['n_opers'], i['n_coeffs'], i['dt'], i['t'],
        i['spectra'][s_ndim], i['idx'])
    F2 = torch.empty((A, A, N, N, W), dtype=torch.complex128, device='cuda')
    shifts = torch.empty((n_out, N, N), dtype=torch.float64, device='cuda')
    wsb = lib.ffk_second_order_workspace_bytes(W, N, A, G, d)
    swsb = lib.ffk_frequency_shifts_workspace_bytes(W, n_idx, s_ndim)
    assert wsb > 0 and swsb > 0
    ws, sws = (torch.empty(n, dtype=torch.uint8, device='cuda') for n in (wsb, swsb))
    _lib.check(lib.ffk_second_order_filter_function_dev(
        *map(_dptr, (D, V, Q, om)), W, _dptr(basis), N, _dptr(nop), A, *map(_dptr, (nc, dt, t)), G, d, _dptr(F2),
        _dptr(ws), wsb, None))
    _lib.check(lib.ffk_frequency_shifts_shard_dev(_dptr(F2), A, N, W, _dptr(S), s_ndim, _dptr(om), W, 0, _dptr(idx),
                                                  n_idx, _dptr(shifts), _dptr(sws), swsb, None))
    torch.cuda.synchronize()
    assert _same_bits([F2.cpu().numpy(), shifts.cpu().numpy()], host)


@pytest.mark.slow
@pytest.mark.parametrize('s_ndim', [1, 2])
def test_host_gradient_call_equals_its_device_pointer_twin(s_ndim):
    """ffk_filter_function_derivative (filter function and infidelity derivative) against
    ffk_filter_function_derivative_shard_dev on the whole grid with a workspace of exactly the queried size."""
    import torch
    lib, memo = _lib.load(), _hostcall_reference()
    i, sh = memo['inputs'], _HOSTCALL_SHAPE
    d, G, A, H, W = sh['d'], sh['G'], sh['A'], sh['H'], sh['W']
    with_ratio = s_ndim == 2
    host = _fresh_result(f'infidelity_derivative s_ndim={s_ndim}')
    D, V, Q, om, nop, nc, cop, ratio, dt, t, S = _dev_buffers(
        i['D'], i['V'], i['Q'], i['omega'], i['n_opers'], i['n_coeffs'], i['c_opers'],
        i['ratio'] if with_ratio else None, i['dt'], i['t'], i['grad_spectra'][s_ndim])
    dF = torch.empty((A, G, H, W), dtype=torch.float64, device='cuda')
    dI = torch.empty((A, G, H), dtype=torch.float64, device='cuda')
    wsb = lib.ffk_filter_function_derivative_workspace_bytes(W, A, H, G, d)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device='cuda')
    _lib.check(lib.ffk_filter_function_derivative_shard_dev(
        *map(_dptr, (D, V, Q, om)), W, _dptr(nop), A, _dptr(nc), _dptr(cop), H, _dptr(ratio), _dptr(dt), _dptr(t), G,
        d, _dptr(S), s_ndim, _dptr(om), W, 0, _dptr(dF), _dptr(dI), _dptr(ws), wsb, None))
    torch.cuda.synchronize()
    _lib.check_kernel_fault()
    assert _same_bits([dF.cpu().numpy(), dI.cpu().numpy()], host)


def test_host_pointer_calls_work_after_a_rejected_call():
    """A host-pointer call that fails its argument check (FFK_EINVAL) leaves the arena usable: the same entry point
    with good arguments then gives the result it gives on a fresh arena.  One entry point of ffk_api.hip, one of
    ffk_api_sequence.hip."""
    lib, memo = _lib.load(), _hostcall_reference()
    sh = _HOSTCALL_SHAPE
    A, N, W = sh['A'], sh['d']**2, sh['W']
    R, out = np.ones((A, N, W), complex), np.empty((A, A, W), complex)
    ref_F = _fresh_result('filter_function which=0')
    ref_R = _fresh_result('control_matrix_periodic')
    with pytest.raises(ValueError):
        _lib.check(lib.ffk_filter_function(_lib.ptr(R), A, N, W, 7, _lib.ptr(out)))             # invalid `which`
    assert _same_bits(memo['cases']['filter_function which=0'](), ref_F)
    with pytest.raises(ValueError):
        _lib.check(lib.ffk_control_matrix_periodic(_lib.ptr(R[0, 0]), _lib.ptr(R), _lib.ptr(np.eye(N)), 0, 0, A, N, W,
                                                   _lib.ptr(np.empty_like(R))))                 # repeats < 1
    assert _same_bits(memo['cases']['control_matrix_periodic'](), ref_R)


@pytest.mark.slow
def test_frozen_host_pointer_calls_work_after_a_rejected_call():
    """... and one of ffk_api_frozen.hip: the gradient asked for an infidelity derivative without a spectrum."""
    lib, memo = _lib.load(), _hostcall_reference()
    ref = _fresh_result('infidelity_derivative s_ndim=2')
    i, sh = memo['inputs'], _HOSTCALL_SHAPE
    d, G, A, H, W = sh['d'], sh['G'], sh['A'], sh['H'], sh['W']
    p = _lib.ptr
    with pytest.raises(ValueError):
        _lib.check(lib.ffk_filter_function_derivative(
            p(i['D']), p(i['V']), p(i['Q']), p(i['omega']), W, p(i['n_opers']), A, p(i['n_coeffs']), p(i['c_opers']), H,
            None, p(i['dt']), p(i['t']), G, d, None, 2, None, p(np.empty((A, G, H)))))
    assert _same_bits(memo['cases']['infidelity_derivative s_ndim=2'](), ref)

"""The front end of every pass -- Hamiltonian sum, Jacobi eigensolver, segment propagator, cumulative products -- on
structured Hamiltonians, against the long-double yardstick of front_yardstick.py (no eigensolver in the reference:
exp(-i H dt) by scaled Taylor series from the FP64 input; eigensystems judged by orthonormality, residual, eigenvalues
and order, never against reference eigenvectors).

Routes:  (a) numeric.diagonalize            eigh_expm_kernel / eigh_expm_generic_kernel + three-phase scan
         (b) ResidentResult.evaluate(H)     the pass on a summed Hamiltonian (fused front while <= 64 chunks)
         (c) ... with controls              eigh_expm_controls_kernel sums H itself
         (d) ff.get_filter_functions        eigh_expm_controls_pulses_kernel, scan_local_pulses_kernel

Bars (front_yardstick.py): the project's own from test_diagonalize, test_gpu_parity.py (TIGHT) and
test_sequences_gpu.py (LONG).  Every test prints its measured worst before it asserts.
"""
import functools

import numpy as np
import pytest

import filter_functions_amd as ff
import front_yardstick as fy
from filter_functions_amd import batch, numeric
from filter_functions_amd._resident import ResidentResult

pytestmark = pytest.mark.gpu

OMEGA = np.array([0.3, 1.7])          # W = 2: the grid only has to exist
SMALL = list(range(2, 17))
LARGE = [17, 24, 33, 64]              # csrc/generic.hip


# ---- inputs and routes ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stack(d):
    """All families of dimension d as one pulse, with the yardstick's segment propagators (computed once per d)."""
    names, H, dt = fy.family_stack(d)
    P = fy.expm_ld(H, dt)
    for a in (H, dt, P):
        a.flags.writeable = False
    return names, H, dt, P


@functools.lru_cache(maxsize=None)
def grid(d):
    """Basis (GGM) and one noise operator for the routes that run a whole pass."""
    basis = ff.Basis.ggm(d)
    n_oper = np.diag(np.r_[1.0, -1.0, np.zeros(d - 2)]).astype(complex)[None]
    return basis, n_oper


def times(dt):
    return np.concatenate([[0.0], np.cumsum(dt)])


def route_a(H, dt):
    return numeric.diagonalize(H, dt)


def route_b(H, dt):
    basis, n_oper = grid(H.shape[-1])
    res = ResidentResult()
    D, V, Q, _ = res.evaluate(H, dt, times(dt), OMEGA, np.asarray(basis), n_oper, np.ones((1, len(dt))))
    return D.copy(), V.copy(), Q.copy()


def route_c(H, dt):
    """Controls = the segments' own matrices, amplitudes = the identity: the device sums exactly H[g] (products with 0
    and 1, sums with 0)."""
    basis, n_oper = grid(H.shape[-1])
    res = ResidentResult()
    D, V, Q, _ = res.evaluate(H, dt, times(dt), OMEGA, np.asarray(basis), n_oper, np.ones((1, len(dt))),
                              c_coeffs=np.eye(len(dt)))
    return D.copy(), V.copy(), Q.copy()


def pulses_from_controls(c_opers, c_coeffs, dt, orders):
    """One pulse per row order of the same controls (the sum is exact in every order)."""
    d = c_opers.shape[-1]
    basis, n_oper = grid(d)
    names = np.array([f'A_{i}' for i in range(len(c_opers))])
    return [ff.PulseSequence.from_arrays(c_opers[o], names[o], c_coeffs[o], n_oper, ['B_0'], np.ones((1, len(dt))),
                                         dt, basis) for o in orders]


def route_d(H, dt, n_pulses=3, c_opers=None, c_coeffs=None):
    """ff.get_filter_functions on pulses built from the same controls in different row orders; returns one (D, V, Q)
    per pulse."""
    if c_opers is None:
        c_opers, c_coeffs = H, np.eye(len(dt))
    n = len(c_opers)
    orders = [np.arange(n), np.arange(n)[::-1], np.roll(np.arange(n), n//2)][:n_pulses]
    pulses = pulses_from_controls(np.asarray(c_opers), c_coeffs, dt, orders)
    ff.get_filter_functions(pulses, OMEGA)
    assert all(isinstance(p._resident, batch._Member) for p in pulses)       # the batched pass really ran
    return [(p.eigvals, p.eigvecs, p.propagators) for p in pulses]


# ---- checks --------------------------------------------------------------------------------------------------------
def front_figures(H, dt, P, D, V, Q):
    """Per segment (orthonormality, residual, eigenvalues, one-step propagator error) and whether D ascends."""
    G, d = H.shape[:2]
    assert D.shape == (G, d) and V.shape == (G, d, d) and Q.shape == (G + 1, d, d)
    Ql = np.asarray(Q).astype(fy.CLD)
    step = np.abs(Ql[1:] - P @ Ql[:-1]).max(axis=(1, 2)).astype(float)
    fig, asc = np.empty((G, 4)), np.empty(G, dtype=bool)
    for g in range(G):
        o, r, e, asc[g] = fy.eigen_errors(H[g], D[g], V[g])
        fig[g] = o, r, e, step[g]
    return fig, asc


BARS = np.array([fy.ORTHO, fy.RESIDUAL, fy.EIGVALS, fy.TIGHT])


def assert_front(label, names, H, dt, P, D, V, Q):
    fig, asc = front_figures(H, dt, P, D, V, Q)
    worst = fig.max(axis=0)
    print(f'{label}: orthonormality {worst[0]:.2e} ({names[fig[:, 0].argmax()]})  residual {worst[1]:.2e} '
          f'({names[fig[:, 1].argmax()]})  eigenvalues {worst[2]:.2e} ({names[fig[:, 2].argmax()]})  '
          f'step {worst[3]:.2e} ({names[fig[:, 3].argmax()]})')
    assert np.array_equal(Q[0], np.eye(H.shape[-1])), label                 # to the last bit
    for g, name in enumerate(names):
        assert asc[g], (label, name, 'eigenvalues not ascending')
        assert np.all(fig[g] < BARS), (label, name, dict(zip(('ortho', 'residual', 'eigvals', 'step'), fig[g])))
    return worst


# ---- eigensystem and segment propagator on every family --------------------------------------------------------------
@pytest.mark.parametrize('d', SMALL)
@pytest.mark.parametrize('route', ['a', 'b', 'c'])
def test_families_single_pulse(route, d):
    names, H, dt, P = stack(d)
    D, V, Q = {'a': route_a, 'b': route_b, 'c': route_c}[route](H, dt)
    assert_front(f'route ({route}) d={d}', names, H, dt, P, D, V, Q)


@pytest.mark.parametrize('d', SMALL)
def test_families_batched_pulses(d):
    names, H, dt, P = stack(d)
    for k, (D, V, Q) in enumerate(route_d(H, dt)):
        assert_front(f'route (d) d={d} pulse {k}', names, H, dt, P, D, V, Q)


@pytest.mark.parametrize('d', LARGE)
def test_families_generic_dimensions(d):
    """d > 16 (eigh_expm_generic_kernel, prefix_generic_kernel): numeric.diagonalize and PulseSequence.diagonalize."""
    names, H, dt, P = stack(d)
    D, V, Q = route_a(H, dt)
    assert_front(f'route (a) d={d}', names, H, dt, P, D, V, Q)
    pulse = pulses_from_controls(H, np.eye(len(dt)), dt, [np.arange(len(dt))[::-1]])[0]
    pulse.diagonalize()
    assert np.array_equal(pulse.eigvals, D) and np.array_equal(pulse.eigvecs, V)
    assert np.array_equal(pulse.propagators, Q)


@pytest.mark.parametrize('d', SMALL + LARGE)
def test_lower_triangle_only(d):
    """Garbage in the upper triangle and in the diagonal's imaginary part: the same bits as the clean call."""
    names, H, dt, _ = stack(d)
    rng = np.random.default_rng(d)
    upper = np.triu(np.ones((d, d), dtype=bool), 1)
    dirty = H.copy()
    dirty[:, upper] = 1e3*(rng.standard_normal((len(H), upper.sum())) + 1j*rng.standard_normal((len(H), upper.sum())))
    dirty[:, np.arange(d), np.arange(d)] += 1j*rng.standard_normal((len(H), d))
    assert np.array_equal(fy.hermitian_from_lower(dirty), H)
    clean, got = route_a(H, dt), route_a(dirty, dt)
    for name, x, y in zip(('eigvals', 'eigvecs', 'propagators'), clean, got):
        assert np.array_equal(x, y), (d, name, np.abs(x - y).max())


# ---- the scan against the long-double product ------------------------------------------------------------------------
LENGTHS = [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049]


@functools.lru_cache(maxsize=None)
def long_pulse(d):
    """Dense random H[g] = sum_i c_i(g) A_i of the longest length for d, rotation angles theta <= 2, with the yardstick's
    cumulative products.  Operators on a 2^-30 grid and amplitudes on a 2^-4 grid: the FP64 sum is exact in any order,
    so the array routes and the route that sums on the device see the same H.  Every shorter length is a prefix."""
    G = 1025 if d == 16 else 2049        # (yardstick: 1.7 s for 1025 products at d = 16, 0.8 s for 2049 at d = 9)
    rng = np.random.default_rng(77 + d)
    c_opers = np.stack([np.round(fy.dense(d, rng)*2**30)/2**30 for _ in range(3)])
    c_coeffs = np.round(rng.uniform(-2, 2, (3, G))*16)/16
    H = np.einsum('ijk,il->ljk', c_opers, c_coeffs)
    exact = np.einsum('ijk,il->ljk', c_opers.astype(fy.CLD), c_coeffs.astype(fy.LD))
    assert np.array_equal(H.astype(fy.CLD), exact)
    theta = rng.uniform(0.05, 2.0, G)
    dt = fy.segment_lengths(H, theta)
    Q = fy.cumulative_ld(H, dt)
    scale = np.abs(Q).max(axis=(1, 2))
    for a in (c_opers, c_coeffs, H, dt, Q, scale):
        a.flags.writeable = False
    return c_opers, c_coeffs, H, dt, Q, scale


@pytest.mark.parametrize('d', [2, 3, 4, 5, 8, 9, 16])
@pytest.mark.parametrize('route', ['a', 'b', 'd'])
def test_scan_against_long_double_product(route, d):
    """The whole Q (G+1, d, d) against cumulative_ld, relative error per segment index, and unitarity of every Q[g]; bar
    TIGHT below 500 segments, LONG from 500 on.  The lengths straddle the chunks of 8 and 16, the grouped d <= 4 path
    with a partial last group, 64 chunks (the fused front's limit) and chunk_length's steps at 64, 256 and 1024."""
    c_opers, c_coeffs, H_all, dt_all, Q_all, scale = long_pulse(d)
    eye = np.eye(d)
    figures, failures = [], []
    for G in [g for g in LENGTHS if g <= len(dt_all)]:
        H, dt = np.ascontiguousarray(H_all[:G]), np.ascontiguousarray(dt_all[:G])
        if route == 'a':
            results = [route_a(H, dt)]
        elif route == 'b':
            results = [route_b(H, dt)]
        else:
            results = route_d(H, dt, 2, c_opers, np.ascontiguousarray(c_coeffs[:, :G]))
        bar = fy.TIGHT if G < 500 else fy.LONG
        for _, _, Q in results:
            assert Q.shape == (G + 1, d, d) and np.array_equal(Q[0], eye)
            err = (np.abs(Q.astype(fy.CLD) - Q_all[:G + 1]).max(axis=(1, 2))/scale[:G + 1]).astype(float)
            unit = float(np.abs(Q.conj().transpose(0, 2, 1) @ Q - eye).max())
            figures.append((G, err.max(), int(err.argmax()), unit))
            if not (err.max() < bar and unit < bar):
                failures.append((G, float(err.max()), int(err.argmax()), unit, bar))
    for G, e, at, u in figures:
        print(f'route ({route}) d={d} G={G}: cumulative {e:.2e} (at {at})  unitarity {u:.2e}')
    below = [f for f in figures if f[0] < 500]
    above = [f for f in figures if f[0] >= 500]
    print(f'route ({route}) d={d}: worst below 500 segments {max(f[1] for f in below):.2e}, '
          f'from 500 on {max(f[1] for f in above):.2e}')
    assert not failures, failures


# ---- inputs out of range: raise or be right ----------------------------------------------------------------------------
POWERS = [-600, -540, -500, -300, 300, 490, 510]


def scaled_inputs(d, k):
    fam = fy.families(d, np.random.default_rng(5000 + d))
    names = ['dense', 'double_levels_rotated', 'diagonal_weakly_coupled']
    H = np.stack([np.ldexp(fam[n].real, k) + 1j*np.ldexp(fam[n].imag, k) for n in names])      # exact
    return names, H, fy.segment_lengths(H, (1.0, 0.25, 0.5))


@pytest.mark.parametrize('d', [2, 4, 9])
@pytest.mark.parametrize('route', ['a', 'b', 'd'])
def test_scaled_by_powers_of_two_raises_or_is_right(route, d):
    """H 2^k far outside the usual range: every segment meets the bars relative to its own scale, or the call raises
    LinAlgError.  A finite answer that misses the bars is a failure (squares of the entries that underflow to zero
    look like convergence to the Jacobi iteration)."""
    failures = []
    for k in POWERS:
        names, H, dt = scaled_inputs(d, k)
        P = fy.expm_ld(H, dt)
        try:
            if route == 'a':
                results = [route_a(H, dt)]
            elif route == 'b':
                results = [route_b(H, dt)]
            else:
                results = route_d(H, dt, 2)
        except np.linalg.LinAlgError:
            print(f'route ({route}) d={d} 2^{k}: LinAlgError')
            continue
        for D, V, Q in results:
            fig, asc = front_figures(H, dt, P, D, V, Q)
            worst = fig.max(axis=0)
            print(f'route ({route}) d={d} 2^{k}: orthonormality {worst[0]:.2e} residual {worst[1]:.2e} '
                  f'eigenvalues {worst[2]:.2e} step {worst[3]:.2e} ascending {bool(asc.all())}')
            if not (np.all(fig < BARS) and asc.all() and np.all(np.isfinite(Q))):
                failures.append((k, worst.tolist(), bool(asc.all())))
    assert not failures, failures


def infinite_inputs(d):
    base = np.diag(np.arange(1.0, d + 1)).astype(complex)
    off = base.copy()
    off[1, 0] = off[0, 1] = np.inf
    neg = base.copy()
    neg[d - 1, 0] = neg[0, d - 1] = -np.inf
    diag = base.copy()
    diag[d - 1, d - 1] = np.inf
    return {'+Inf off the diagonal': off, '-Inf off the diagonal': neg, 'Inf on the diagonal': diag}, base


@pytest.mark.parametrize('d', [2, 4, 9])
@pytest.mark.parametrize('route', ['a', 'b', 'd'])
def test_infinite_entries_raise(route, d):
    """One infinite entry in an otherwise diagonal H raises LinAlgError as NaN does.  One-segment pulses: the control
    sum of the batched route is 1 x H, no 0 x Inf."""
    bad, base = infinite_inputs(d)
    dt = np.array([0.5])
    outcome = {}
    for name, H in bad.items():
        try:
            if route == 'a':
                D = route_a(H[None], dt)[0]
            elif route == 'b':
                D = route_b(H[None], dt)[0]
            else:
                pulses = [pulses_from_controls(M[None], np.ones((1, 1)), dt, [np.arange(1)])[0] for M in (H, base)]
                ff.get_filter_functions(pulses, OMEGA)
                D = pulses[0].eigvals
            outcome[name] = f'no error, eigenvalues {np.asarray(D)[0]}'
        except np.linalg.LinAlgError:
            outcome[name] = 'LinAlgError'
    print(f'route ({route}) d={d}:', outcome)
    assert all(v == 'LinAlgError' for v in outcome.values()), outcome

"""The front end's yardstick, checked on the host: expm_ld against mpmath at 50 digits, NumPy's own eigh + eigen-expm
against the bars that test_front_exact_gpu.py sets for the device (the bars are reachable by a backward-stable FP64
solver on every family), and the families against the structure they are named for."""
import numpy as np
import pytest

import front_yardstick as fy

DIMS = list(range(2, 17))


def _mpf(mp, x):
    """A long double as an mpf, exactly: its FP64 head and tail."""
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - fy.LD(hi)))


@pytest.mark.parametrize('d', [2, 3, 4, 7, 16])
def test_yardstick_against_mpmath(d):
    """expm_ld vs mpmath.expm at 50 digits on every family, with the segment lengths the GPU test uses (theta = 0.25, 1,
    0) and with theta = 0.7 and 2 (the scan test's largest): max abs error <= 1e-16."""
    mp = pytest.importorskip('mpmath')
    names, H, dt = fy.family_stack(d)
    worst = 0.0
    with mp.workdps(50):
        # (d = 16 costs 6 s per set of segment lengths in mpmath: the second set up to d = 7)
        for thetas in ((fy.THETAS, (0.7, 2.0)) if d <= 7 else (fy.THETAS,)):
            dts = fy.segment_lengths(H, thetas)
            got = fy.expm_ld(H, dts)
            for g, name in enumerate(names):
                A = mp.matrix(d, d)
                for i in range(d):
                    for j in range(d):
                        h = H[g, i, j]
                        A[i, j] = mp.mpc(0, -1)*mp.mpc(float(h.real), float(h.imag))*mp.mpf(float(dts[g]))
                ref = mp.expm(A, method='taylor')
                err = max(abs(mp.mpc(_mpf(mp, got[g, i, j].real), _mpf(mp, got[g, i, j].imag)) - ref[i, j])
                          for i in range(d) for j in range(d))
                worst = max(worst, float(err))
                assert err <= 1e-16, (name, thetas, float(err))
    print(f'd={d}: expm_ld vs mpmath, worst abs error {worst:.2e}')


def test_cumulative_is_the_left_to_right_product():
    rng = np.random.default_rng(3)
    H = np.stack([fy.dense(3, rng) for _ in range(5)])
    dt = fy.segment_lengths(H, (0.5, 2.0))
    Q = fy.cumulative_ld(H, dt)
    P = fy.expm_ld(H, dt)
    assert Q.dtype == fy.CLD and Q.shape == (6, 3, 3)
    assert np.array_equal(Q[0], np.eye(3))
    assert np.array_equal(Q[3], P[2] @ (P[1] @ P[0]))
    assert np.abs(Q[5].conj().T @ Q[5] - np.eye(3)).max() < 1e-16


def test_eigen_errors_see_a_wrong_eigensystem():
    """The yardstick's own sensitivity: an exact eigensystem scores ~eps, a perturbed one scores the perturbation --
    also on a matrix of scale 1e-12 (no floor on the scale) and on the zero matrix."""
    rng = np.random.default_rng(4)
    for scale in (1.0, 1e-12, 1e12):
        H = fy.dense(5, rng)*scale
        D, V = np.linalg.eigh(H)
        o, r, e, asc = fy.eigen_errors(H, D, V)
        assert o < 1e-14 and r < 1e-14 and e < 1e-14 and asc
        Vbad = V.copy()
        Vbad[:, 1] += 1e-9*V[:, 2]
        assert fy.eigen_errors(H, D, Vbad)[0] > 5e-10 and fy.eigen_errors(H, D, Vbad)[1] > 1e-11
        Dbad = D.copy()
        Dbad[3] += 1e-9*scale
        assert fy.eigen_errors(H, Dbad, V)[2] > 1e-10
        assert not fy.eigen_errors(H, D[::-1], V[:, ::-1])[3]
    Z = np.zeros((3, 3), dtype=complex)
    assert fy.eigen_errors(Z, np.zeros(3), np.eye(3)) == (0.0, 0.0, 0.0, True)
    assert fy.eigen_errors(Z, np.array([0, 0, 1e-300]), np.eye(3))[2] == float('inf')
    H = fy.dense(4, rng)
    U = fy.hermitian_from_lower(np.tril(H) + np.triu(np.full((4, 4), 7.0), 1) + 3j*np.eye(4))
    assert np.array_equal(U, H)


@pytest.mark.parametrize('d', DIMS)
def test_numpy_reference_meets_the_gpu_bars(d):
    """numpy.linalg.eigh and V exp(-i D dt) V^dag on every family through the checks of the GPU test: the bars ask
    nothing of the device that LAPACK in FP64 does not deliver on the same inputs."""
    names, H, dt = fy.family_stack(d)
    worst = np.zeros(4)
    Q = np.eye(d, dtype=complex)
    for g, name in enumerate(names):
        D, V = np.linalg.eigh(H[g])
        o, r, e, asc = fy.eigen_errors(H[g], D, V)
        Qn = (V*np.exp(-1j*dt[g]*D)) @ V.conj().T @ Q
        s = fy.step_error(H[g], dt[g], Q, Qn)
        Q = Qn
        worst = np.maximum(worst, (o, r, e, s))
        assert asc, name
        assert o < fy.ORTHO and r < fy.RESIDUAL and e < fy.EIGVALS and s < fy.TIGHT, (name, o, r, e, s)
    print(f'd={d}: numpy worst orthonormality {worst[0]:.1e} residual {worst[1]:.1e} eigenvalues {worst[2]:.1e} '
          f'step {worst[3]:.1e}')


@pytest.mark.parametrize('d', DIMS + [17, 33])
def test_families_keep_their_structure(d):
    names, H, dt = fy.family_stack(d)
    fam = dict(zip(names, H))
    k = np.arange(d)
    assert len(fam) == (18 if d in (4, 8, 16) else 17)
    assert np.array_equal(H, H.conj().transpose(0, 2, 1))                      # exactly Hermitian
    ev = {name: np.linalg.eigvalsh(M) for name, M in fam.items()}
    off = {name: np.abs(M - np.diag(np.diagonal(M))).max() for name, M in fam.items()}
    assert off['dense'] > 0.1 and np.abs(fam['dense'].imag).max() > 0.1
    assert not fam['zero'].any()
    assert np.array_equal(fam['identity'], fam['identity'][0, 0]*np.eye(d)) and fam['identity'][0, 0] != 0
    diag = np.diagonal(fam['diagonal_descending']).real
    assert off['diagonal_descending'] == 0 and np.all(np.diff(diag) < 0)
    assert np.ptp(ev['equal_levels_rotated']) < 1e-12 and ev['equal_levels_rotated'][0] > 0.5
    if d > 2:
        assert off['equal_levels_rotated'] > 0                                  # (dense at rounding level)
    pairs = ev['double_levels_rotated']
    assert np.abs(pairs[1::2] - pairs[:2*(d//2):2]).max() < 1e-12 and (d == 2 or off['double_levels_rotated'] > 1e-3)
    if d > 3:
        assert np.all(np.diff(pairs[::2]) > 0.5)
    close = ev['close_levels_rotated']
    assert np.abs(close - (1 + 1e-9*k)).max() < 1e-12 and off['close_levels_rotated'] > 1e-12
    r1 = ev['rank_one']
    assert np.abs(r1[:-1]).max() < 1e-12*r1[-1] and r1[-1] > 0.1
    weak = fam['diagonal_weakly_coupled']
    assert np.abs(np.diagonal(weak).real - k).max() < 1e-9 and 1e-12 < off['diagonal_weakly_coupled'] < 1e-9
    hop = fam['hopping']
    assert np.array_equal(hop, np.diag(np.ones(d - 1), 1) + np.diag(np.ones(d - 1), -1))
    im = fam['imaginary_offdiagonal']
    assert not im.real.any() and np.array_equal(np.abs(im.imag), 1 - np.eye(d)) and np.all(np.tril(im.imag, -1) >= 0)
    assert np.array_equal(fam['all_ones'], np.ones((d, d)))
    assert np.array_equal(fam['wilkinson'], hop + np.diag(np.abs(k - (d - 1)/2)))
    graded = np.abs(fam['graded'])
    assert graded[-1, -1]/graded[0, 0] > 1e6 and off['graded'] > 1e-3
    assert 1e-13 < np.abs(fam['dense_1e-12']).max() < 1e-11 and 1e11 < np.abs(fam['dense_1e12']).max() < 1e13
    a = d//2
    blk = fam['block_diagonal']
    assert not blk[:a, a:].any() and not blk[a:, :a].any() and (d < 4 or (off['block_diagonal'] > 1e-3))
    if 'pauli_exchange' in fam:
        P = fam['pauli_exchange']
        assert np.array_equal(P.real, np.round(P.real)) and np.array_equal(P.imag, np.round(P.imag))
        levels = ev['pauli_exchange']
        assert np.sum(np.diff(levels) > 1e-12*np.abs(levels).max()) + 1 <= d/2    # multiplets
        assert np.sum(np.diff(levels) < 1e-12*np.abs(levels).max()) >= d/2
    # segment lengths: rotation angles 0.25, 1, 0 in turn, dt = 1 on the zero matrix
    norm = np.abs(H).sum(axis=1).max(axis=1)
    angle = dt*norm
    assert dt[names.index('zero')] == 1.0 and np.all(dt >= 0) and np.all(np.isfinite(dt))
    want = np.resize(fy.THETAS, len(dt))
    assert np.allclose(np.delete(angle, names.index('zero')), np.delete(want, names.index('zero')), rtol=1e-14)
    assert (dt == 0).sum() >= 5

"""Extended-precision yardstick for the front end of a pass (eigensolver, segment propagators, cumulative
products): NumPy long double only, no device, no oracle.  Used by test_front_exact_host.py (which checks the
yardstick itself against mpmath) and test_front_exact_gpu.py.

Nothing here compares eigenvectors with reference eigenvectors: their gauge is free.  An eigensystem is judged by
what it must satisfy (orthonormality, residual, eigenvalues, order), a propagator by exp(-i H dt) evaluated from
the FP64 Hamiltonian without any eigensolver.
"""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble

# The project's bars, shared by the host and the GPU test
ORTHO = 1e-13         # max|V^dag V - 1|                       (test_diagonalize)
RESIDUAL = 2e-13      # max|V^dag H V - diag D| / max|H|       (test_diagonalize)
EIGVALS = 1e-13       # max|D - eigvalsh(H)| / max|H|          (test_diagonalize)
TIGHT = 2e-13         # one propagator step; cumulative products of fewer than 500 segments
LONG = 1e-12          # cumulative products of 500 segments or more

THETAS = (0.25, 1.0, 0.0)


def hermitian_from_lower(H):
    """What the device reads: the lower triangle, the diagonal's real part."""
    H = np.asarray(H)
    L = np.tril(H, -1)
    return L + L.conj().swapaxes(-1, -2) + np.real(np.diagonal(H, axis1=-2, axis2=-1))[..., None]*np.eye(H.shape[-1])


def expm_ld(H, dt):
    """exp(-i H dt) in clongdouble from FP64 *H* (..., d, d) and *dt* (...): Taylor series of 24 terms after
    scaling by a power of two to a 1-norm of at most 2^-4 (truncation (2^-4)^25/25! ~ 5e-56), then repeated
    squaring.  Accurate to ~2^s d eps_ld with s squarings: keep ||H dt||_1 of order one."""
    H = np.asarray(H)
    d = H.shape[-1]
    dt = np.broadcast_to(np.asarray(dt, dtype=LD), H.shape[:-2])
    A = CLD(-1j)*H.astype(CLD)*dt[..., None, None]
    norm = np.abs(A).sum(axis=-2).max(axis=-1)
    if not np.all(np.isfinite(norm)):
        raise ValueError('expm_ld: non-finite input')
    s = np.zeros(norm.shape, dtype=np.int64)
    nz = norm > 0
    s[nz] = np.maximum(0, np.ceil(np.log2(norm[nz].astype(np.float64))).astype(np.int64) + 4)
    s[norm*np.ldexp(LD(1), -s) > LD(2)**-4] += 1          # (log2 rounded in FP64: make sure)
    A = A*np.ldexp(LD(1), -s)[..., None, None]            # exact
    eye = np.broadcast_to(np.eye(d, dtype=CLD), A.shape)
    E, term = eye.copy(), eye.copy()
    for k in range(1, 25):
        term = term @ A/LD(k)
        E = E + term
    for i in range(int(s.max()) if s.size else 0):
        E = np.where((i < s)[..., None, None], E @ E, E)
    return E


def cumulative_ld(H, dt):
    """Q[0] = 1, Q[g+1] = expm_ld(H[g], dt[g]) Q[g], multiplied strictly left to right in clongdouble: (G+1, d, d)."""
    P = expm_ld(H, dt)
    G, d = P.shape[0], P.shape[-1]
    Q = np.empty((G + 1, d, d), dtype=CLD)
    Q[0] = np.eye(d, dtype=CLD)
    for g in range(G):
        Q[g + 1] = P[g] @ Q[g]
    return Q


def _over(num, scale):
    """num/scale; where the scale is zero every error must be zero too."""
    if scale > 0:
        return float(num/scale)
    return 0.0 if num == 0 else float('inf')


def eigen_errors(H, D, V):
    """(orthonormality, residual/scale, eigenvalue error/scale, ascending) of the eigensystem (D, V) of the Hermitian
    (d, d) matrix *H*, evaluated in long double with scale = max|H| (no floor: a tiny matrix is judged on its own
    scale).  The eigenvalues are compared with numpy.linalg.eigvalsh of H/scale (LAPACK, itself good to a few eps)."""
    H = np.asarray(H)
    d = H.shape[-1]
    Hl, Vl, Dl = H.astype(CLD), np.asarray(V).astype(CLD), np.asarray(D).astype(LD)
    scale = LD(np.abs(H).max())
    Vh = Vl.conj().T
    ortho = float(np.abs(Vh @ Vl - np.eye(d, dtype=CLD)).max())
    residual = _over(np.abs(Vh @ Hl @ Vl - np.diag(Dl)).max(), scale)
    # (H/scale by an exact power of two: LAPACK never sees a subnormal or an overflowing intermediate)
    e = int(np.frexp(np.float64(scale))[1]) if scale > 0 else 0
    ref = np.ldexp(np.linalg.eigvalsh(np.ldexp(H.real, -e) + 1j*np.ldexp(H.imag, -e)).astype(LD), e)
    eigvals = _over(np.abs(Dl - ref).max(), scale)
    return ortho, residual, eigvals, bool(np.all(np.diff(np.asarray(D)) >= 0))


def step_error(H_g, dt_g, Q_prev, Q_next):
    """max|Q[g+1] - exp(-i H_g dt_g) Q[g]| with the device's own Q[g]: one segment's propagator on its own."""
    return float(np.abs(np.asarray(Q_next).astype(CLD) - expm_ld(H_g, dt_g) @ np.asarray(Q_prev).astype(CLD)).max())


def segment_lengths(H, thetas=THETAS):
    """dt_g = theta_g/||H_g||_1 with theta cycling through *thetas* (a zero-length segment among them), dt = 1 where
    H = 0: the rotation angle ||H dt||_1 stays of order one whatever the scale of H, where expm_ld is accurate."""
    H = np.asarray(H)
    norm = np.abs(H).sum(axis=-2).max(axis=-1)
    theta = np.resize(np.asarray(thetas, dtype=np.float64), len(H))
    with np.errstate(divide='ignore', invalid='ignore'):
        dt = theta/norm
    dt[norm == 0] = 1.0
    return dt


# ---- matrix families -----------------------------------------------------------------------------------------------
def dense(d, rng):
    M = rng.standard_normal((d, d)) + 1j*rng.standard_normal((d, d))
    return (M + M.conj().T)/2


def random_unitary(d, rng):
    Q, R = np.linalg.qr(rng.standard_normal((d, d)) + 1j*rng.standard_normal((d, d)))
    return Q*(np.diagonal(R)/np.abs(np.diagonal(R)))


def rotated(levels, rng):
    """U diag(levels) U^dag with a random unitary, exactly Hermitian."""
    U = random_unitary(len(levels), rng)
    M = (U*np.asarray(levels, dtype=np.float64)) @ U.conj().T
    return (M + M.conj().T)/2


def hopping(d):
    return np.diag(np.ones(d - 1), 1) + np.diag(np.ones(d - 1), -1) + 0j


_PAULI = (np.array([[0, 1], [1, 0]], dtype=complex), np.array([[0, -1j], [1j, 0]]),
          np.array([[1, 0], [0, -1]], dtype=complex))


def pauli_exchange(n, rng):
    """sum_{j<k} c_jk (X_j X_k + Y_j Y_k + Z_j Z_k) on n qubits with integer c_jk in 1..3: entries are exact small
    integers, and the SU(2) symmetry makes every total-spin multiplet exactly degenerate."""
    def string(op, j, k):
        out = np.eye(1, dtype=complex)
        for q in range(n):
            out = np.kron(out, op if q in (j, k) else np.eye(2))
        return out
    H = np.zeros((2**n, 2**n), dtype=complex)
    for j in range(n):
        for k in range(j + 1, n):
            c = int(rng.integers(1, 4))
            for op in _PAULI:
                H += c*string(op, j, k)
    return H


def families(d, rng):
    """Hermitian d x d matrices by name, in a fixed order: what a control Hamiltonian looks like and a dense random
    matrix does not.  test_front_exact_host.py asserts that each has the property it is named for."""
    k = np.arange(d)
    grade = 10.0**np.linspace(-4, 4, d)
    a = d//2
    block = np.zeros((d, d), dtype=complex)
    block[:a, :a], block[a:, a:] = dense(a, rng), dense(d - a, rng)
    imag = 1j*(np.tril(np.ones((d, d)), -1) - np.triu(np.ones((d, d)), 1))
    v = rng.standard_normal(d) + 1j*rng.standard_normal(d)
    rank_one = np.outer(v, v.conj())
    fam = {
        'dense': dense(d, rng),
        'zero': np.zeros((d, d), dtype=complex),
        'identity': 1.5*np.eye(d, dtype=complex),
        'diagonal_descending': np.diag(0.37*(d - k)) + 0j,
        'equal_levels_rotated': rotated(np.full(d, 0.8), rng),
        'double_levels_rotated': rotated((k//2).astype(float) - 1.0, rng),
        'close_levels_rotated': rotated(1 + 1e-9*k, rng),
        'rank_one': (rank_one + rank_one.conj().T)/2,
        'diagonal_weakly_coupled': np.diag(k.astype(float)) + 1e-10*dense(d, rng),
        'hopping': hopping(d),
        'imaginary_offdiagonal': imag,
        'all_ones': np.ones((d, d), dtype=complex),
        'wilkinson': hopping(d) + np.diag(np.abs(k - (d - 1)/2)),
        'graded': dense(d, rng)*np.sqrt(np.outer(grade, grade)),
        'dense_1e-12': dense(d, rng)*1e-12,
        'dense_1e12': dense(d, rng)*1e12,
        'block_diagonal': block,
    }
    if d in (4, 8, 16):
        fam['pauli_exchange'] = pauli_exchange(int(np.log2(d)), rng)
    return fam


def family_stack(d, seed=0):
    """(names, H (G, d, d), dt (G,)) of all families of dimension d as the G segments of one pulse."""
    fam = families(d, np.random.default_rng(1000*d + seed))
    H = np.ascontiguousarray(np.stack(list(fam.values())), dtype=np.complex128)
    return list(fam), H, segment_lengths(H)

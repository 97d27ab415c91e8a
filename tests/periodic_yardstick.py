"""Yardsticks of the periodic-driving tests (test helper, no test in here).

``closed_form_control_matrix`` is the closed form of filter_functions_amd/periodic.py written in NumPy, term for
term as DESIGN.md section 7.15 states it; ``series_control_matrices_mp`` sums the series of n periods term by term
at 60 digits, with the SAME rounded product fl(w T) as every route of the package uses and the exact matrix powers
of the propagator it is handed.
"""
import numpy as np


def eigensystem(U):
    """Unitary V and eigenphases phi of a unitary U through the complex Schur form (unitary whatever coincides)."""
    from scipy.linalg import schur
    T, V = schur(np.asarray(U, dtype=complex), output='complex')
    return V, np.angle(np.diag(T))


def rotated(R1, basis, V):
    """X'[a, j, k, w] = (V^dag (sum_l R1[a, l, w] C_l) V)[j, k]."""
    C = np.asarray(basis)
    Cp = np.einsum('ji,ljk,km->lim', V.conj(), C, V)
    return np.einsum('alw,ljk->ajkw', np.asarray(R1), Cp), Cp


def reduced_angles(omega, T, phi):
    """theta[j, k, w] = fl(w T) - (phi_j - phi_k), reduced to [-pi, pi]."""
    theta = (np.asarray(omega, dtype=float)*T)[None, None, :] - (phi[:, None] - phi[None, :])[:, :, None]
    return theta - 2*np.pi*np.round(theta/(2*np.pi))


def dirichlet(theta, n):
    """s = sum_{g<n} e^{i g theta} = e^{i (n-1) theta/2} sin(n theta/2)/sin(theta/2); n where the sine vanishes."""
    half = 0.5*theta
    den = np.sin(half)
    safe = np.where(den == 0.0, 1.0, den)
    ratio = np.where(den == 0.0, float(n), np.sin(n*half)/safe)
    return np.exp(1j*(n - 1)*half)*ratio


def closed_form_control_matrix(R1, basis, U, T, omega, n):
    """R_n (A, N, W) of n periods from one period's control matrix R1, its total propagator U and duration T."""
    V, phi = eigensystem(U)
    X, Cp = rotated(R1, basis, V)
    Xn = X*dirichlet(reduced_angles(omega, T, phi), n)[None]
    # R_n[a, l] = tr(C_l V X'_n V^dag) = sum_jk C'_l[k, j] X'_n[j, k]
    return np.einsum('lkj,ajkw->alw', Cp, Xn)


def closed_form_filter_function(R1, basis, U, T, omega, n):
    """F_n[a, w] = sum_jk |X'[j, k]|^2 sin^2(n theta_jk/2)/sin^2(theta_jk/2)."""
    V, phi = eigensystem(U)
    X, _ = rotated(R1, basis, V)
    return np.einsum('ajkw,jkw->aw', np.abs(X)**2, np.abs(dirichlet(reduced_angles(omega, T, phi), n))**2)


_BITS = 220          # fixed point behind the binary point: 66 digits, six more than the phase factors carry


def _fixed(x):
    """Array of doubles -> array of Python integers, x 2^_BITS (exact for |x| >= 2^-167)."""
    from fractions import Fraction
    flat = [int(Fraction(float(v))*(1 << _BITS)) for v in np.ravel(x)]
    out = np.empty(len(flat), dtype=object)
    out[:] = flat
    return out.reshape(np.shape(x))


def series_control_matrices_mp(R1, basis, U, T, omega, repeats, dps=60):
    """{n: R_n (A, N, W) complex128} for every n of *repeats*: one walk over the terms
    X_g = e^{i w T} U^dag X_{g-1} U, X_0 = sum_l R1[l] C_l, summed term by term, R_n[l] = tr(C_l sum_{g<n} X_g) -- the
    propagator's exact matrix powers.  The phase factor e^{i fl(w T)} comes from mpmath at *dps* digits; U, the basis
    and R1 (doubles) are taken as exact; the products and sums run in 220-bit fixed point on Python integers (the
    same arithmetic as mpmath's at a tenth of its cost: the terms are bounded by |X_0|, nothing can overflow or lose
    more than 2^-220 per operation).  Rounded to double once, at the end."""
    import mpmath as mp
    R1 = np.asarray(R1, dtype=complex)
    C = np.asarray(basis, dtype=complex)
    U = np.asarray(U, dtype=complex)
    A, N, W = R1.shape
    d = U.shape[0]
    one = 1 << _BITS
    with mp.workdps(dps):
        z = [mp.expj(mp.mpf(float(np.float64(w)*np.float64(T)))) for w in omega]      # the rounded product
        zr = np.array([int(mp.floor(v.real*one + mp.mpf(0.5))) for v in z], dtype=object)[:, None]
        zi = np.array([int(mp.floor(v.imag*one + mp.mpf(0.5))) for v in z], dtype=object)[:, None]
    Ur, Ui, Cr, Ci = _fixed(U.real), _fixed(U.imag), _fixed(C.real), _fixed(C.imag)
    Rr, Ri = _fixed(R1.real.transpose(2, 0, 1)), _fixed(R1.imag.transpose(2, 0, 1))       # (W, A, N)

    def cmul(ar, ai, br, bi):
        return (ar*br - ai*bi) >> _BITS, (ar*bi + ai*br) >> _BITS

    # X_0[j][k]: arrays (W, A)
    xr = [[0*Rr[:, :, 0] for _ in range(d)] for _ in range(d)]
    xi = [[0*Rr[:, :, 0] for _ in range(d)] for _ in range(d)]
    for l in range(N):
        for j in range(d):
            for k in range(d):
                pr, pi = cmul(Rr[:, :, l], Ri[:, :, l], Cr[l, j, k], Ci[l, j, k])
                xr[j][k], xi[j][k] = xr[j][k] + pr, xi[j][k] + pi
    tr, ti = [row[:] for row in xr], [row[:] for row in xi]
    wanted = sorted(int(n) for n in repeats)
    out = {}
    for g in range(1, wanted[-1] + 1):
        if g in wanted:
            Rn = np.zeros((A, N, W), dtype=complex)
            scale = float(one)
            for l in range(N):
                accr, acci = 0*tr[0][0], 0*tr[0][0]
                for j in range(d):
                    for k in range(d):          # tr(C_l X) = sum_jk C_l[k, j] X[j, k]
                        pr, pi = cmul(tr[j][k], ti[j][k], Cr[l, k, j], Ci[l, k, j])
                        accr, acci = accr + pr, acci + pi
                re = np.array([[int(v)/scale for v in row] for row in accr])
                im = np.array([[int(v)/scale for v in row] for row in acci])
                Rn[:, l, :] = (re + 1j*im).T
            out[g] = Rn
        if g == wanted[-1]:
            break
        # Y = X U, then X' = z U^dag Y
        yr = [[None]*d for _ in range(d)]
        yi = [[None]*d for _ in range(d)]
        for j in range(d):
            for k in range(d):
                accr, acci = 0, 0
                for m in range(d):
                    pr, pi = cmul(xr[j][m], xi[j][m], Ur[m, k], Ui[m, k])
                    accr, acci = accr + pr, acci + pi
                yr[j][k], yi[j][k] = accr, acci
        for j in range(d):
            for k in range(d):
                accr, acci = 0, 0
                for m in range(d):
                    pr, pi = cmul(yr[m][k], yi[m][k], Ur[m, j], -Ui[m, j])
                    accr, acci = accr + pr, acci + pi
                xr[j][k], xi[j][k] = cmul(accr, acci, zr, zi)
                tr[j][k], ti[j][k] = tr[j][k] + xr[j][k], ti[j][k] + xi[j][k]
    return out


def filter_function_of(R):
    """Diagonal fidelity filter function (A, W) of a control matrix (A, N, W)."""
    return (np.abs(np.asarray(R))**2).sum(axis=1)

"""Yardsticks of the second-order periodic-driving tests (test helper, no test in here).

``sequential_frequency_shifts`` builds the frequency shifts of n periods ONE PERIOD AT A TIME -- n - 1 steps (m, 1)
of the integrated concatenation rule --, in the operator basis and without the propagator's
eigensystem: the control matrix of m periods by the first-order rule R_{m+1} = R_m + e^{i w m T} R_1 Q_m, the
Liouville matrix Q_{m+1} = Q_m Q_1 and the phase e^{i w (m+1) T} = e^{i w m T} e^{i w T} by running products.  A
different order of steps and different operands from the device's doubling in the eigenbasis; with *extended* all of
it runs in ``np.longdouble`` (where that is wider than the double).

``doubling_frequency_shifts`` is the device's algorithm in NumPy: the steps of a plan, both operands element-wise in
the eigenbasis, term for term as periodic_batch.hip states them.
"""
import numpy as np

import periodic_yardstick as yard

EXTENDED = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def trapezoid_weights(spectrum, omega, n_idx, real=np.float64):
    """c[a, w] = S_a(w) x trapezoid weight / 2 pi, (n_idx, W), for a real spectrum of one or two dimensions."""
    omega = np.asarray(omega, dtype=real)
    w = np.zeros(len(omega), dtype=real)
    w[:-1] += np.diff(omega)/2
    w[1:] += np.diff(omega)/2
    S = np.broadcast_to(np.asarray(spectrum).real.astype(real), (n_idx, len(omega)))
    return S*w/(8*np.arctan(real(1)))                                  # (2 pi in the working format)


def liouville(U, basis, cplx=np.complex128):
    """Q[i, j] = Re tr(U^dag C_i U C_j)."""
    U, C = np.asarray(U, dtype=cplx), np.asarray(basis, dtype=cplx)
    return np.einsum('ba,ibc,cd,jda->ij', U.conj(), C, U, C).real


def sequential_frequency_shifts(R1, basis, U, T, omega, spectrum, delta1, repeats, extended=False):
    """{n: Delta_n (n_idx, N, N) float64} for every n of *repeats*, from one period's control matrix R1 (n_idx, N, W)
    -- the rows of the selected noise operators --, its total propagator U, its duration T and its own frequency
    shifts *delta1* (n_idx, N, N), one period at a time:

        Delta_{m+1} = Delta_m + Q_m^T Delta_1 Q_m + X,
        X[k, l] = sum_w c_w Re( conj( e^{i w m T} (R_1 Q_m)[k, w] ) R_m[l, w] ).
    """
    real, cplx = (np.longdouble, np.clongdouble) if extended else (np.float64, np.complex128)
    R1 = np.asarray(R1, dtype=cplx)
    n_idx = len(R1)
    c = trapezoid_weights(spectrum, omega, n_idx, real)
    Q1 = liouville(U, basis, cplx).astype(real)
    x = (np.asarray(omega, dtype=np.float64)*np.float64(T)).astype(real)          # fl(w T), as every route forms it
    z = np.exp(1j*x.astype(cplx))
    D1 = np.asarray(delta1, dtype=real)
    Rm, Qm, zm, D = R1.copy(), Q1.copy(), z.copy(), D1.copy()
    wanted = {int(n) for n in repeats}
    out = {}
    if 1 in wanted:
        out[1] = D.astype(np.float64)
    for m in range(1, max(wanted)):
        step = zm[None, None, :]*np.einsum('akw,kl->alw', R1, Qm.astype(cplx))
        X = np.einsum('aw,akw,alw->akl', c.astype(cplx), step.conj(), Rm).real
        D = D + Qm.T @ D1 @ Qm + X
        Rm, Qm, zm = Rm + step, Qm @ Q1, zm*z
        if m + 1 in wanted:
            out[m + 1] = D.astype(np.float64)
    return out


def doubling_frequency_shifts(R1, basis, U, T, omega, spectrum, delta1, steps, count_slots):
    """The device's walk in NumPy (complex128): *steps* (S, 4) and *count_slots* (K,) of
    ``periodic_second_order.step_plan``; the rows (K, n_idx, N, N) of the counts."""
    R1 = np.asarray(R1, dtype=complex)
    n_idx = len(R1)
    c = trapezoid_weights(spectrum, omega, n_idx)
    V, phi = yard.eigensystem(U)
    X1, Cp = yard.rotated(R1, basis, V)                                # X'[a, j, k, w], C'_l[j, k]
    theta = yard.reduced_angles(omega, T, phi)                         # (d, d, W)
    dphi = phi[:, None] - phi[None, :]
    table = [np.asarray(delta1, dtype=float)]
    for m, mp, slot_m, slot_mp in np.asarray(steps).reshape(-1, 4):
        m, mp = int(m), int(mp)
        B = X1*yard.dirichlet(theta, m)[None]
        A = X1*(yard.dirichlet(theta, mp)*np.exp(1j*m*theta))[None]
        M = np.einsum('aw,ajkw,auvw->ajkuv', c, A.conj(), B)           # M[e = (j, k), f = (u, v)]
        # E[(j, k), l] = C'_l[k, j]
        X = np.einsum('lkj,ajkuv,nvu->aln', Cp.conj(), M, Cp).real
        Q = np.einsum('ab,iab,jba->ij', np.exp(-1j*m*dphi), Cp, Cp).real
        table.append(table[slot_m] + np.einsum('pk,apq,ql->akl', Q, table[slot_mp], Q) + X)
    return np.stack([table[s] for s in count_slots])

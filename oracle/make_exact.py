"""Generate tests/golden/gradient_exact.npz: gradients of the filter function and of the control matrix from
the DEFINITIONS, in 60-digit arithmetic, at and next to the degeneracies where the closed forms of the
nested integral J (gradient kernels, ff_oracle.filter_function_derivative, the upstream reference) lose digits.

TEST INFRASTRUCTURE, CPU only, needs mpmath (imported inside the functions that use it, so that the input
recipes below can be imported without it).

    python oracle/make_exact.py

The reference shares nothing with the closed forms of J except the first-order integral I1:

    per segment   H = sum_h c_h A_h = V D V^dag (mp.eighe),  T = V^dag Q
    Y_a(w)       += e^{i w t_g} T^dag (V^dag (n_a B_a) V o I1) T,  I1[m][n] = (e^{i x dt} - 1)/(i x), x = w + D_m - D_n
    Q            <- V e^{-i D dt} V^dag Q
    F_a(w)        = sum_ij |Y_ij|^2  (orthonormal basis),   R_ak(w) = tr(Y_a C_k)
    dF, dR        = central differences in c_coeffs[h, s], step 1e-20 (checked against step 1e-18)

The file also holds a table of J itself (x, b and the exact value) for the host test of ffk_math.h's
derivative_integral.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
OUT = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'gradient_exact.npz')

DPS = 60
STEP, STEP_CHECK = '1e-20', '1e-18'
G, A = 4, 2
# a negative frequency, 0, |w dt| < 2 and > 2 for every dt in [0.2, 1.2], one above 30
OMEGA = np.array([-3.1, -0.4, 0.0, 0.013, 0.9, 4.7, 11.0, 37.0])
NEAR_IDLE_EPS = (1e-2, 1e-3, 1e-4, 1e-6, 1e-9, 1e-12, 1e-15)
CROSSING_DELTA = (1e-3, 1e-6, 1e-9, 1e-12)
RESONANCE_EPS = (0.0, 2.0**-50, 1e-12, 1e-9, 1e-6, 1e-4)
J_DT = 0.37
SEEDS = dict(exact=9100, near_idle=9200, crossing=9300, near_resonant=9400)


# ---- inputs: NumPy only -------------------------------------------------------------------------------------------
def _herm(rng, n, d):
    M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
    return (M + M.conj().transpose(0, 2, 1))/2


def _ggm(d):
    import ff_oracle as orc
    return np.asarray(orc.basis_ggm(d), dtype=complex)


def _common(rng, d, H):
    return dict(n_opers=_herm(rng, A, d), n_coeffs=rng.random((A, G)) + 0.1, dt=rng.random(G) + 0.2,
                omega=OMEGA.copy(), basis=_ggm(d), c_ids=np.array([f'c{h}' for h in range(H)]))


def case_inputs(family, d, param=None):
    """The inputs of one case, float64 / complex128.  Cases of one family and d differ in `param` alone."""
    rng = np.random.default_rng(SEEDS[family] + d)
    if family in ('exact', 'near_idle'):
        c_opers, c_coeffs = _herm(rng, 2, d), rng.standard_normal((2, G))
        c_coeffs[:, 1] = 0.0 if family == 'exact' else param*np.array([1.0, -0.7])
        return dict(c_opers=c_opers, c_coeffs=c_coeffs, **_common(rng, d, 2))
    if family == 'crossing':
        # segment 1: K0 + delta K1, K0 with one doubly degenerate level that K1 splits; a third control at 0
        U = np.linalg.qr(rng.standard_normal((d, d)) + 1j*rng.standard_normal((d, d)))[0]
        levels = np.concatenate(([0.8, 0.8], -0.5 - 0.9*np.arange(d - 2)))
        K0 = (U*levels) @ U.conj().T
        K1 = (U*np.eye(d)[1]) @ U.conj().T
        c_opers = np.stack([(K0 + K0.conj().T)/2, (K1 + K1.conj().T)/2, _herm(rng, 1, d)[0]])
        c_coeffs = rng.standard_normal((3, G))
        c_coeffs[:, 1] = [1.0, param, 0.0]
        return dict(c_opers=c_opers, c_coeffs=c_coeffs, **_common(rng, d, 3))
    if family == 'near_resonant':
        import ff_oracle as orc
        c_opers, c_coeffs = _herm(rng, 2, d), rng.standard_normal((2, G))
        inputs = dict(c_opers=c_opers, c_coeffs=c_coeffs, **_common(rng, d, 2))
        D = orc.diagonalize(orc.hamiltonian(c_opers, c_coeffs), inputs['dt'])[0][2]
        pairs = [(0, 1), (1, 0)] if d == 2 else [(0, 1), (3, 1)]
        grid = [-(D[m] - D[n])*(1.0 + e) for m, n in pairs for e in RESONANCE_EPS]
        inputs['omega'] = np.sort(np.array(grid + [1e-9, -1e-9, 1e-12, -1e-12, 0.0]))
        assert len(np.unique(inputs['omega'])) == len(inputs['omega'])
        return inputs
    raise ValueError(family)


def all_cases():
    """name -> (family, d, param, stores dR)"""
    cases = {}
    for d in (2, 3, 4):
        cases[f'exact_d{d}'] = ('exact', d, None, True)
    for d in (2, 3, 4):
        for e in NEAR_IDLE_EPS:
            cases[f'near_idle_d{d}_{e:.0e}'] = ('near_idle', d, e, d == 3 and e == 1e-9)
    for d in (3, 4):
        for e in CROSSING_DELTA:
            cases[f'crossing_d{d}_{e:.0e}'] = ('crossing', d, e, d == 4 and e == 1e-9)
    for d in (2, 4):
        cases[f'near_resonant_d{d}'] = ('near_resonant', d, None, False)
    return cases


def j_grid(theta, x_switch, dt=J_DT):
    """x, b in +-{0, 1e-15 ... 1e3}, with |b dt| = theta (1 +- 2^-30) and |x dt| = 2 (1 +- 2^-30) and
    x_switch (1 +- 2^-30), the two sides of where the code changes its evaluation: all pairs"""
    mags = [0.0] + [10.0**k for k in range(-15, 4)]
    base = sorted({s*m for m in mags for s in (1.0, -1.0)})
    edge = [s*(1.0 + e*2.0**-30) for s in (1.0, -1.0) for e in (1.0, -1.0)]
    xs = base + [2.0/dt*f for f in edge] + [x_switch/dt*f for f in edge]
    bs = base + [theta/dt*f for f in edge]
    x, b = np.meshgrid(xs, bs, indexing='ij')
    return x.ravel().copy(), b.ravel().copy()


# ---- the 60-digit reference ---------------------------------------------------------------------------------------
def _mp():
    import mpmath as mp
    mp.mp.dps = DPS
    return mp


def _matmul(X, Y):
    n = len(X)
    return [[sum(X[i][k]*Y[k][j] for k in range(n)) for j in range(n)] for i in range(n)]


def _dagger(X):
    n = len(X)
    return [[X[j][i].conjugate() for j in range(n)] for i in range(n)]


def _i1(mp, x, dt):
    if x == 0:
        return mp.mpc(dt)
    with mp.workdps(2*DPS):                    # (x of the size of the step: the cancellation costs 20 digits)
        v = (mp.expj(x*dt) - 1)/(mp.mpc(0, 1)*x)
    return +v


def j_exact(x, b, dt=J_DT):
    """J(x, b) = int_0^dt dtau e^{i x tau} int_0^tau dtau' e^{i b tau'} at the given doubles, complex128"""
    mp = _mp()
    out = np.empty(len(x), dtype=complex)
    t = mp.mpf(dt)
    for i, (xi, bi) in enumerate(zip(x, b)):
        xi, bi = mp.mpf(float(xi)), mp.mpf(float(bi))
        if bi != 0:
            v = (_i1(mp, xi + bi, t) - _i1(mp, xi, t))/(mp.mpc(0, 1)*bi)
        elif xi != 0:
            v = (t*mp.expj(xi*t) - _i1(mp, xi, t))/(mp.mpc(0, 1)*xi)
        else:
            v = t*t/2
        out[i] = complex(v)
    return out


class _Pulse:
    """Y_a(w) of a pulse from the definitions; a segment's own part is cached per (segment, amplitudes)."""

    def __init__(self, inputs):
        mp = self.mp = _mp()
        conv = lambda M: [[mp.mpc(complex(v).real, complex(v).imag) for v in row] for row in M]      # noqa: E731
        self.c_opers = [conv(M) for M in inputs['c_opers']]
        self.n_opers = [conv(M) for M in inputs['n_opers']]
        self.basis = np.asarray(inputs['basis'])
        self.n_coeffs = [[mp.mpf(float(v)) for v in row] for row in inputs['n_coeffs']]
        self.dt = [mp.mpf(float(v)) for v in inputs['dt']]
        self.omega = [mp.mpf(float(v)) for v in inputs['omega']]
        self.t = [sum(self.dt[:g], mp.mpf(0)) for g in range(len(self.dt))]
        self.d = len(self.c_opers[0])
        self.cache = {}

    def segment(self, g, amps):
        key = (g, tuple(amps))
        if key not in self.cache:
            mp, d = self.mp, self.d
            Hm = mp.matrix(d, d)
            for c, M in zip(amps, self.c_opers):
                for i in range(d):
                    for j in range(d):
                        Hm[i, j] += c*M[i][j]
            E, Vm = mp.eighe(Hm)
            V = [[Vm[i, j] for j in range(d)] for i in range(d)]
            Vd = _dagger(V)
            ph = [mp.expj(-E[m]*self.dt[g]) for m in range(d)]
            P = _matmul([[V[i][m]*ph[m] for m in range(d)] for i in range(d)], Vd)
            K = []
            for a, B in enumerate(self.n_opers):
                Bbar = _matmul(Vd, _matmul(B, V))
                row = []
                for w in self.omega:
                    inner = [[self.n_coeffs[a][g]*Bbar[m][n]*_i1(mp, w + E[m] - E[n], self.dt[g])
                              for n in range(d)] for m in range(d)]
                    row.append(_matmul(V, _matmul(inner, Vd)))
                K.append(row)
            self.cache[key] = (P, K)
        return self.cache[key]

    def noise_operators(self, coeffs):
        """Y[a][w] (d x d lists) for the (H, G) amplitudes `coeffs` (mpf)"""
        mp, d = self.mp, self.d
        n_seg = len(self.dt)
        Q = [[mp.mpc(int(i == j)) for j in range(d)] for i in range(d)]
        Y = [[[[mp.mpc(0) for _ in range(d)] for _ in range(d)] for _ in self.omega] for _ in self.n_opers]
        for g in range(n_seg):
            P, K = self.segment(g, [row[g] for row in coeffs])
            Qd = _dagger(Q)
            for a in range(len(self.n_opers)):
                for o, w in enumerate(self.omega):
                    step = _matmul(Qd, _matmul(K[a][o], Q))
                    ph = mp.expj(w*self.t[g])
                    for i in range(d):
                        for j in range(d):
                            Y[a][o][i][j] += ph*step[i][j]
            Q = _matmul(P, Q)
        return Y

    def observables(self, coeffs, with_R):
        Y = self.noise_operators(coeffs)
        d = self.d
        F = [[sum(abs(v)**2 for row in Yaw for v in row) for Yaw in Ya] for Ya in Y]
        R = None
        if with_R:
            nz = [[(i, j, complex(C[j, i])) for i in range(d) for j in range(d) if C[j, i] != 0] for C in self.basis]
            R = [[[sum(Yaw[i][j]*self.mp.mpc(c.real, c.imag) for i, j, c in terms) for terms in nz]
                  for Yaw in Ya] for Ya in Y]
        return F, R


def exact_derivatives(inputs, with_dR):
    """dF (A, G, H, W) float64 and, on request, dR (H, W, G, A, d^2) complex128."""
    mp = _mp()
    pulse = _Pulse(inputs)
    base = [[mp.mpf(float(v)) for v in row] for row in inputs['c_coeffs']]
    n_ctrl, n_seg = len(base), len(base[0])
    n_nops, W, N = len(pulse.n_opers), len(pulse.omega), len(pulse.basis)
    dF = np.empty((n_nops, n_seg, n_ctrl, W))
    dR = np.empty((n_ctrl, W, n_seg, n_nops, N), dtype=complex) if with_dR else None
    worst = mp.mpf(0)
    for h in range(n_ctrl):
        for s in range(n_seg):
            diffs = []
            for step in (mp.mpf(STEP), mp.mpf(STEP_CHECK)):
                obs = []
                for sign in (1, -1):
                    coeffs = [list(row) for row in base]
                    coeffs[h][s] = base[h][s] + sign*step
                    obs.append(pulse.observables(coeffs, with_dR))
                (Fp, Rp), (Fm, Rm) = obs
                flat = [(Fp[a][o] - Fm[a][o])/(2*step) for a in range(n_nops) for o in range(W)]
                if with_dR:
                    flat += [(Rp[a][o][k] - Rm[a][o][k])/(2*step)
                             for a in range(n_nops) for o in range(W) for k in range(N)]
                diffs.append(flat)
            fine, coarse = diffs
            scale = max(abs(v) for v in fine)
            worst = max(worst, max(abs(u - v) for u, v in zip(fine, coarse))/scale)
            dF[:, s, h, :] = np.array([float(v) for v in fine[:n_nops*W]]).reshape(n_nops, W)
            if with_dR:
                dR[h, :, s, :, :] = np.array([complex(v) for v in fine[n_nops*W:]]).reshape(
                    n_nops, W, N).transpose(1, 0, 2)
    assert worst < mp.mpf('1e-25'), f'steps {STEP} and {STEP_CHECK} differ by {mp.nstr(worst, 3)}'
    return dF, dR


def check_rows(name, dF, dR):
    """every row carries weight: the tests bound each row's error by 1e-10 of the row's own maximum"""
    rows = np.abs(dF).max(axis=-1)
    assert rows.min() >= 1e-6*rows.max(), (name, 'dF', rows.min()/rows.max())
    if dR is not None:
        rows = np.abs(dR).max(axis=(1, 4))                 # (H, G, A)
        assert rows.min() >= 1e-6*rows.max(), (name, 'dR', rows.min()/rows.max())


def main():
    import ctypes
    import time
    out = {}
    for name, (family, d, param, with_dR) in all_cases().items():
        tic = time.time()
        inputs = case_inputs(family, d, param)
        dF, dR = exact_derivatives(inputs, with_dR)
        check_rows(name, dF, dR)
        for key, value in inputs.items():
            out[f'{name}_{key}'] = value
        out[f'{name}_dF'] = dF
        if with_dR:
            out[f'{name}_dR'] = dR
        print(f'{name}: {time.time() - tic:.1f} s', flush=True)
    # the table of J for the host test; theta and the switch in x dt from the built host harness
    lib = ctypes.CDLL(os.path.join(os.path.dirname(HERE), 'tests', 'csrc', 'libffk_math_host.so'))
    lib.ffk_host_derivative_integral_band.restype = ctypes.c_double
    lib.ffk_host_derivative_integral_taylor.restype = ctypes.c_double
    theta, x_switch = lib.ffk_host_derivative_integral_band(), lib.ffk_host_derivative_integral_taylor()
    x, b = j_grid(theta, x_switch)
    out.update(J_theta=np.float64(theta), J_x_switch=np.float64(x_switch), J_dt=np.float64(J_DT), J_x=x, J_b=b,
               J_exact=j_exact(x, b))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f'{OUT}: {size} bytes')
    assert size < 300*1024


if __name__ == '__main__':
    main()

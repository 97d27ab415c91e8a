"""Generate tests/golden/second_order_exact.npz: second-order filter functions F2[a,b,k,l,w] from the DEFINITION, in
60-digit arithmetic, at and next to the degeneracies where the closed forms of the nested segment integral

    I_{ij,mn}(w) = J(a, b) = int_0^dt dtau e^{i a tau} int_0^tau dtau' e^{i b tau'},  a = W_ij - w,  b = w + W_mn

(csrc/second.hip before its series, ff_oracle.second_order_integral, the upstream reference) lose digits: they take the
limits only at b == 0.0 and a == 0.0 exactly, and they evaluate f(a + b) at fl(W_ij + W_mn), not at the sum of the
rounded a and b.

TEST INFRASTRUCTURE, CPU only, needs mpmath (imported inside the functions that use it).

    python oracle/make_exact_second_order.py

Per segment g, with H = sum_h c_h A_h = V D V^dag (mp.eighe), T = Q^dag V, Q the propagator up to t_g:

    NB_{ak,ij}  = s_a(g) (V^dag B_a V)_ij (T^dag C_k T)_ji
    G_ak(w)     = e^{i w t_g} sum_ij NB_{ak,ij} I1(w + W_ij)
    F2[a,b,k,l] += conj(G_ak) sum_{g'<g} G^(g')_bl  +  sum_{ij,mn} NB_{ak,ij} J(W_ij - w, w + W_mn) NB_{bl,mn}

J = (I1(a + b) - I1(a))/(i b) in 120 digits with a, b formed exactly from the 60-digit levels and the input double w;
the limit forms only where those exact values vanish.

Inputs: the recipes and seeds of make_exact.py (make_exact.SEEDS[family] + d), G = 4, GGM basis; A = 2 noise operators
at d = 2, 3 (so that a != b blocks exist), A = 1 at d = 4, 5; the grids below.  Per case the file also holds `near`
(which frequencies sit next to a degeneracy) and, for the near-resonant cases, `e` (the relative detuning, NaN
elsewhere).
It also holds a table of J at the arguments the kernels form, a = fl(-w + W_ij), b = fl(w + W_mn), ab = fl(W_ij + W_mn).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
OUT = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'second_order_exact.npz')

import make_exact  # noqa: E402
from make_exact import DPS, J_DT, _dagger, _i1, _matmul, _mp  # noqa: E402

MAX_BYTES = 500*1000
# a negative frequency, 0, |w dt| < 2 and > 2 for every dt in [0.2, 1.2]
# (and none of them on a resonance of the crossing cases, whose levels are 0.9, 1.3 and 2.2 apart)
OMEGA_EXACT = (-3.1, -0.4, 0.0, 0.7, 11.0)
OMEGA_BENIGN = (-3.1, 0.7, 11.0)
NEAR_IDLE_EPS = (1e-6, 1e-9, 1e-12, 1e-15)
CROSSING_DELTA = (1e-6, 1e-9, 1e-12)
RESONANCE_EPS = make_exact.RESONANCE_EPS
NEAR_ZERO = (1e-9, -1e-9, 1e-12, -1e-12)
# d -> (segment, level pairs (m, n) of it) whose resonances the grid sits on: of all segments and pairs those where the
# resonant entry weighs most in F2(w) -- the closed forms lose u/(e |W_mn| dt) of dt^2/2 in ONE entry, and at e = 1e-9
# that has to show against the whole of F2(w) for the host test to tell the formulas apart.  d = 5: flat index
# m d + n >= 16, the second chunk of the vector kernel's walk over mn
RESONANT = {2: (0, ((0, 1), (1, 0))), 4: (3, ((2, 0), (1, 3))), 5: (0, ((4, 3), (4, 2)))}
RESONANCE_EPS_D5 = (2.0**-50, 1e-9)
# the levels and frequencies of the issue's measurement, for the table of J
J_LEVELS_DELTA = (1e-6, 1e-12)


def n_nops(d):
    return 2 if d <= 3 else 1


# ---- inputs: NumPy only -------------------------------------------------------------------------------------------
def case_inputs(family, d, param=None):
    """The inputs of one case plus `near` and `e` (per frequency), float64 / complex128."""
    import ff_oracle as orc
    inputs = make_exact.case_inputs(family, d, param)
    A = n_nops(d)
    inputs['n_opers'], inputs['n_coeffs'] = inputs['n_opers'][:A].copy(), inputs['n_coeffs'][:A].copy()
    if family == 'exact':
        grid = [(w, False, np.nan) for w in OMEGA_EXACT]
    elif family in ('near_idle', 'crossing'):
        # near_idle: the segment's level spacings are of the size of param; crossing: one spacing IS param
        small = [0.0, 0.5*param, -0.5*param] + ([0.37*param] if family == 'near_idle' else [param, -param])
        grid = [(w, False, np.nan) for w in OMEGA_BENIGN] + [(w, True, np.nan) for w in small]
    elif family == 'near_resonant':
        segment, pairs = RESONANT[d]
        D = orc.diagonalize(orc.hamiltonian(inputs['c_opers'], inputs['c_coeffs']), inputs['dt'])[0][segment]
        if d == 5:
            grid = [(-(D[m] - D[n])*(1.0 + e), True, e) for m, n in pairs for e in RESONANCE_EPS_D5]
            grid += [(0.0, False, np.nan), (1e-9, True, np.nan)]
        else:
            # e = 0 takes the oracle's exact-zero branch, e = 1e-4 costs it 1e-12: neither is near
            grid = [(-(D[m] - D[n])*(1.0 + e), e not in (0.0, 1e-4), e) for m, n in pairs
                    for e in RESONANCE_EPS]
            grid += [(0.0, False, np.nan)] + [(w, True, np.nan) for w in NEAR_ZERO]
    else:
        raise ValueError(family)
    grid.sort(key=lambda row: row[0])
    inputs['omega'] = np.array([row[0] for row in grid])
    inputs['near'] = np.array([row[1] for row in grid])
    inputs['e'] = np.array([row[2] for row in grid])
    assert len(np.unique(inputs['omega'])) == len(inputs['omega'])
    return inputs


def all_cases():
    """name -> (family, d, param)"""
    cases = {}
    for d in (2, 3, 4):
        cases[f'exact_d{d}'] = ('exact', d, None)
    for d in (2, 3, 4):
        for e in NEAR_IDLE_EPS if d != 3 else (1e-9,):
            cases[f'near_idle_d{d}_{e:.0e}'] = ('near_idle', d, e)
    for d in (3, 4):
        for e in CROSSING_DELTA if d != 3 else (1e-9,):
            cases[f'crossing_d{d}_{e:.0e}'] = ('crossing', d, e)
    for d in (2, 4, 5):
        cases[f'near_resonant_d{d}'] = ('near_resonant', d, None)
    return cases


def j_points():
    """(a, b, ab) as the kernels form them for the levels (-0.5, 0.5, 0.5 + delta) and the frequencies 0, delta/2, 1.3,
    1 + delta, 1 (1 + 2^-50): a = fl(-w + W_ij), b = fl(w + W_mn), ab = fl(W_ij + W_mn); unique triples"""
    rows = set()
    for delta in J_LEVELS_DELTA:
        D = np.array([-0.5, 0.5, 0.5 + delta])
        dE = np.unique(np.subtract.outer(D, D))
        for w in (0.0, 0.5*delta, 1.3, 1.0 + delta, 1.0*(1.0 + 2.0**-50)):
            for wij in dE:
                for wmn in dE:
                    rows.add((float(-w + wij), float(w + wmn), float(wij + wmn)))
    a, b, ab = (np.array(col) for col in zip(*sorted(rows)))
    return a, b, ab


# ---- the 60-digit reference ---------------------------------------------------------------------------------------
def _j(mp, a, b, dt):
    with mp.workdps(2*DPS):
        i = mp.mpc(0, 1)
        if b != 0:
            v = (_i1(mp, a + b, dt) - _i1(mp, a, dt))/(i*b)
        elif a != 0:
            v = (dt*mp.expj(a*dt) - _i1(mp, a, dt))/(i*a)
        else:
            v = mp.mpc(dt*dt/2)
    return +v


def exact_second_order(inputs):
    """F2 (A, A, N, N, W) complex128"""
    mp = _mp()
    conv = lambda M: [[mp.mpc(complex(v).real, complex(v).imag) for v in row] for row in M]      # noqa: E731
    c_opers, n_opers = [conv(M) for M in inputs['c_opers']], [conv(M) for M in inputs['n_opers']]
    basis = [conv(M) for M in inputs['basis']]
    c_coeffs = [[mp.mpf(float(v)) for v in row] for row in inputs['c_coeffs']]
    n_coeffs = [[mp.mpf(float(v)) for v in row] for row in inputs['n_coeffs']]
    dt = [mp.mpf(float(v)) for v in inputs['dt']]
    omega = [mp.mpf(float(v)) for v in inputs['omega']]
    d, A, N, W = len(c_opers[0]), len(n_opers), len(basis), len(omega)
    AN, d2 = A*N, d*d
    Q = [[mp.mpc(int(i == j)) for j in range(d)] for i in range(d)]
    F2 = [[[mp.mpc(0) for _ in range(AN)] for _ in range(AN)] for _ in range(W)]
    cum = [[mp.mpc(0) for _ in range(AN)] for _ in range(W)]
    t = mp.mpf(0)
    for g in range(len(dt)):
        Hm = mp.matrix(d, d)
        for c, M in zip(c_coeffs, c_opers):
            for i in range(d):
                for j in range(d):
                    Hm[i, j] += c[g]*M[i][j]
        E, Vm = mp.eighe(Hm)
        V = [[Vm[i, j] for j in range(d)] for i in range(d)]
        Vd = _dagger(V)
        T = _matmul(_dagger(Q), V)
        Td = _dagger(T)
        Cbar = [_matmul(Td, _matmul(C, T)) for C in basis]
        Bbar = [_matmul(Vd, _matmul(B, V)) for B in n_opers]
        NB = [[n_coeffs[a][g]*Bbar[a][i][j]*Cbar[k][j][i] for i in range(d) for j in range(d)]
              for a in range(A) for k in range(N)]
        gap = [E[i] - E[j] for i in range(d) for j in range(d)]
        for o, w in enumerate(omega):
            I1 = [_i1(mp, w + x, dt[g]) for x in gap]
            ph = mp.expj(w*t)
            step = [ph*mp.fdot(NB[p], I1) for p in range(AN)]
            # column f = (m, n) of J: J(W_ij - w, w + W_mn); X = NB J first, then X NB^T
            JT = [[_j(mp, x - w, w + y, dt[g]) for x in gap] for y in gap]
            X = [[mp.fdot(NB[p], JT[f]) for f in range(d2)] for p in range(AN)]
            for p in range(AN):
                row = F2[o][p]
                for q in range(AN):
                    v = mp.fdot(X[p], NB[q])
                    if g > 0:
                        v += step[p].conjugate()*cum[o][q]
                    row[q] += v
            for q in range(AN):
                cum[o][q] += step[q]
        ph = [mp.expj(-E[m]*dt[g]) for m in range(d)]
        Q = _matmul(_matmul([[V[i][m]*ph[m] for m in range(d)] for i in range(d)], Vd), Q)
        t += dt[g]
    out = np.empty((A, A, N, N, W), dtype=complex)
    for o in range(W):
        out[..., o] = np.array([[complex(v) for v in row] for row in F2[o]]).reshape(A, N, A, N).transpose(0, 2, 1, 3)
    return out


def j_exact(a, b, dt=J_DT):
    """J(a, b) at the given doubles, complex128"""
    mp = _mp()
    t = mp.mpf(dt)
    return np.array([complex(_j(mp, mp.mpf(float(x)), mp.mpf(float(y)), t)) for x, y in zip(a, b)])


def check_weight(name, F2):
    """every frequency carries weight: the tests bound each frequency's error by 1e-10 of its own maximum"""
    per_w = np.abs(F2).max(axis=(0, 1, 2, 3))
    assert per_w.min() >= 1e-6*per_w.max(), (name, per_w.min()/per_w.max())


def main():
    import time
    out = {}
    for name, (family, d, param) in all_cases().items():
        tic = time.time()
        inputs = case_inputs(family, d, param)
        F2 = exact_second_order(inputs)
        check_weight(name, F2)
        for key, value in inputs.items():
            out[f'{name}_{key}'] = value
        out[f'{name}_F2'] = F2
        print(f'{name}: W = {len(inputs["omega"])}, {time.time() - tic:.1f} s', flush=True)
    a, b, ab = j_points()
    out.update(J_dt=np.float64(J_DT), J_a=a, J_b=b, J_ab=ab, J_exact=j_exact(a, b))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f'{OUT}: {size} bytes')
    assert size <= MAX_BYTES


if __name__ == '__main__':
    main()

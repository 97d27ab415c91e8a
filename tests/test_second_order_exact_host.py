"""CPU side of the exact second-order fixture (tests/golden/second_order_exact.npz, oracle/make_exact_second_order.py):
  * the generator reproduces the file;
  * the fixture tells the two formulas of the nested integral I_{ij,mn} = J(a, b) apart: the oracle (the reference's
    closed forms with their exact-zero tests, f(a + b) at fl(W_ij + W_mn)) meets the per-frequency bound at the exact
    degeneracies and at every benign frequency, and misses it by orders of magnitude at the frequencies next to a
    degeneracy -- so tests/test_second_order_exact_gpu.py fails on kernels that share those forms;
  * ffk_math.h's second_order_integral, compiled for the host, against J in 60 digits.

Criterion everywhere: for every frequency, max_abkl |got - ref| <= 1e-10 max_abkl |ref|."""
import ctypes
import os
import sys

import numpy as np
import pytest

import ff_oracle as orc
from conftest import ROOT, load_golden

TOL = 1e-10
INPUTS = ('c_opers', 'c_coeffs', 'n_opers', 'n_coeffs', 'dt', 'omega', 'basis')
EXACT = [f'exact_d{d}' for d in (2, 3, 4)]
NEAR_IDLE = ([f'near_idle_d{d}_{e}' for d in (2, 4) for e in ('1e-06', '1e-09', '1e-12', '1e-15')] +
             ['near_idle_d3_1e-09'])
CROSSING = [f'crossing_d4_{e}' for e in ('1e-06', '1e-09', '1e-12')] + ['crossing_d3_1e-09']
NEAR_RESONANT = [f'near_resonant_d{d}' for d in (2, 4, 5)]
MUST_MISS_EPS = (2.0**-50, 1e-12, 1e-9)


@pytest.fixture(scope='module')
def exact():
    return load_golden('second_order_exact')


@pytest.fixture(scope='module')
def oracle_errors(exact):
    """case -> the oracle's error per frequency, computed once"""
    cache = {}

    def errors(name):
        if name not in cache:
            inp = {k: exact[f'{name}_{k}'] for k in INPUTS}
            D, V, Q = orc.diagonalize(orc.hamiltonian(inp['c_opers'], inp['c_coeffs']), inp['dt'])
            got = orc.second_order_filter_function(D, V, Q, inp['omega'], inp['basis'], inp['n_opers'],
                                                   inp['n_coeffs'], inp['dt'])
            cache[name] = frequency_errors(got, exact[f'{name}_F2'])
        return cache[name]
    return errors


def frequency_errors(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    axes = tuple(range(ref.ndim - 1))
    return np.abs(got - ref).max(axis=axes)/np.abs(ref).max(axis=axes)


def test_the_generator_reproduces_the_fixture(exact):
    pytest.importorskip('mpmath')
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import make_exact_second_order as gen
    cases = gen.all_cases()
    assert sorted(cases) == sorted(EXACT + NEAR_IDLE + CROSSING + NEAR_RESONANT)
    name = 'exact_d2'
    inputs = gen.case_inputs(*cases[name])
    for key, value in inputs.items():
        assert np.array_equal(value, exact[f'{name}_{key}'], equal_nan=value.dtype.kind == 'f'), key
    F2 = gen.exact_second_order(inputs)
    ref = exact[f'{name}_F2']
    assert F2.shape == ref.shape and F2.dtype == ref.dtype
    assert np.abs(F2 - ref).max() <= 1e-14*np.abs(ref).max()
    # every case of the generator is in the file with the generator's grid, and every frequency carries weight
    for case, spec in cases.items():
        gen.check_weight(case, exact[f'{case}_F2'])
        inputs = gen.case_inputs(*spec)
        for key in ('omega', 'near', 'e'):
            assert np.array_equal(inputs[key], exact[f'{case}_{key}'], equal_nan=key == 'e'), (case, key)
        assert exact[f'{case}_F2'].shape[-1] == len(inputs['omega']) <= 25
    for got, key in zip(gen.j_points(), ('J_a', 'J_b', 'J_ab')):
        assert np.array_equal(got, exact[key]), key


def test_the_grids_hold_what_the_cases_are_about(exact):
    for name in EXACT:
        w, dt = exact[f'{name}_omega'], exact[f'{name}_dt']
        assert w.min() < 0 and np.any(w == 0) and not exact[f'{name}_near'].any()
        assert np.any(np.abs(w).max()*dt.min() > 2) and np.any((w > 0) & (w*dt.max() < 2))
        assert np.all(exact[f'{name}_c_coeffs'][:, 1] == 0)
    for name in NEAR_IDLE + CROSSING:
        size = float(name.rsplit('_', 1)[1])
        w, near = exact[f'{name}_omega'], exact[f'{name}_near']
        assert np.array_equal(near, np.abs(w) <= size) and {0.0, 0.5*size, -0.5*size} <= set(w[near])
    for name in NEAR_RESONANT:
        w, e = exact[f'{name}_omega'], exact[f'{name}_e']
        assert {2.0**-50, 1e-9} <= set(e[~np.isnan(e)]) and {0.0, 1e-9} <= set(w)
    assert exact['near_resonant_d5_omega'].size in (4, 5, 6)
    assert exact['near_resonant_d2_n_opers'].shape[0] == 2 and exact['near_resonant_d4_n_opers'].shape[0] == 1


@pytest.mark.parametrize('name', EXACT)
def test_the_oracle_meets_the_bound_at_exact_degeneracies(oracle_errors, name):
    err = oracle_errors(name)
    print(f'{name}: oracle worst frequency {err.max():.3e}')
    assert err.max() <= TOL


@pytest.mark.parametrize('name', NEAR_IDLE + CROSSING + NEAR_RESONANT)
def test_the_oracle_meets_the_bound_at_the_benign_frequencies(exact, oracle_errors, name):
    """what makes the criterion fair: away from the degeneracies the reference's own formulas pass it"""
    near = exact[f'{name}_near']
    assert (~near).any()
    err = oracle_errors(name)[~near]
    print(f'{name}: oracle worst benign frequency {err.max():.3e}')
    assert err.max() <= TOL


@pytest.mark.parametrize('name', [n for n in NEAR_IDLE + CROSSING if not n.endswith('1e-06')])
def test_the_oracle_misses_the_bound_next_to_a_degeneracy(exact, oracle_errors, name):
    """The closed forms lose u/|b dt| (b = w + W_mn small, not zero) and u/|a dt| (b == 0) of dt^2/2: at 1e-9 about
    1e-7 of one entry -- the weakness of the reference's formula on record, and the proof that the GPU test tells a
    kernel with those forms from one without."""
    err = oracle_errors(name)[exact[f'{name}_near']]
    print(f'{name}: oracle worst frequency next to the degeneracy {err.max():.3e}')
    assert err.max() >= 100*TOL


@pytest.mark.parametrize('name', NEAR_RESONANT)
def test_the_oracle_misses_the_bound_next_to_a_resonance(exact, oracle_errors, name):
    """every frequency w = -W_mn (1 + e), e in {2^-50, 1e-12, 1e-9}, by itself: f(a + b) at fl(W_ij + W_mn) is not
    f at the sum of the rounded a and b, so the numerator does not vanish with b -- order one at 2^-50"""
    e, err = exact[f'{name}_e'], oracle_errors(name)
    picked = np.isin(e, MUST_MISS_EPS)
    assert picked.sum() >= 4 and exact[f'{name}_near'][picked].all()
    for eps, value in zip(e[picked], err[picked]):
        print(f'{name}: e = {eps:.1e}: oracle {value:.3e}')
    assert err[picked].min() >= 100*TOL


def test_second_order_integral_on_the_host(exact):
    """I_{ij,mn} = J(a, b) of csrc/ffk_math.h (second_order_integral: what the second-order kernels evaluate per entry)
    against J in 60 digits at dt = 0.37, on
      * the gradient fixture's table: a, b in +-{0, 1e-15 ... 1e3}, |b dt| on both sides of theta, |a dt| on both sides
        of 2 and of where the moments change from recurrence to series; f(a + b) at fl(a + b);
      * the arguments the kernels form for the levels (-0.5, 0.5, 0.5 + delta) at w = 0, delta/2, 1.3, 1 + delta,
        1 + 2^-50: a = fl(-w + W_ij), b = fl(w + W_mn), f(a + b) at fl(W_ij + W_mn).
    Bound 8 u/theta of dt^2/2 (u = 2^-53): twice the divided difference's own rounding at the switch.  The closed
    forms with exact-zero tests reach order one on the second set."""
    path = os.path.join(ROOT, 'tests', 'csrc', 'libffk_math_host.so')
    if not os.path.exists(path):
        pytest.skip('host math harness not built')
    lib = ctypes.CDLL(path)
    lib.ffk_host_derivative_integral_band.restype = ctypes.c_double
    lib.ffk_host_derivative_integral_taylor.restype = ctypes.c_double
    theta, x_switch = lib.ffk_host_derivative_integral_band(), lib.ffk_host_derivative_integral_taylor()
    table = load_golden('gradient_exact')
    assert (theta, x_switch) == (float(table['J_theta']), float(table['J_x_switch'])), \
        'the switches moved: regenerate the fixtures (oracle/make_exact.py, oracle/make_exact_second_order.py)'
    dt = float(exact['J_dt'])
    assert dt == float(table['J_dt'])
    bound = 8*2.0**-53/theta
    assert bound <= 1e-12
    dp = ctypes.POINTER(ctypes.c_double)

    def errors(a, b, ab, ref):
        a, b, ab = (np.ascontiguousarray(v, dtype=float) for v in (a, b, ab))
        out = np.empty(2*a.size)
        lib.ffk_host_second_order_integral(ctypes.c_long(a.size), a.ctypes.data_as(dp), b.ctypes.data_as(dp),
                                           ab.ctypes.data_as(dp), ctypes.c_double(dt), out.ctypes.data_as(dp))
        return np.abs(out[0::2] + 1j*out[1::2] - ref)/(dt*dt/2)

    a, b = table['J_x'], table['J_b']
    assert np.any(np.abs(a*dt) == x_switch*(1 + 2.0**-30)) and np.any(np.abs(a*dt) == x_switch*(1 - 2.0**-30))
    assert np.any(np.abs(b*dt) == theta*(1 + 2.0**-30)) and np.any(np.abs(b*dt) < theta)
    assert np.any(b == 0) and np.any(a == 0) and np.any(np.abs(a*dt) > 2)
    err = errors(a, b, a + b, table['J_exact'])
    series = np.abs(b*dt) < theta
    print(f'table of the gradients, theta = {theta}: series worst {err[series].max():.3e}, divided difference worst '
          f'{err[~series].max():.3e}, bound {bound:.3e}')
    assert err.max() <= bound

    a, b, ab = exact['J_a'], exact['J_b'], exact['J_ab']
    series = np.abs(b*dt) < theta
    assert series.any() and (~series).any() and np.any(b == 0) and np.any((b != 0) & (np.abs(b) < 1e-15))
    assert np.any(ab != a + b)
    err = errors(a, b, ab, exact['J_exact'])
    print(f'arguments as the kernels form them: series worst {err[series].max():.3e}, divided difference worst '
          f'{err[~series].max():.3e}, bound {bound:.3e}')
    assert err.max() <= bound
    # the closed forms with exact-zero tests on the same arguments (what the kernels evaluated before)
    with np.errstate(all='ignore'):
        f = lambda v: np.where(v == 0, 1j*dt, orc.cexpm1(v*dt)/np.where(v == 0, 1, v))      # noqa: E731
        old = np.where(b != 0, (f(a) - f(ab))/np.where(b == 0, 1, b),
                       np.where(a != 0, (f(a) - 1j*dt*orc.cexp(a*dt))/np.where(a == 0, 1, a), dt*dt/2))
    old_err = np.abs(old - exact['J_exact'])/(dt*dt/2)
    print(f'closed forms with exact-zero tests: worst {old_err.max():.3e}')
    assert old_err.max() > 0.1

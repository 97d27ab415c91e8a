"""CPU side of the exact gradient fixture (tests/golden/gradient_exact.npz, oracle/make_exact.py):
  * the generator reproduces the file;
  * the fixture tells the two formulas of the nested integral J apart: the oracle (the reference's closed forms with
    their exact-zero tests) meets the row bound at the exact degeneracies and misses it by orders of magnitude next to
    them -- so tests/test_gradient_exact_gpu.py fails on kernels that share those forms;
  * ffk_math.h's derivative_integral, compiled for the host, against J in 60 digits."""
import ctypes
import os
import sys

import numpy as np
import pytest

import ff_oracle as orc
from conftest import ROOT, load_golden

TOL = 1e-10
INPUTS = ('c_opers', 'c_coeffs', 'n_opers', 'n_coeffs', 'dt', 'omega', 'basis')


@pytest.fixture(scope='module')
def exact():
    return load_golden('gradient_exact')


def oracle_row_error(g, name):
    inp = {k: g[f'{name}_{k}'] for k in INPUTS}
    D, V, Q = orc.diagonalize(orc.hamiltonian(inp['c_opers'], inp['c_coeffs']), inp['dt'])
    got = orc.filter_function_derivative(D, V, Q, inp['omega'], inp['basis'], inp['n_opers'], inp['n_coeffs'],
                                         inp['c_opers'], inp['dt'])
    ref = g[f'{name}_dF']
    return float((np.abs(got - ref).max(axis=-1)/np.abs(ref).max(axis=-1)).max())


def test_the_generator_reproduces_the_fixture(exact):
    pytest.importorskip('mpmath')
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import make_exact
    name = 'exact_d2'
    family, d, param, with_dR = make_exact.all_cases()[name]
    inputs = make_exact.case_inputs(family, d, param)
    for key, value in inputs.items():
        assert np.array_equal(value, exact[f'{name}_{key}']), key
    dF, dR = make_exact.exact_derivatives(inputs, with_dR)
    for got, ref in ((dF, exact[f'{name}_dF']), (dR, exact[f'{name}_dR'])):
        assert got.shape == ref.shape and got.dtype == ref.dtype
        assert np.abs(got - ref).max() <= 1e-14*np.abs(ref).max()
    # every case of the generator is in the file, and the rows the tests bound one by one all carry weight
    for case, (_, _, _, stores_dR) in make_exact.all_cases().items():
        make_exact.check_rows(case, exact[f'{case}_dF'], exact[f'{case}_dR'] if stores_dR else None)
        assert (f'{case}_dR' in exact) == stores_dR


@pytest.mark.parametrize('d', [2, 3, 4])
def test_the_oracle_meets_the_row_bound_at_exact_degeneracies(exact, d):
    err = oracle_row_error(exact, f'exact_d{d}')
    print(f'exact_d{d}: oracle worst row {err:.3e}')
    assert err <= TOL


@pytest.mark.parametrize('name', [f'near_idle_d{d}_{e}' for d in (2, 3, 4) for e in ('1e-09', '1e-12', '1e-15')] +
                         [f'crossing_d{d}_{e}' for d in (3, 4) for e in ('1e-09', '1e-12')])
def test_the_oracle_misses_the_row_bound_next_to_them(exact, name):
    """The closed forms lose eps/|b dt| (two levels b apart) and eps/|x dt| (b == 0, x = w + W_mn) of dt^2/2: at 1e-9
    about 1e-7 -- the weakness of the reference's formula on record, and the proof that the GPU test tells a kernel
    with those forms from one without."""
    err = oracle_row_error(exact, name)
    print(f'{name}: oracle worst row {err:.3e}')
    assert err >= 100*TOL


def test_derivative_integral_on_the_host(exact):
    """J(x, b) of csrc/ffk_math.h from I1(x) and I1 at the rounded sum x + b, as the kernels form it, against J in
    60 digits: dt = 0.37, x, b in +-{0, 1e-15 ... 1e3}, |b dt| on both sides of theta, |x dt| on both sides of 2 and of
    where the code's series changes its evaluation.
    Bound 8 u/theta of dt^2/2 (u = 2^-53): twice the divided difference's own rounding at the switch.  On this grid the
    closed forms with exact-zero tests reach 1.3 dt^2/2."""
    path = os.path.join(ROOT, 'tests', 'csrc', 'libffk_math_host.so')
    if not os.path.exists(path):
        pytest.skip('host math harness not built')
    lib = ctypes.CDLL(path)
    lib.ffk_host_derivative_integral_band.restype = ctypes.c_double
    theta = lib.ffk_host_derivative_integral_band()
    x, b, dt = exact['J_x'], exact['J_b'], float(exact['J_dt'])
    lib.ffk_host_derivative_integral_taylor.restype = ctypes.c_double
    x_switch = lib.ffk_host_derivative_integral_taylor()
    assert (theta, x_switch) == (float(exact['J_theta']), float(exact['J_x_switch'])), \
        'the switches moved: regenerate the fixture (oracle/make_exact.py)'
    assert np.any(np.abs(x*dt) == x_switch*(1 + 2.0**-30)) and np.any(np.abs(x*dt) == x_switch*(1 - 2.0**-30))
    assert np.any(np.abs(b*dt) == theta*(1 + 2.0**-30)) and np.any(np.abs(b*dt) < theta) and np.any(b == 0)
    assert np.any(np.abs(x*dt) > 2) and np.any((np.abs(x*dt) < 2) & (np.abs(x*dt) > 1.99)) and np.any(x == 0)
    bound = 8*2.0**-53/theta
    assert bound <= 1e-12
    dp = ctypes.POINTER(ctypes.c_double)
    out = np.empty(2*x.size)
    lib.ffk_host_derivative_integral(ctypes.c_long(x.size), x.ctypes.data_as(dp), b.ctypes.data_as(dp),
                                     ctypes.c_double(dt), out.ctypes.data_as(dp))
    err = np.abs(out[0::2] + 1j*out[1::2] - exact['J_exact'])/(dt*dt/2)
    series = np.abs(b*dt) < theta
    print(f'theta = {theta}: series worst {err[series].max():.3e}, divided difference worst {err[~series].max():.3e}, '
          f'bound {bound:.3e}')
    assert err.max() <= bound
    # the closed forms with exact-zero tests on the same grid (what the kernels evaluated before)
    with np.errstate(all='ignore'):
        i1 = lambda v: np.where(v == 0, dt, orc.cexpm1(v*dt)/(1j*np.where(v == 0, 1, v)))      # noqa: E731
        old = np.where(b != 0, (i1(x + b) - i1(x))/(1j*np.where(b == 0, 1, b)),
                       np.where(x != 0, (dt*orc.cexp(x*dt) - i1(x))/(1j*np.where(x == 0, 1, x)), dt*dt/2))
    old_err = np.abs(old - exact['J_exact'])/(dt*dt/2)
    print(f'closed forms with exact-zero tests: worst {old_err.max():.3e}')
    assert old_err.max() > 1e-3

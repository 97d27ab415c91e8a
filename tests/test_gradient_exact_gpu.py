"""The gradient kernels (csrc/grad.hip, csrc/grad_batch.hip) against derivatives taken from the DEFINITIONS in 60-digit
arithmetic (tests/golden/gradient_exact.npz, written by oracle/make_exact.py), at and next to the degeneracies where
the closed forms of the nested integral J divide a difference of nearly equal numbers by a small one: an exactly idle
segment, a nearly idle one, two levels of a segment a distance delta apart, frequencies on and next to resonances.
The oracle and the upstream reference share those closed forms and lose up to all digits there
(tests/test_gradient_exact_host.py); ffk_math.h's derivative_integral does not.

Criterion everywhere: for every row (a, s, h), max_w |got - ref| <= 1e-10 max_w |ref| -- by row, so that one bad
segment cannot hide behind the others.  For the derivative of the control matrix a row is (h, s, a), over w and k."""
import numpy as np
import pytest

import ff_oracle as orc
import filter_functions_amd as ff
from conftest import load_golden
from filter_functions_amd import gradient, numeric

pytestmark = pytest.mark.gpu

TOL = 1e-10          # the project's bar (test_gpu_parity.py), here per row
NEAR_IDLE_EPS = ('1e-02', '1e-03', '1e-04', '1e-06', '1e-09', '1e-12', '1e-15')
CROSSING_DELTA = ('1e-03', '1e-06', '1e-09', '1e-12')
# the cases of one family and dimension share a shape: one batched pass
GROUPS = {**{f'exact d={d}': [f'exact_d{d}'] for d in (2, 3, 4)},
          **{f'near-idle d={d}': [f'near_idle_d{d}_{e}' for e in NEAR_IDLE_EPS] for d in (2, 3, 4)},
          **{f'crossing d={d}': [f'crossing_d{d}_{e}' for e in CROSSING_DELTA] for d in (3, 4)},
          **{f'near-resonant d={d}': [f'near_resonant_d{d}'] for d in (2, 4)}}
WITH_DR = ('exact_d2', 'exact_d3', 'exact_d4', 'near_idle_d3_1e-09', 'crossing_d4_1e-09')


@pytest.fixture(scope='module')
def exact():
    return load_golden('gradient_exact')


def make_pulse(g, name):
    d = g[f'{name}_c_opers'].shape[-1]
    pulse = ff.PulseSequence(
        [[op, c, str(i)] for op, c, i in zip(g[f'{name}_c_opers'], g[f'{name}_c_coeffs'], g[f'{name}_c_ids'])],
        [[op, c, f'n{a}'] for a, (op, c) in enumerate(zip(g[f'{name}_n_opers'], g[f'{name}_n_coeffs']))],
        g[f'{name}_dt'], ff.Basis(g[f'{name}_basis'], btype='GGM'))
    assert pulse.d == d
    return pulse


def in_fixture_order(got, pulse, g, name):
    """the library orders the control axis by sorted identifier; the fixture by c_opers"""
    assert list(pulse.n_oper_identifiers) == sorted(pulse.n_oper_identifiers)
    ids = [str(i) for i in g[f'{name}_c_ids']]
    position = {ident: k for k, ident in enumerate(sorted(ids))}
    return np.take(got, [position[i] for i in ids], axis=-2 if got.ndim == 4 else -1)


def row_error(got, ref, axes=-1):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((np.abs(got - ref).max(axis=axes)/np.abs(ref).max(axis=axes)).max())


def spectra(omega, A):
    return {'1-D': 1.0/(1.0 + omega**2),
            '(A, W)': np.stack([(a + 1.0)/(1.0 + (omega/(a + 2.0))**2) for a in range(A)])}


def exact_infidelity_derivative(dF, S, omega, d):
    """the project's trapezoid rule on S dF_exact, over 2 pi d"""
    return orc.integrate((S[:, None, None, :] if S.ndim == 2 else S)*dF, omega)/(2*np.pi*d)


def batch_of(g, names):
    """fresh pulses; a group of one is doubled, a lone pulse would not take the batched route"""
    names = list(names)*2 if len(names) == 1 else list(names)
    return names, [make_pulse(g, name) for name in names]


@pytest.mark.parametrize('group', list(GROUPS))
def test_single_path_against_exact_derivatives(exact, group):
    """gradient.filter_function_derivative (grad_kernel) on a fresh pulse per case"""
    worst = 0.0
    for name in GROUPS[group]:
        pulse = make_pulse(exact, name)
        got = in_fixture_order(gradient.filter_function_derivative(pulse, exact[f'{name}_omega']), pulse, exact, name)
        err = row_error(got, exact[f'{name}_dF'])
        print(f'{name}: dF single, worst row {err:.3e}')
        worst = max(worst, err)
    print(f'{group}: dF single, worst row of the family {worst:.3e}')
    assert worst <= TOL


@pytest.mark.parametrize('name', WITH_DR)
def test_control_matrix_derivative_against_exact_derivatives(exact, name):
    """gradient.calculate_derivative_of_control_matrix_from_scratch (grad_ctrlmat_kernel), rows (h, s, a) over (w, k)"""
    g = exact
    dt, c_opers = g[f'{name}_dt'], g[f'{name}_c_opers']
    D, V, Q = numeric.diagonalize(np.einsum('hij,hg->gij', c_opers, g[f'{name}_c_coeffs']), dt)
    dR = gradient.calculate_derivative_of_control_matrix_from_scratch(
        g[f'{name}_omega'], Q, D, V, g[f'{name}_basis'], None, dt, g[f'{name}_n_opers'], g[f'{name}_n_coeffs'], c_opers)
    err = row_error(dR, g[f'{name}_dR'], axes=(1, 4))
    print(f'{name}: dR, worst row {err:.3e}')
    assert err <= TOL


@pytest.mark.parametrize('group', list(GROUPS))
def test_batched_pass_against_exact_derivatives(exact, group):
    """ff.filter_function_derivatives on the cases of one family and dimension as one list (grad_batch_kernel): a
    nearly idle member beside its neighbours; once more in reversed order"""
    worst = 0.0
    for flip in (False, True):
        names, pulses = batch_of(exact, GROUPS[group][::-1] if flip else GROUPS[group])
        dF = ff.filter_function_derivatives(pulses, exact[f'{names[0]}_omega'])
        for name, pulse, member in zip(names, pulses, dF):
            err = row_error(in_fixture_order(member, pulse, exact, name), exact[f'{name}_dF'])
            print(f'{name}: dF batched{" reversed" if flip else ""}, worst row {err:.3e}')
            worst = max(worst, err)
    print(f'{group}: dF batched, worst row of the family {worst:.3e}')
    assert worst <= TOL


@pytest.mark.parametrize('group', list(GROUPS))
def test_infidelity_derivatives_against_the_trapezoid_of_exact_derivatives(exact, group):
    """ff.infidelity_derivatives and gradient.infidelity_derivative, 1-D and (A, W) spectrum: a row is one number"""
    g = exact
    worst = {}
    omega = g[f'{GROUPS[group][0]}_omega']
    for key, S in spectra(omega, 2).items():
        names, pulses = batch_of(g, GROUPS[group])
        batched = ff.infidelity_derivatives(pulses, S, omega)
        for name, pulse, member in zip(names, pulses, batched):
            ref = exact_infidelity_derivative(g[f'{name}_dF'], S, omega, pulse.d)
            single = gradient.infidelity_derivative(make_pulse(g, name), S, omega)
            for route, got in (('batched', member), ('single', single)):
                got = in_fixture_order(got, pulse, g, name)
                err = float((np.abs(got - ref)/np.abs(ref)).max())
                print(f'{name}: dI {route}, {key} spectrum, worst row {err:.3e}')
                worst[route, key] = max(worst.get((route, key), 0.0), err)
    for (route, key), err in worst.items():
        print(f'{group}: dI {route}, {key} spectrum, worst row of the family {err:.3e}')
    for (route, key), err in worst.items():
        assert err <= TOL, (route, key)

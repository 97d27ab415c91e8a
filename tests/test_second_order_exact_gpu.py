"""The second-order kernels (csrc/second.hip) against F2 from the DEFINITION in 60-digit arithmetic
(tests/golden/second_order_exact.npz, written by oracle/make_exact_second_order.py), at and next to the degeneracies
where the closed forms of the nested segment integral I_{ij,mn} = J(W_ij - w, w + W_mn) divide a difference of nearly
equal numbers by a small one: an exactly idle segment, a nearly idle one, two levels of a segment a distance delta
apart, frequencies on and next to resonances.  The oracle and the upstream reference share those closed forms and lose up to
all digits there (tests/test_second_order_exact_host.py); ffk_math.h's series does not.

Criterion: for every frequency, max_abkl |got - ref| <= 1e-10 max_abkl |ref| -- by frequency, so that one bad frequency
cannot hide behind the others.  Frequency shifts: per noise operator (pair), over (k, l)."""
import numpy as np
import pytest

import ff_oracle as orc
import filter_functions_amd as ff
from conftest import load_golden
from filter_functions_amd import numeric

pytestmark = pytest.mark.gpu

TOL = 1e-10          # the project's bar (test_gpu_parity.py), here per frequency
GROUPS = {**{f'exact d={d}': [f'exact_d{d}'] for d in (2, 3, 4)},
          **{f'near-idle d={d}': [f'near_idle_d{d}_{e}' for e in ('1e-06', '1e-09', '1e-12', '1e-15')] for d in (2, 4)},
          'near-idle d=3': ['near_idle_d3_1e-09'],
          'crossing d=3': ['crossing_d3_1e-09'],
          'crossing d=4': [f'crossing_d4_{e}' for e in ('1e-06', '1e-09', '1e-12')],
          **{f'near-resonant d={d}': [f'near_resonant_d{d}'] for d in (2, 4, 5)}}


@pytest.fixture(scope='module')
def exact():
    return load_golden('second_order_exact')


def make_pulse(g, name):
    return ff.PulseSequence(
        [[op, c, str(i)] for op, c, i in zip(g[f'{name}_c_opers'], g[f'{name}_c_coeffs'], g[f'{name}_c_ids'])],
        [[op, c, f'n{a}'] for a, (op, c) in enumerate(zip(g[f'{name}_n_opers'], g[f'{name}_n_coeffs']))],
        g[f'{name}_dt'], ff.Basis(g[f'{name}_basis'], btype='GGM'))


def frequency_error(got, ref):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype)
    axes = tuple(range(ref.ndim - 1))
    return float((np.abs(got - ref).max(axis=axes)/np.abs(ref).max(axis=axes)).max())


def check_group(exact, group, route, compute):
    worst = 0.0
    for name in GROUPS[group]:
        err = frequency_error(compute(name), exact[f'{name}_F2'])
        print(f'{name}: F2 {route}, worst frequency {err:.3e}')
        worst = max(worst, err)
    print(f'{group}: F2 {route}, worst frequency of the family {worst:.3e}')
    assert worst <= TOL


@pytest.mark.parametrize('group', list(GROUPS))
def test_matrix_core_kernel_against_exact_second_order(exact, group):
    """pulse.get_filter_function(omega, order=2), default route (so_mfma_kernel at these shapes)"""
    check_group(exact, group, 'matrix cores',
                lambda name: make_pulse(exact, name).get_filter_function(exact[f'{name}_omega'], order=2))


@pytest.mark.parametrize('group', list(GROUPS))
def test_vector_kernel_against_exact_second_order(exact, group, monkeypatch):
    """the same with FFK_TUNE_SO_MFMA=0 (so_accumulate_kernel; d = 5 walks mn in two chunks)"""
    monkeypatch.setenv('FFK_TUNE_SO_MFMA', '0')
    check_group(exact, group, 'vector kernel',
                lambda name: make_pulse(exact, name).get_filter_function(exact[f'{name}_omega'], order=2))


@pytest.mark.parametrize('group', list(GROUPS))
def test_free_function_against_exact_second_order(exact, group):
    """numeric.calculate_second_order_filter_function_from_scratch on the library's own eigensystem"""
    def compute(name):
        pulse = make_pulse(exact, name)
        pulse.diagonalize()
        return numeric.calculate_second_order_filter_function_from_scratch(
            pulse.eigvals, pulse.eigvecs, pulse.propagators, exact[f'{name}_omega'], pulse.basis, pulse.n_opers,
            pulse.n_coeffs, pulse.dt)
    check_group(exact, group, 'free function', compute)


@pytest.mark.parametrize('group', list(GROUPS))
def test_device_pipeline_against_exact_second_order(exact, group):
    """DevicePipeline.second_order_filter_function(): eigensystem and F2 stay in HBM"""
    from filter_functions_amd.device import DevicePipeline

    def compute(name):
        g = exact
        pipe = DevicePipeline(g[f'{name}_c_opers'], g[f'{name}_c_coeffs'], g[f'{name}_n_opers'],
                              g[f'{name}_n_coeffs'], g[f'{name}_dt'], g[f'{name}_basis'], g[f'{name}_omega'])
        pipe.launch(with_infidelity=False)
        return pipe.second_order_filter_function().cpu().numpy()
    check_group(exact, group, 'device pipeline', compute)


def spectra(omega, A):
    return {'1-D': 1.0/(1.0 + omega**2),
            '(A, W)': np.stack([(a + 1.0)/(1.0 + (omega/(a + 2.0))**2) for a in range(A)])}


@pytest.mark.parametrize('group', list(GROUPS))
def test_fused_frequency_shifts_against_the_trapezoid_of_exact_second_order(exact, group):
    """numeric.calculate_frequency_shifts on a fresh pulse (the fused pass), 1-D and (A, W) spectrum, against the
    project's trapezoid rule on the exact F2; per noise operator, max_kl |got - ref| <= 1e-10 max_kl |ref|"""
    worst = {}
    for name in GROUPS[group]:
        omega, F2 = exact[f'{name}_omega'], exact[f'{name}_F2']
        A = F2.shape[0]
        for key, S in spectra(omega, A).items():
            ref = orc.frequency_shifts(F2, S, omega, np.arange(A))
            got = numeric.calculate_frequency_shifts(make_pulse(exact, name), S, omega)
            assert got.shape == ref.shape == (A,) + F2.shape[2:4]
            err = float((np.abs(got - ref).max(axis=(1, 2))/np.abs(ref).max(axis=(1, 2))).max())
            print(f'{name}: frequency shifts, {key} spectrum, worst operator {err:.3e}')
            worst[key] = max(worst.get(key, 0.0), err)
    for key, err in worst.items():
        print(f'{group}: frequency shifts, {key} spectrum, worst operator of the family {err:.3e}')
    for key, err in worst.items():
        assert err <= TOL, key

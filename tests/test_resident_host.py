"""CPU side of the resident entry points (ffk_api_resident.hip): argument checks that come before any device call."""
import ctypes

import numpy as np
import pytest

from filter_functions_amd import _lib


@pytest.mark.parametrize('idx', [[0, 2], [-1, 0]])
def test_noise_operator_indices_outside_the_operators_are_rejected(idx):
    """idx[i] outside [0, A) is FFK_EINVAL in the single and in the batched resident pass (it used to reach the
    integral's kernel, which read the filter function out of bounds)."""
    lib = _lib.load()
    G, d, W, N, A, n_c, P = 3, 2, 8, 4, 2, 2, 2
    rng = np.random.default_rng(5)
    idx = np.array(idx, dtype=np.int32)

    def inputs(*lead):
        c_opers = rng.standard_normal(lead + (n_c, d, d)) + 0j
        n_opers = rng.standard_normal(lead + (A, d, d)) + 0j
        dt = np.ones(lead + (G,))
        t = np.concatenate([np.zeros(lead + (1,)), dt.cumsum(axis=-1)], axis=-1)
        return c_opers, rng.standard_normal(lead + (n_c, G)), dt, t, n_opers, np.ones(lead + (A, G))
    omega = np.linspace(0.1, 2.0, W)
    basis = rng.standard_normal((N, d, d)) + 0j
    spectrum = np.ones((A, W))
    out = [ctypes.c_void_p() for _ in range(4)]
    results = tuple(ctypes.byref(p) for p in out)
    handle = ctypes.c_void_p()
    _lib.check(lib.ffk_resident_create(ctypes.byref(handle)))
    try:
        C, c, dt, t, B, s = inputs()
        infid = np.zeros(len(idx))
        rc = lib.ffk_resident_filter_function_infidelity(
            handle, C.ctypes.data, n_c, c.ctypes.data, dt.ctypes.data, t.ctypes.data, G, d, omega.ctypes.data, W,
            basis.ctypes.data, N, B.ctypes.data, A, s.ctypes.data, spectrum.ctypes.data, 2, 1, idx.ctypes.data,
            len(idx), d, *results, infid.ctypes.data)
        assert rc == _lib.FFK_EINVAL
        assert b'idx' in lib.ffk_last_error()
        C, c, dt, t, B, s = inputs(P)
        infid, n_failed = np.zeros((P, len(idx))), np.zeros(P, dtype=np.int32)
        rc = lib.ffk_resident_batch_filter_function_infidelity(
            handle, P, C.ctypes.data, n_c, c.ctypes.data, dt.ctypes.data, t.ctypes.data, G, d, omega.ctypes.data, W,
            basis.ctypes.data, N, B.ctypes.data, A, s.ctypes.data, spectrum.ctypes.data, 2, 1, idx.ctypes.data,
            len(idx), d, *results, infid.ctypes.data, n_failed.ctypes.data)
        assert rc == _lib.FFK_EINVAL
        assert b'idx' in lib.ffk_last_error()
    finally:
        lib.ffk_resident_destroy(handle)

"""ffk_math.h::sin_small, the sine of sincos_small without its cosine, on the host (no GPU): the same operations in
the same order, so the same bits.  The harness tests/csrc/sin_small_host.hip is built by __graft_entry__.build()."""
import ctypes
import os

import numpy as np

from conftest import ROOT

DP = ctypes.POINTER(ctypes.c_double)


def _harness():
    path = os.path.join(ROOT, 'tests', 'csrc', 'libffk_sin_small_host.so')
    assert os.path.exists(path), 'host harness not built: run __graft_entry__.build()'
    return ctypes.CDLL(path)


def _call(fn, x, *more):
    out = np.empty_like(x)
    fn(ctypes.c_long(x.size), x.ctypes.data_as(DP), *more, out.ctypes.data_as(DP))
    return out


def _arguments():
    rng = np.random.default_rng(5)
    tiny = np.nextafter(0.0, 1.0)                                  # the smallest denormal
    special = np.array([0.0, -0.0, tiny, -tiny, 1e-310, -1e-310, 2.0**-1022, -2.0**-1022, 2.0**-5, -2.0**-5,
                        np.nextafter(2.0**-5, 0.0), -np.nextafter(2.0**-5, 0.0)])
    uniform = (rng.random(60000)*2 - 1)*2.0**-5
    decades = (rng.random(40000)*2 - 1)*2.0**-5*10.0**(-16*rng.random(40000))
    return np.concatenate((special, uniform, decades))


def test_sin_small_is_the_sine_of_sincos_small_bit_for_bit():
    lib = _harness()
    x = _arguments()
    assert x.size >= 100000 and np.abs(x).max() == 2.0**-5
    s = _call(lib.ffk_host_sin_small, x)
    ref = _call(lib.ffk_host_sincos_small_sine, x)
    assert np.array_equal(s.view(np.uint64), ref.view(np.uint64))
    # and it is a sine: within an ulp of NumPy's on the whole interval
    err = np.abs(s - np.sin(x))
    assert (err <= np.spacing(np.abs(np.sin(x)))).all()


def test_near_form_of_an_entry():
    """phased_q_near: 2 sin(x dt/2)/x, and dt at x == 0 of either sign."""
    lib = _harness()
    dt = 0.7
    x = np.concatenate(([0.0, -0.0], _arguments()[12:2012]/dt*2))
    q = _call(lib.ffk_host_phased_q_near, x, ctypes.c_double(dt))
    assert q[0] == dt and q[1] == dt
    nz = x != 0
    ref = 2*np.sin(0.5*(x[nz]*dt))/x[nz]
    assert np.abs(q[nz] - ref).max() <= 4*np.spacing(dt)

"""Per-pulse time of the loop against the batched call (ff.infidelities), host clocks around synchronous calls,
one process, warm-up first:
  (a) [ff.infidelity(p, S, omega) for p in fresh pulses]
  (b) ff.infidelities(fresh pulses, S, omega)
  (c) the device time of the batched pass (HIP events around ffk_pipeline_batch_dev on device copies of the inputs)
at config 2 x 64 (workloads.random_pulse_inputs(**CONFIG2), 64 seeds) and config 1 x 4096 (the Hadamard pulse of
workloads.hadamard_pulse with perturbed amplitudes).  Prints one JSON line.

    python tools/time_batch.py [--reps 5] [--only cfg2|cfg1]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import filter_functions_amd as ff  # noqa: E402
import workloads as wl  # noqa: E402
from filter_functions_amd import _lib  # noqa: E402


def config2(P):
    basis = ff.Basis.pauli(2)
    inputs = [wl.random_pulse_inputs(**dict(wl.CONFIG2, seed=1000 + s)) for s in range(P)]
    omega = wl.random_pulse_omega(inputs[0][4], wl.CONFIG2['W'])

    def make():
        return [ff.PulseSequence(list(zip(c, cc)), list(zip(n, nc)), dt, basis) for c, cc, n, nc, dt in inputs]
    return make, omega, 1e-3/omega


def config1(P):
    rng = np.random.default_rng(0)
    X, Y, Z = ff.util.paulis[1:]
    amps = [(np.pi*(1 + 0.01*rng.standard_normal(2)), np.pi/2*(1 + 0.01*rng.standard_normal(2))) for _ in range(P)]
    omega = np.geomspace(1e-2, 1e2, 1000)

    def make():
        return [ff.PulseSequence([[X/2, [0, a[1]]], [Y/2, [b[0], 0]]], [[Z/2, [1, 1]]], [1, 1]) for a, b in amps]
    return make, omega, 1e-3/omega


def device_ms(pulses, omega, S, reps):
    """HIP events around one ffk_pipeline_batch_dev of the whole batch on device-resident inputs."""
    import torch
    lib = _lib.load()
    dev = torch.device('cuda')
    c128 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.complex128)).to(dev)   # noqa: E731
    f64 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)       # noqa: E731
    P, p0 = len(pulses), pulses[0]
    C = c128(np.stack([p.c_opers for p in pulses]))
    cc = f64(np.stack([p.c_coeffs for p in pulses]))
    dt = f64(np.stack([p.dt for p in pulses]))
    t = f64(np.stack([p.t for p in pulses]))
    B = c128(np.stack([p.n_opers for p in pulses]))
    nc = f64(np.stack([p.n_coeffs for p in pulses]))
    om, basis = f64(omega), c128(np.asarray(p0.basis))
    spec = c128(S.astype(np.complex128))
    A, G, d, W, N = len(p0.n_opers), len(p0.dt), p0.d, len(omega), len(p0.basis)
    idx = torch.arange(A, dtype=torch.int32, device=dev)
    F = torch.empty((P, A, A, W), dtype=torch.complex128, device=dev)
    infid = torch.empty((P, A), dtype=torch.float64, device=dev)
    wsb = lib.ffk_pipeline_batch_workspace_bytes(P, W, N, A, G, d, A, 1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    addr = lambda x: x.data_ptr()      # noqa: E731

    def run():
        _lib.check(lib.ffk_pipeline_batch_dev(P, addr(C), len(p0.c_opers), addr(cc), addr(dt), addr(t), G, d,
                                              addr(om), W, addr(basis), N, addr(B), A, addr(nc), addr(spec), 1,
                                              addr(idx), A, None, None, None, None, addr(F), addr(infid),
                                              addr(ws), wsb, stream))
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    _lib.check_kernel_fault()
    return float(np.median(times))


def measure(name, setup, P, reps):
    make, omega, S = setup(P)
    loop, batch = [], []
    for r in range(reps + 1):              # the first round is the warm-up
        pulses = make()
        t0 = time.perf_counter()
        for p in pulses:
            ff.infidelity(p, S, omega)
        t1 = time.perf_counter()
        pulses = make()
        t2 = time.perf_counter()
        ff.infidelities(pulses, S, omega)
        t3 = time.perf_counter()
        if r:
            loop.append(t1 - t0)
            batch.append(t3 - t2)
    dev = device_ms(make(), omega, S, max(5, reps))
    loop_ms, batch_ms = 1e3*np.median(loop)/P, 1e3*np.median(batch)/P
    return {f'{name}_pulses': P, f'{name}_loop_ms_per_pulse': round(loop_ms, 5),
            f'{name}_batch_ms_per_pulse': round(batch_ms, 5),
            f'{name}_device_ms_per_pulse': round(dev/P, 5), f'{name}_speedup': round(loop_ms/batch_ms, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--only', choices=('cfg2', 'cfg1'))
    args = ap.parse_args()
    out = {'device': _lib.device_info()[0]}
    if args.only in (None, 'cfg2'):
        out.update(measure('cfg2', config2, 64, args.reps))
    if args.only in (None, 'cfg1'):
        out.update(measure('cfg1', config1, 4096, args.reps))
    print(json.dumps(out))


if __name__ == '__main__':
    main()

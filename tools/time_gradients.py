"""Per-pulse time of the loop of gradient.infidelity_derivative against ff.infidelity_derivatives; host clocks around
synchronous calls, one process, warm-up first, loop and batch alternating in the same job.  Two timings per workload:
  derivative  on pulses diagonalised OUTSIDE the timed region:
              [gradient.infidelity_derivative(p, S, omega) for p in pulses]   against
              ff.infidelity_derivatives(pulses, S, omega)
  step        an optimiser's step on fresh pulses:
              [(ff.infidelity(p, S, omega), gradient.infidelity_derivative(p, S, omega)) for p in pulses]   against
              ff.infidelities(pulses, S, omega); ff.infidelity_derivatives(pulses, S, omega)
Every repetition of either side gets fresh pulses made outside the timed region, and the previous side's pulses are
freed BEFORE the new ones are made (tools/time_processes.py: the runtime releases the host pages pinned for their
copies at the next synchronisation, time that belongs to the side that made them).  Workloads:
  population  an optimiser's population: 64 pulses of wl.random_pulse_inputs(seed, 2, 100, 2, n_cops=2), 500
              frequencies, spectrum 1e-3/omega
  cfg2        config 2 x 16: d = 4, G = 256, A = 3, H = 3, W = 4096
  population_idle, cfg2_idle
              the same with the amplitudes of every second segment scaled by 1e-9 (the ends of a smooth envelope):
              on those segments every level pair is inside the band |W_mn dt| < theta, where the nested integral comes
              from its series (csrc/ffk_math.h, derivative_integral) and not from the divided difference
Writes one JSON object (medians, ranges, the worst pairing of a loop time with a batched time) to --out (default
profiles/gradients_time.json) and prints it.

    python tools/time_gradients.py [--reps 7] [--only population|cfg2] [--out FILE]

With --trace WORKLOAD --pulses P the tool makes P diagonalised pulses and runs the batched call ONCE: the workload of
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_gradients.py --trace cfg2 --pulses 16
whose rows for the kernels of the pass (gradb_*, grad_batch_kernel, the spectral weights) are
profiles/gradients_kernel_stats.csv: as many launches for P = 2 as for P = 64 (config 2: 16, one pass).
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import filter_functions_amd as ff  # noqa: E402
import workloads as wl  # noqa: E402
from filter_functions_amd import _lib, gradient  # noqa: E402


def population(P=64):
    basis = ff.Basis.pauli(1)
    inputs = [wl.random_pulse_inputs(2000 + s, 2, 100, 2, n_cops=2) for s in range(P)]
    omega = wl.random_pulse_omega(inputs[0][4], 500)
    return inputs, basis, omega, 1e-3/omega


def config2(P=16):
    basis = ff.Basis.pauli(2)
    inputs = [wl.random_pulse_inputs(**dict(wl.CONFIG2, seed=1000 + s)) for s in range(P)]
    omega = wl.random_pulse_omega(inputs[0][4], wl.CONFIG2['W'])
    return inputs, basis, omega, 1e-3/omega


def idle_like(setup):
    def scaled(P=None):
        inputs, basis, omega, S = setup() if P is None else setup(P)
        out = []
        for c, cc, n, nc, dt in inputs:
            cc = np.array(cc, dtype=float)
            cc[:, 1::2] *= 1e-9
            out.append((c, cc, n, nc, dt))
        return out, basis, omega, S
    return scaled


WORKLOADS = {'population': population, 'cfg2': config2,
             'population_idle': idle_like(population), 'cfg2_idle': idle_like(config2)}


def make(inputs, basis, diagonalized):
    pulses = [ff.PulseSequence(list(zip(c, cc)), list(zip(n, nc)), dt, basis) for c, cc, n, nc, dt in inputs]
    if diagonalized:
        for p in pulses:
            p.diagonalize()
    return pulses


def spread(seconds, P):
    ms = 1e3*np.asarray(seconds)/P
    return {'median': round(float(np.median(ms)), 5), 'min': round(float(ms.min()), 5),
            'max': round(float(ms.max()), 5)}


def loop_side(pulses, S, omega, step):
    if step:
        return np.stack([(ff.infidelity(p, S, omega), gradient.infidelity_derivative(p, S, omega))[1] for p in pulses])
    return np.stack([gradient.infidelity_derivative(p, S, omega) for p in pulses])


def batch_side(pulses, S, omega, step):
    if step:
        ff.infidelities(pulses, S, omega)
    return ff.infidelity_derivatives(pulses, S, omega)


def measure(setup, reps, step):
    inputs, basis, omega, S = setup()
    loop, many, worst = [], [], 0.0
    pulses = None
    for r in range(reps + 1):              # the first round is the warm-up
        del pulses
        gc.collect()
        pulses = make(inputs, basis, not step)
        t0 = time.perf_counter()
        ref = loop_side(pulses, S, omega, step)
        t1 = time.perf_counter()
        del pulses
        gc.collect()
        pulses = make(inputs, basis, not step)
        t2 = time.perf_counter()
        got = batch_side(pulses, S, omega, step)
        t3 = time.perf_counter()
        worst = max(worst, float(np.abs(got - ref).max()/np.abs(ref).max()))
        if r:
            loop.append(t1 - t0)
            many.append(t3 - t2)
    P = len(pulses)
    return {'pulses': P, 'n_omega': len(omega), 'repetitions': reps,
            'loop_ms_per_pulse': spread(loop, P), 'batch_ms_per_pulse': spread(many, P),
            'batch_ms_per_call': round(1e3*float(np.median(many)), 4),
            'speedup': round(float(np.median(loop)/np.median(many)), 2),
            'speedup_worst_case': round(float(min(loop)/max(many)), 2),
            'max_rel_difference': worst}


def trace(name, P):
    inputs, basis, omega, S = WORKLOADS[name](P)
    pulses = make(inputs, basis, True)
    ff.infidelity_derivatives(pulses, S, omega)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--only', choices=tuple(WORKLOADS))
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  'profiles', 'gradients_time.json'))
    ap.add_argument('--trace', choices=tuple(WORKLOADS))
    ap.add_argument('--pulses', type=int, default=64)
    args = ap.parse_args()
    if args.trace:
        trace(args.trace, args.pulses)
        return
    out = {'device': _lib.device_info()[0]}
    for name, setup in WORKLOADS.items():
        if args.only in (None, name):
            out[name] = {'derivative': measure(setup, args.reps, False), 'step': measure(setup, args.reps, True)}
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()

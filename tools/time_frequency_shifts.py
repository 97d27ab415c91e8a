"""Per-pulse time of the loop of numeric.calculate_frequency_shifts against ff.frequency_shifts; host clocks around
synchronous calls, one process, warm-up first, loop and batch alternating in the same job:
    [numeric.calculate_frequency_shifts(p, S, omega) for p in pulses]   against   ff.frequency_shifts(pulses, S, omega)
on fresh pulses.  Every repetition of either side gets fresh pulses made outside the timed region, and the previous
side's pulses are freed BEFORE the new ones are made (tools/time_gradients.py).  Workloads, those of that tool:
  population  64 pulses of wl.random_pulse_inputs(seed, 2, 100, 2, n_cops=2), 500 frequencies, spectrum 1e-3/omega
  cfg2        config 2 x 16: d = 4, G = 256, A = 3, W = 4096
Writes one JSON object (medians, ranges, the worst pairing of a loop time with a batched time) to --out (default
profiles/frequency_shifts_time.json) and prints it.

    python tools/time_frequency_shifts.py [--reps 5] [--only population|cfg2] [--out FILE]

FFK_TUNE_SO_SHIFT_TILE=1 in the environment forces the fused kernel's 16 x 16 tile (the tile measurement of DESIGN.md
7.5); give such a run an --out of its own.

With --trace WORKLOAD --pulses P the tool makes P diagonalised pulses and runs the batched call ONCE: the workload of
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_frequency_shifts.py --trace cfg2 --pulses 16
whose rows for the kernels of the pass are profiles/frequency_shifts_kernel_stats.csv: as many launches for P = 2 as
for P = 16.
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import filter_functions_amd as ff  # noqa: E402
from filter_functions_amd import _lib, numeric  # noqa: E402
from time_gradients import config2, make, population, spread  # noqa: E402

WORKLOADS = {'population': population, 'cfg2': config2}


def measure(setup, reps):
    inputs, basis, omega, S = setup()
    loop, many, worst = [], [], 0.0
    pulses = None
    for r in range(reps + 1):              # the first round is the warm-up
        del pulses
        gc.collect()
        pulses = make(inputs, basis, False)
        t0 = time.perf_counter()
        ref = np.stack([numeric.calculate_frequency_shifts(p, S, omega) for p in pulses])
        t1 = time.perf_counter()
        del pulses
        gc.collect()
        pulses = make(inputs, basis, False)
        t2 = time.perf_counter()
        got = ff.frequency_shifts(pulses, S, omega)
        t3 = time.perf_counter()
        scale = np.abs(ref).max(axis=(-2, -1), keepdims=True)
        worst = max(worst, float((np.abs(got - ref)/scale).max()))
        if r:
            loop.append(t1 - t0)
            many.append(t3 - t2)
    P = len(pulses)
    return {'pulses': P, 'n_omega': len(omega), 'repetitions': reps,
            'loop_ms_per_pulse': spread(loop, P), 'batch_ms_per_pulse': spread(many, P),
            'batch_ms_per_call': round(1e3*float(np.median(many)), 4),
            'speedup': round(float(np.median(loop)/np.median(many)), 2),
            'speedup_worst_case': round(float(min(loop)/max(many)), 2),
            'batch_worst_over_loop_median': round(float(max(many)/np.median(loop)), 4),
            'max_rel_difference_per_pair': worst}


def trace(name, P):
    inputs, basis, omega, S = WORKLOADS[name](P)
    pulses = make(inputs, basis, True)
    ff.frequency_shifts(pulses, S, omega)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--only', choices=tuple(WORKLOADS))
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  'profiles', 'frequency_shifts_time.json'))
    ap.add_argument('--trace', choices=tuple(WORKLOADS))
    ap.add_argument('--pulses', type=int, default=16)
    args = ap.parse_args()
    if args.trace:
        trace(args.trace, args.pulses)
        return
    out = {'device': _lib.device_info()[0], 'forced_tile': os.environ.get('FFK_TUNE_SO_SHIFT_TILE')}
    for name, setup in WORKLOADS.items():
        if args.only in (None, name):
            out[name] = measure(setup, args.reps)
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()

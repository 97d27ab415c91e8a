"""Per-pulse time of the loop of ff.error_transfer_matrix against ff.error_transfer_matrices on pulses whose control
matrices are resident in HBM; host clocks around synchronous calls, one process, warm-up first, loop and batch
alternating in the same job:
  (a) [ff.error_transfer_matrix(p, S, omega) for p in members]     (the first read fetches every control matrix)
  (b) ff.error_transfer_matrices(members, S, omega)                (the control matrices are read in place)
Every repetition of either side gets fresh members from a pass OUTSIDE the timed region: a second loop over the
same members would skip the fetch the user pays.  Shapes:
  cfg2   config 2 x 64: members of one ff.get_filter_functions pass (d = 4, A = 3, W = 4096; R totals 201.3 MB)
  study  the randomized-benchmarking study: 1050 results of ff.concatenate_sequences, 301 frequencies
Writes one JSON object (medians and ranges) to --out (default profiles/processes_time.json) and prints it.

    python tools/time_processes.py [--reps 7] [--only cfg2|study] [--out FILE]

With --trace N the tool only runs the batched call of config 2 x 64 N times after a warm-up: the workload of
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_processes.py --trace 20
whose per-kernel table is profiles/processes_kernel_stats.csv (processes_decay_kernel + processes_reduce_kernel
are the decay launch).
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
from filter_functions_amd import _lib  # noqa: E402


def config2(P=64):
    basis = ff.Basis.pauli(2)
    inputs = [wl.random_pulse_inputs(**dict(wl.CONFIG2, seed=1000 + s)) for s in range(P)]
    omega = wl.random_pulse_omega(inputs[0][4], wl.CONFIG2['W'])

    def make():
        pulses = [ff.PulseSequence(list(zip(c, cc)), list(zip(n, nc)), dt, basis) for c, cc, n, nc, dt in inputs]
        ff.get_filter_functions(pulses, omega)
        return pulses
    return make, omega, 1e-3/omega


def study(P=1050):
    omega = wl.rb_omega(301, wl.CONFIG3['T'])
    _, cliffords = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])
    cliffords = np.array(cliffords, dtype=object)
    lengths = np.repeat(np.linspace(2, 152, 21).astype(int), P//21)
    seqs = [cliffords[np.random.default_rng(k).integers(0, 24, m)] for k, m in enumerate(lengths)]

    def make():
        return ff.concatenate_sequences(seqs)
    return make, omega, wl.rb_spectrum(omega, 0.7)


def spread(seconds, P):
    ms = 1e3*np.asarray(seconds)/P
    return {'median': round(float(np.median(ms)), 5), 'min': round(float(ms.min()), 5),
            'max': round(float(ms.max()), 5)}


def measure(name, setup, reps):
    make, omega, S = setup()
    loop, many, worst = [], [], 0.0
    pulses = None
    for r in range(reps + 1):              # the first round is the warm-up
        # the previous side's pulses go BEFORE the new members are made: the loop leaves 64 fetched control matrices
        # behind, and the runtime releases the host pages it pinned for their copies at the next synchronisation
        # after they are freed -- 7 to 16 ms that belong to the loop, not to whatever runs next
        del pulses
        gc.collect()
        pulses = make()
        t0 = time.perf_counter()
        ref = np.stack([ff.error_transfer_matrix(p, S, omega) for p in pulses])
        t1 = time.perf_counter()
        del pulses
        gc.collect()
        pulses = make()
        t2 = time.perf_counter()
        got = ff.error_transfer_matrices(pulses, S, omega)
        t3 = time.perf_counter()
        worst = max(worst, float(np.abs(got - ref).max()))
        if r:
            loop.append(t1 - t0)
            many.append(t3 - t2)
    P = len(pulses)
    out = {'pulses': P, 'n_omega': len(omega), 'repetitions': reps,
           'loop_ms_per_pulse': spread(loop, P), 'batch_ms_per_pulse': spread(many, P),
           'batch_ms_per_call': round(1e3*float(np.median(many)), 4),
           'speedup': round(float(np.median(loop)/np.median(many)), 2),
           'speedup_worst_case': round(float(min(loop)/max(many)), 2),
           'max_abs_difference': worst}
    return {name: out}


def trace(calls):
    make, omega, S = config2()
    pulses = make()
    for _ in range(3 + calls):
        ff.error_transfer_matrices(pulses, S, omega)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--only', choices=('cfg2', 'study'))
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  'profiles', 'processes_time.json'))
    ap.add_argument('--trace', type=int, default=0)
    args = ap.parse_args()
    if args.trace:
        trace(args.trace)
        return
    out = {'device': _lib.device_info()[0]}
    if args.only in (None, 'cfg2'):
        out.update(measure('cfg2x64', config2, args.reps))
    if args.only in (None, 'study'):
        out.update(measure('study', study, args.reps))
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()

"""Time of ff.correlation_infidelities against the loop over ff.infidelity(ff.concatenate(s,
calc_pulse_correlation_FF=True), S, omega, which='correlations') on the randomized-benchmarking study's shape: the 24
Cliffords of workloads.rb_cliffords, 301 frequencies, the 21 lengths 1 ... 151 with the inverting gate appended
(2 ... 152 gates), 50 draws each.  Host clocks around synchronous calls, one process, warm-up first.

The loop makes one library call per gate pair, so it is timed only where it finishes in seconds: the lengths 2, 9, 16
and 31 (the first gates of the study's draws), --draws sequences each.  Loop and batched call alternate on the same
sequences; per length the medians, the worst pairing (fastest loop over slowest batched call) and the largest difference of the results are reported, per
sequence and per gate pair.  The whole study of 1050 sequences goes through the batched call alone and is reported as
a time of its own.  Writes one JSON object to --out (default profiles/correlations_time.json) and prints it.

    python tools/time_correlations.py [--reps 5] [--draws 3] [--out FILE]

With --trace the tool runs the study's batched call ONCE: the workload of
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_correlations.py --trace
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import filter_functions_amd as ff  # noqa: E402
import workloads as wl  # noqa: E402
from filter_functions_amd import _lib  # noqa: E402

LOOP_LENGTHS = (2, 9, 16, 31)


def study(draws=50):
    omega = wl.rb_omega(301, wl.CONFIG3['T'])
    cliffords = np.array(wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])[1], dtype=object)
    lengths = np.linspace(1, 151, 21).astype(int)
    seqs = []
    for k, m in enumerate(np.repeat(lengths, draws)):
        draw = np.random.default_rng(100 + k).integers(0, 24, m)
        U = ff.concatenate_without_filter_function(cliffords[draw]).total_propagator
        inverse = int(np.argmax([abs(np.trace(g.total_propagator @ U)) for g in cliffords]))
        seqs.append(list(cliffords[draw]) + [cliffords[inverse]])
    return omega, cliffords, seqs, wl.rb_spectrum(omega)


def loop(seqs, S, omega):
    return [ff.infidelity(ff.concatenate(s, calc_pulse_correlation_FF=True, omega=omega), S, omega,
                          which='correlations') for s in seqs]


def spread(times, n):
    t = 1e3*np.asarray(times)/n
    return {'median': round(float(np.median(t)), 5), 'min': round(float(t.min()), 5), 'max': round(float(t.max()), 5)}


def measure(reps, draws):
    omega, cliffords, seqs, S = study()
    out = {'n_omega': len(omega), 'repetitions': reps, 'lengths': {}}
    for G in LOOP_LENGTHS:
        some = [s[:G] for s in seqs if len(s) >= G][:draws]      # the first G gates of the study's shortest such draws
        t_loop, t_many, worst = [], [], 0.0
        for r in range(reps + 1):              # the first round is the warm-up
            t0 = time.perf_counter()
            ref = loop(some, S, omega)
            t1 = time.perf_counter()
            got = ff.correlation_infidelities(some, S, omega)
            t2 = time.perf_counter()
            worst = max([worst] + [float(np.abs(g - f).max()/np.abs(f).max()) for g, f in zip(got, ref)])
            if r:
                t_loop.append(t1 - t0)
                t_many.append(t2 - t1)
        n = len(some)
        out['lengths'][str(G)] = {
            'sequences': n, 'loop_ms_per_sequence': spread(t_loop, n), 'batch_ms_per_sequence': spread(t_many, n),
            'loop_us_per_gate_pair': spread(t_loop, n*G*G/1e3), 'batch_us_per_gate_pair': spread(t_many, n*G*G/1e3),
            'speedup': round(float(np.median(t_loop)/np.median(t_many)), 1),
            'speedup_worst_pairing': round(float(min(t_loop)/max(t_many)), 1), 'max_rel_difference': worst}
    whole = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        got = ff.correlation_infidelities(seqs, S, omega)
        whole.append(time.perf_counter() - t0)
    pairs = sum(len(s)**2 for s in seqs)
    out['study'] = {'sequences': len(seqs), 'gate_pairs': pairs, 'seconds': spread(whole[1:], 1e3),
                    'ms_per_sequence': spread(whole[1:], len(seqs)), 'us_per_gate_pair': spread(whole[1:], pairs/1e3),
                    'output_megabytes': round(8*pairs/1e6, 1)}
    del got
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--draws', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'correlations_time.json'))
    ap.add_argument('--trace', action='store_true')
    args = ap.parse_args()
    if args.trace:
        omega, _, seqs, S = study()
        ff.correlation_infidelities(seqs, S, omega)
        return
    out = {'device': _lib.device_info()[0]}
    out.update(measure(args.reps, args.draws))
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()

"""Time of ff.sequence_correlation_infidelities against the routes it replaces on the randomized-benchmarking study's
shape: 301 frequencies, the study's draws (the 21 lengths 1 ... 151 with the inverting gate appended, 50 draws each).
Host clocks around synchronous calls, one process, the routes alternating after a warm-up round; the results are
compared before anything is timed.

  single_qubit   the 24 Cliffords of workloads.rb_cliffords (d = 2): the loop over ff.infidelity(ff.concatenate(...,
                 calc_pulse_correlation_FF=True), which='correlations'), ff.correlation_infidelities and the new call
  two_qubit      the 25 two-qubit gates of tools/time_sequence_infidelities.py (d = 4, Basis.pauli(2), noise on XI and
                 IX): the loop -- the only other route there -- and the new call

The loop makes one library call per gate pair, so the routes are compared at the lengths 2, 9, 16 and 31 (the first
gates of the study's shortest such draws, --draws sequences each).  Per length and route the median of --reps rounds
with its range, the speed-up of the medians and the worst pairing (fastest other route over slowest new call).  The
whole study of 1050 sequences at d = 4 goes through the new call alone.  Writes one JSON object to --out (default
profiles/sequence_correlations_time.json) and prints it.

    python tools/time_sequence_correlations.py [--reps 5] [--draws 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import filter_functions_amd as ff  # noqa: E402
import workloads as wl  # noqa: E402
from filter_functions_amd import _lib  # noqa: E402
from time_sequence_infidelities import study_draws, two_qubit_gate_set  # noqa: E402

LOOP_LENGTHS = (2, 9, 16, 31)
T = wl.CONFIG3['T']


def loop(table, seqs, S, omega):
    return [ff.infidelity(ff.concatenate(table[s], calc_pulse_correlation_FF=True, omega=omega), S, omega,
                          which='correlations') for s in seqs]


def spread(times, n):
    t = 1e3*np.asarray(times)/n
    return {'median': round(float(np.median(t)), 5), 'min': round(float(t.min()), 5), 'max': round(float(t.max()), 5)}


def difference(got, ref):
    return max(float(np.abs(g - f).max()/np.abs(f).max()) for g, f in zip(got, ref))


def compare(routes, n, G, reps):
    """*routes*: {name: callable}, 'new' among them.  The results are compared first (that round is the warm-up),
    then every route runs once per round."""
    results = {name: run() for name, run in routes.items()}
    others = [name for name in routes if name != 'new']
    out = {'sequences': n, 'max_rel_difference': {name: difference(results['new'], results[name]) for name in others}}
    for name, bound in out['max_rel_difference'].items():
        assert bound < 1e-12, (name, G, bound)
    times = {name: [] for name in routes}
    for _ in range(reps):
        for name, run in routes.items():
            t0 = time.perf_counter()
            run()
            times[name].append(time.perf_counter() - t0)
    for name, t in times.items():
        out[name + '_ms_per_sequence'] = spread(t, n)
        out[name + '_us_per_gate_pair'] = spread(t, n*G*G/1e3)
    for name in others:
        out['speedup_over_' + name] = round(float(np.median(times[name])/np.median(times['new'])), 2)
        out['worst_pairing_over_' + name] = round(float(min(times[name])/max(times['new'])), 2)
    return out


def measure(reps, draws):
    omega = wl.rb_omega(301, T)
    S = wl.rb_spectrum(omega)
    cliffords = np.array(wl.rb_cliffords(ff, omega, T)[1], dtype=object)
    seqs = study_draws(cliffords)
    gates = two_qubit_gate_set(omega)
    table = np.array(gates, dtype=object)
    out = {'n_omega': len(omega), 'repetitions': reps, 'single_qubit': {}, 'two_qubit': {'gates': len(gates)}}
    for G in LOOP_LENGTHS:
        some = [s[:G] for s in seqs if len(s) >= G][:draws]
        out['single_qubit'][str(G)] = compare({
            'loop': lambda: loop(cliffords, some, S, omega),
            'correlation_infidelities': lambda: ff.correlation_infidelities([cliffords[s] for s in some], S, omega),
            'new': lambda: ff.sequence_correlation_infidelities(cliffords, some, S, omega)}, len(some), G, reps)
        out['two_qubit'][str(G)] = compare({
            'loop': lambda: loop(table, some, S, omega),
            'new': lambda: ff.sequence_correlation_infidelities(gates, some, S, omega)}, len(some), G, reps)
    whole = []
    for r in range(reps + 1):                  # the first round is the warm-up
        t0 = time.perf_counter()
        got = ff.sequence_correlation_infidelities(gates, seqs, S, omega)
        whole.append(time.perf_counter() - t0)
    pairs = sum(len(s)**2 for s in seqs)
    out['two_qubit']['study'] = {'sequences': len(seqs), 'gate_pairs': pairs, 'seconds': spread(whole[1:], 1e3),
                                 'ms_per_sequence': spread(whole[1:], len(seqs)),
                                 'us_per_gate_pair': spread(whole[1:], pairs/1e3),
                                 'output_megabytes': round(8*pairs/1e6, 1)}
    del got
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--draws', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sequence_correlations_time.json'))
    args = ap.parse_args()
    out = {'device': _lib.device_info()[0]}
    out.update(measure(args.reps, args.draws))
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()

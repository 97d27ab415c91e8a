"""Time of ff.sequence_frequency_shifts against the loop it replaces, on the randomized-benchmarking study's shape
(tools/time_sequence_infidelities.py: 1050 sequences of 2 to 152 gates, 301 frequencies, the two spectra of the
study, white and 1/f^0.7).  Host clocks around synchronous calls (no kernel trace), one process, the routes
alternating, warm-up round first.

  loop           ff.concatenate(gates[s], calc_second_order_FF=True, omega=omega) + numeric.calculate_frequency_shifts
                 per sequence and spectrum: the only other route.  It is timed on every --stride-th sequence (d = 2)
                 and every --stride4-th (d = 4), all lengths among them, on a gate set of its own whose second-order
                 filter functions stay cached from the warm-up round on (warm: the loop at its best).
  new_single     ff.sequence_frequency_shifts, one call per spectrum, on the same subset
  new_stacked    ff.sequence_frequency_shifts(..., stacked=True), one call, on the same subset
  whole study    new_single, new_stacked and ff.sequence_decay_amplitudes(..., stacked=True) on all 1050 sequences,
                 and ff.frequency_shifts of the gate set under both spectra alone: its share of new_stacked

  single_qubit   the 24 Cliffords of workloads.rb_cliffords (d = 2)
  two_qubit      the same draws over the 25 two-qubit gates of tools/time_sequence_infidelities.py (d = 4)

The gate set of the new calls is never touched by the loop, so ff.frequency_shifts takes its batched route in every
round.  Before anything is timed the routes' results are compared per sequence and spectrum (max |difference| / max
|value|) and asserted to agree within the sum of the two routes' bars against extended precision (2e-13 each), and
stacked against single calls bit for bit.  Per shape: medians of --reps rounds with their ranges, the ratio of the
loop to new_stacked and its worst pairing (fastest loop round over slowest new round).  Writes one JSON object to --out
(default profiles/sequence_second_order_time.json) and prints it.

    python tools/time_sequence_second_order.py [--reps 5] [--stride 10] [--stride4 50] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]

import filter_functions_amd as ff  # noqa: E402
import workloads as wl  # noqa: E402
from filter_functions_amd import _lib, numeric  # noqa: E402
from time_sequence_infidelities import T, alternate, spread, study_draws, two_qubit_gate_set  # noqa: E402
from time_sequence_processes import difference  # noqa: E402

AGREE = 4e-13
NEW = ('new_single', 'new_stacked')


def loop(gates, seqs, spectra, omega):
    out = []
    for s in seqs:
        pulse = ff.concatenate(gates[s], calc_second_order_FF=True, omega=omega)
        out.append([numeric.calculate_frequency_shifts(pulse, S, omega) for S in spectra])
    return np.array(out).swapaxes(0, 1)


def single(gates, seqs, spectra, omega):
    return np.array([ff.sequence_frequency_shifts(gates, seqs, S, omega) for S in spectra])


def stacked(gates, seqs, spectra, omega):
    return ff.sequence_frequency_shifts(gates, seqs, np.stack(spectra), omega, stacked=True)


def decay(gates, seqs, spectra, omega):
    return ff.sequence_decay_amplitudes(gates, seqs, np.stack(spectra), omega, stacked=True)


def own_shifts(gates, seqs, spectra, omega):
    return np.array([ff.frequency_shifts(gates, S, omega) for S in spectra])


def shape(gates, loop_gates, seqs, stride, spectra, omega, reps):
    some = seqs[::stride]
    table = np.array(loop_gates, dtype=object)
    routes = {'loop': lambda: loop(table, some, spectra, omega),
              'new_single': lambda: single(gates, some, spectra, omega),
              'new_stacked': lambda: stacked(gates, some, spectra, omega)}
    results = {name: run() for name, run in routes.items()}
    assert np.array_equal(results['new_single'], results['new_stacked']), 'stacked and single calls differ in bits'
    agreement = difference(results['new_stacked'], results['loop'])
    assert agreement < AGREE, agreement
    times = alternate(routes, reps)[0]
    new = times['new_stacked']
    out = {'gates': len(gates), 'stride': stride, 'sequences': len(some), 'loop_second_order_caches': 'warm',
           'seconds': {name: spread(t) for name, t in times.items()},
           'speedup': round(float(np.median(times['loop'])/np.median(new)), 2),
           'speedup_worst_pairing': round(float(min(times['loop'])/max(new)), 2),
           'speedup_single_calls_worst_pairing': round(float(min(times['loop'])/max(times['new_single'])), 2),
           'max_rel_difference': agreement}
    whole = alternate({name: (lambda run=run: run(gates, seqs, spectra, omega))
                       for name, run in (('new_single', single), ('new_stacked', stacked),
                                         ('decay_amplitudes_stacked', decay), ('gate_frequency_shifts', own_shifts))},
                      reps)[0]
    median = {name: float(np.median(t)) for name, t in whole.items()}
    out['whole_study'] = {'sequences': len(seqs), 'seconds': {name: spread(t) for name, t in whole.items()},
                          'single_calls_over_stacked': round(median['new_single']/median['new_stacked'], 2),
                          'over_decay_amplitudes': round(median['new_stacked']/median['decay_amplitudes_stacked'], 2),
                          'share_of_gate_frequency_shifts':
                              round(median['gate_frequency_shifts']/median['new_stacked'], 2),
                          'loop_extrapolated_seconds': round(float(np.median(times['loop']))*len(seqs)/len(some), 2)}
    return out


def measure(reps, stride, stride4):
    omega = wl.rb_omega(301, T)
    spectra = [wl.rb_spectrum(omega, 0.0), wl.rb_spectrum(omega, 0.7)]
    cliffords = np.array(wl.rb_cliffords(ff, omega, T)[1], dtype=object)
    seqs = study_draws(cliffords)
    out = {'n_omega': len(omega), 'repetitions': reps, 'spectra': len(spectra),
           'positions': int(sum(len(s) for s in seqs)), 'agreement_bar': AGREE,
           'clock': 'host clocks around synchronous calls'}
    out['single_qubit'] = shape(list(wl.rb_cliffords(ff, omega, T)[1]), list(cliffords), seqs, stride, spectra, omega,
                                reps)
    out['two_qubit'] = shape(two_qubit_gate_set(omega), two_qubit_gate_set(omega), seqs, stride4, spectra, omega, reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--stride', type=int, default=10)
    ap.add_argument('--stride4', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sequence_second_order_time.json'))
    args = ap.parse_args()
    out = {'device': _lib.device_info()[0]}
    out.update(measure(args.reps, args.stride, args.stride4))
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()

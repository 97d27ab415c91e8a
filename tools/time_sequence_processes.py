"""Time of ff.sequence_decay_amplitudes against the routes it replaces, on the randomized-benchmarking study's shape
(tools/time_sequence_infidelities.py: 1050 sequences of 2 to 152 gates, 301 frequencies, the two spectra of the
study, white and 1/f^0.7).  Host clocks around synchronous calls, one process, the routes alternating, warm-up first.

  loop                   ff.concatenate + numeric.calculate_decay_amplitudes per sequence and spectrum
  concatenate_sequences  d = 2 only: ff.decay_amplitudes(ff.concatenate_sequences(...), S, omega) per spectrum
  new_single             ff.sequence_decay_amplitudes, one call per spectrum
  new_stacked            ff.sequence_decay_amplitudes(..., stacked=True), one call

  single_qubit   the 24 Cliffords of workloads.rb_cliffords (d = 2): every route on the whole study
  two_qubit      the same draws over the 25 two-qubit gates of tools/time_sequence_infidelities.py (d = 4).  The only
                 other route is the loop; it is timed on every --stride-th sequence (105 by default, all lengths),
                 alternating with the new calls on the same subset; the new calls' times for the whole study are
                 reported next to it.

Before anything is timed the routes' results are compared per sequence and spectrum (max |difference| / max |value|)
and asserted to agree within the sum of the two routes' bars against extended precision (2e-13 each below 500
positions).  Per shape: medians of --reps rounds with their ranges, the ratio of the fastest other route to
new_stacked, the worst pairing (fastest round of the other route over slowest round of new_stacked), and new_single
over new_stacked: what forming Gamma for every spectrum in one walk buys.  Writes one JSON object to --out (default
profiles/sequence_processes_time.json) and prints it.

    python tools/time_sequence_processes.py [--reps 5] [--stride 10] [--out FILE]
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

AGREE = 4e-13
NEW = ('new_single', 'new_stacked')


def loop(gates, seqs, spectra, omega):
    out = []
    for s in seqs:
        pulse = ff.concatenate(gates[s], omega=omega)
        out.append([numeric.calculate_decay_amplitudes(pulse, S, omega) for S in spectra])
    return np.array(out).swapaxes(0, 1)


def batched(gates, seqs, spectra, omega):
    pulses = ff.concatenate_sequences([gates[s] for s in seqs])
    return np.array([ff.decay_amplitudes(pulses, S, omega) for S in spectra])


def single(gates, seqs, spectra, omega):
    return np.array([ff.sequence_decay_amplitudes(gates, seqs, S, omega) for S in spectra])


def stacked(gates, seqs, spectra, omega):
    return ff.sequence_decay_amplitudes(gates, seqs, np.stack(spectra), omega, stacked=True)


def difference(a, b):
    """The largest relative difference of two results (K, P, ...) per sequence and spectrum."""
    a, b = a.reshape(a.shape[:2] + (-1,)), b.reshape(b.shape[:2] + (-1,))
    return float((np.abs(a - b).max(axis=-1)/np.abs(b).max(axis=-1)).max())


def compare(routes):
    results = {name: run() for name, run in routes.items()}
    others = [name for name in routes if name not in NEW]
    assert np.array_equal(results['new_single'], results['new_stacked']), 'stacked and single calls differ in bits'
    found = {name: difference(results['new_stacked'], results[name]) for name in others}
    assert max(found.values()) < AGREE, found
    return found


def report(times, agreement, n):
    others = [name for name in times if name not in NEW]
    fastest = min(others, key=lambda name: np.median(times[name]))
    new = times['new_stacked']
    return {'sequences': n, 'seconds': {name: spread(t) for name, t in times.items()}, 'fastest_other_route': fastest,
            'speedup': round(float(np.median(times[fastest])/np.median(new)), 2),
            'speedup_worst_pairing': round(float(min(min(times[name]) for name in others)/max(new)), 2),
            'single_calls_over_stacked': round(float(np.median(times['new_single'])/np.median(new)), 2),
            'single_calls_over_stacked_worst_pairing': round(float(min(times['new_single'])/max(new)), 2),
            'max_rel_difference': agreement}


def measure(reps, stride):
    omega = wl.rb_omega(301, T)
    spectra = [wl.rb_spectrum(omega, 0.0), wl.rb_spectrum(omega, 0.7)]
    cliffords = np.array(wl.rb_cliffords(ff, omega, T)[1], dtype=object)
    seqs = study_draws(cliffords)
    out = {'n_omega': len(omega), 'repetitions': reps, 'spectra': len(spectra),
           'positions': int(sum(len(s) for s in seqs)), 'agreement_bar': AGREE}
    routes = {'loop': lambda: loop(cliffords, seqs, spectra, omega),
              'concatenate_sequences': lambda: batched(cliffords, seqs, spectra, omega),
              'new_single': lambda: single(cliffords, seqs, spectra, omega),
              'new_stacked': lambda: stacked(cliffords, seqs, spectra, omega)}
    agreement = compare(routes)
    out['single_qubit'] = report(alternate(routes, reps)[0], agreement, len(seqs))
    gates = two_qubit_gate_set(omega)
    table = np.array(gates, dtype=object)
    some = seqs[::stride]
    routes = {'loop': lambda: loop(table, some, spectra, omega),
              'new_single': lambda: single(gates, some, spectra, omega),
              'new_stacked': lambda: stacked(gates, some, spectra, omega)}
    agreement = compare(routes)
    out['two_qubit'] = dict(report(alternate(routes, reps)[0], agreement, len(some)), gates=len(gates), stride=stride)
    whole, _ = alternate({name: (lambda run=run: run(gates, seqs, spectra, omega))
                          for name, run in (('new_single', single), ('new_stacked', stacked))}, reps)
    out['two_qubit']['whole_study'] = {'sequences': len(seqs),
                                       'seconds': {name: spread(t) for name, t in whole.items()}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--stride', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sequence_processes_time.json'))
    args = ap.parse_args()
    out = {'device': _lib.device_info()[0]}
    out.update(measure(args.reps, args.stride))
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()

"""Time of ff.sequence_prefix_infidelities and ff.sequence_prefix_decay_amplitudes against the routes they replace, on
the randomized-benchmarking study's shape (tools/time_sequence_infidelities.py: 1050 sequences of 2 to 152 gates, 301
frequencies, the two spectra of the study, white and 1/f^0.7, stacked) and on three sequences each of 2, 16, 31 and
152 gates.  Host clocks around synchronous calls, one process, the routes alternating, warm-up first.

  prefixes_as_sequences  every truncation of every sequence handed to ff.sequence_infidelities (one call per spectrum)
                         and ff.sequence_decay_amplitudes (stacked) as a sequence of its own: G (G + 1) / 2 positions
                         per sequence.  The index arrays are built before the clock starts
  loop                   ff.concatenate per truncation, ff.infidelity and numeric.calculate_decay_amplitudes per
                         spectrum; on the study timed on every --stride-th sequence (all lengths), alternating with
                         the other routes on the same subset
  new                    ff.sequence_prefix_infidelities and ff.sequence_prefix_decay_amplitudes, stacked, one call each

  single_qubit   the 24 Cliffords of workloads.rb_cliffords (d = 2)
  two_qubit      the same draws over the 25 two-qubit gates of tools/time_sequence_infidelities.py (d = 4)

Before anything is timed the routes' results are compared per position and spectrum (max |difference| / max |value|
over the curve) and asserted to agree within the sum of the two routes' bars against extended precision (2e-13 each
below 500 positions).  Per shape: medians of --reps rounds with their ranges, the ratio of the fastest other route
to the new calls and the worst pairing (fastest round of the other route over slowest round of the new calls).  The
new calls are also timed one by one (infidelities, diagonal, decay amplitudes) on the whole study: what storing and
adding the per-position tiles costs next to the walk alone.  Writes one JSON object to --out (default
profiles/sequence_prefixes_time.json) and prints it.

    python tools/time_sequence_prefixes.py [--reps 5] [--stride 50] [--out FILE]
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
LENGTHS = (2, 16, 31, 152)


def truncations(seqs):
    return [np.asarray(s[:m]) for s in seqs for m in range(1, len(s) + 1)]


def as_sequences(gates, flat, spectra, omega):
    infid = np.array([ff.sequence_infidelities(gates, flat, S, omega) for S in spectra])
    return infid, ff.sequence_decay_amplitudes(gates, flat, np.stack(spectra), omega, stacked=True)


def loop(table, seqs, spectra, omega):
    infid, gamma = [], []
    for s in seqs:
        for m in range(1, len(s) + 1):
            pulse = ff.concatenate(table[s[:m]], omega=omega)
            infid.append([ff.infidelity(pulse, S, omega) for S in spectra])
            gamma.append([numeric.calculate_decay_amplitudes(pulse, S, omega) for S in spectra])
    return np.array(infid).swapaxes(0, 1), np.array(gamma).swapaxes(0, 1)


def new(gates, seqs, spectra, omega):
    S = np.stack(spectra)
    return (ff.sequence_prefix_infidelities(gates, seqs, S, omega, stacked=True),
            ff.sequence_prefix_decay_amplitudes(gates, seqs, S, omega, stacked=True))


def difference(curves, b, seqs):
    """The largest relative difference of the new calls' curves (one (K, G, ...) array per sequence) from another
    route's result (K, n_index, ...), per sequence and spectrum (over its curve)."""
    worst, at = 0.0, 0
    for s, a in zip(seqs, curves):
        x, y = a.reshape(len(a), -1), b[:, at:at + len(s)].reshape(len(b), -1)
        worst = max(worst, float((np.abs(x - y).max(axis=-1)/np.abs(y).max(axis=-1)).max()))
        at += len(s)
    return worst


def compare(routes, seqs):
    results = {name: run() for name, run in routes.items()}
    found = {name: max(difference(results['new'][n], results[name][n], seqs) for n in range(2))
             for name in routes if name != 'new'}
    assert max(found.values()) < AGREE, found
    return found


def report(times, agreement, seqs):
    others = [name for name in times if name != 'new']
    fastest = min(others, key=lambda name: np.median(times[name]))
    return {'sequences': len(seqs), 'positions': int(sum(len(s) for s in seqs)),
            'positions_as_sequences': int(sum(len(s)*(len(s) + 1)//2 for s in seqs)),
            'seconds': {name: spread(t) for name, t in times.items()}, 'fastest_other_route': fastest,
            'speedup': round(float(np.median(times[fastest])/np.median(times['new'])), 2),
            'speedup_worst_pairing': round(float(min(min(times[name]) for name in others)/max(times['new'])), 2),
            'max_rel_difference': agreement}


def shape(gates, seqs, spectra, omega, reps, with_loop=True):
    table = np.array(gates, dtype=object)
    flat = truncations(seqs)
    routes = {'prefixes_as_sequences': lambda: as_sequences(gates, flat, spectra, omega)}
    if with_loop:
        routes['loop'] = lambda: loop(table, seqs, spectra, omega)
    routes['new'] = lambda: new(gates, seqs, spectra, omega)
    agreement = compare(routes, seqs)
    return report(alternate(routes, reps)[0], agreement, seqs)


def modes(gates, seqs, spectra, omega, reps):
    S = np.stack(spectra)
    routes = {'infidelities': lambda: ff.sequence_prefix_infidelities(gates, seqs, S, omega, stacked=True),
              'diagonal': lambda: ff.sequence_prefix_decay_amplitudes(gates, seqs, S, omega, diagonal=True,
                                                                      stacked=True),
              'decay_amplitudes': lambda: ff.sequence_prefix_decay_amplitudes(gates, seqs, S, omega, stacked=True)}
    return {name: spread(t) for name, t in alternate(routes, reps)[0].items()}


def measure(reps, stride):
    omega = wl.rb_omega(301, T)
    spectra = [wl.rb_spectrum(omega, 0.0), wl.rb_spectrum(omega, 0.7)]
    cliffords = list(wl.rb_cliffords(ff, omega, T)[1])
    seqs = study_draws(np.array(cliffords, dtype=object))
    out = {'n_omega': len(omega), 'repetitions': reps, 'spectra': len(spectra), 'agreement_bar': AGREE,
           'stride': stride}
    for name, gates in (('single_qubit', cliffords), ('two_qubit', two_qubit_gate_set(omega))):
        print(f'{name}: the whole study', file=sys.stderr, flush=True)
        entry = {'gates': len(gates), 'whole_study': shape(gates, seqs, spectra, omega, reps, with_loop=False)}
        entry['whole_study']['new_calls_one_by_one'] = modes(gates, seqs, spectra, omega, reps)
        print(f'{name}: every {stride}th sequence', file=sys.stderr, flush=True)
        entry['subset'] = shape(gates, seqs[::stride], spectra, omega, reps)
        for G in LENGTHS:
            print(f'{name}: three sequences of {G} gates', file=sys.stderr, flush=True)
            three = [np.random.default_rng(7*G + k).integers(0, 24, G) for k in range(3)]
            entry[f'length_{G}'] = shape(gates, three, spectra, omega, reps)
        out[name] = entry
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--stride', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sequence_prefixes_time.json'))
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

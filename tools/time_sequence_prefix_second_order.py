"""Time of ff.sequence_prefix_frequency_shifts against the routes it replaces, on the randomized-benchmarking study's
shape (tools/time_sequence_infidelities.py: 1050 sequences of 2 to 152 gates, 301 frequencies, the two spectra of the
study, white and 1/f^0.7, stacked) and on three sequences each of 2, 16, 31 and 152 gates, every truncation closed by a
gate of its own.  Host clocks around synchronous calls, one process, the routes alternating, warm-up first.

  truncations_as_sequences  every truncation of every sequence, its closing gate appended, handed to
                            ff.sequence_frequency_shifts (stacked) as a sequence of its own: G (G + 3) / 2 positions
                            per sequence.  The index arrays are built before the clock starts.  On the two-qubit study
                            timed on every --stride-sequences-th sequence, alternating with the new call on that subset
  loop                      ff.concatenate(..., calc_second_order_FF=True) per truncation and
                            numeric.calculate_frequency_shifts per spectrum; timed on the three sequences of 2, 16 and
                            31 gates and on every --stride-loop-th sequence of the study (one round after the warm-up)
  new                       ff.sequence_prefix_frequency_shifts, stacked, one call

  single_qubit   the 24 Cliffords of workloads.rb_cliffords (d = 2), every truncation closed by its inverse
  two_qubit      the same draws over the 25 two-qubit gates of tools/time_sequence_infidelities.py (d = 4), closed by
                 drawn gates (the set is no group)

Before anything is timed the routes' results are compared per sequence and spectrum (max |difference| / max |value|
over the curve) and asserted to agree within the sum of the two routes' bars against extended precision (2e-13 each
below 500 positions; 1e-12 against the loop).  Per row: medians of --reps rounds with their ranges, the ratio of the
fastest other route to the new call and the worst pairing (fastest round of the other route over slowest round of the
new call).  Writes one JSON object to --out (default profiles/sequence_prefix_second_order_time.json), rewritten after
every row, and prints it.

    python tools/time_sequence_prefix_second_order.py [--reps 5] [--stride-loop 350] [--stride-sequences 10] [--out FILE]
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
AGREE_LOOP = 1e-12
LENGTHS = (2, 16, 31, 152)


def truncations(seqs, close):
    return [np.append(s[:m], c[m - 1]) for s, c in zip(seqs, close) for m in range(1, len(s) + 1)]


def as_sequences(gates, flat, spectra, omega):
    return ff.sequence_frequency_shifts(gates, flat, np.stack(spectra), omega, stacked=True)


def loop(table, seqs, close, spectra, omega):
    out = []
    for s, c in zip(seqs, close):
        for m in range(1, len(s) + 1):
            pulse = ff.concatenate(list(table[s[:m]]) + [table[c[m - 1]]], calc_second_order_FF=True, omega=omega)
            out.append([numeric.calculate_frequency_shifts(pulse, S, omega) for S in spectra])
    return np.array(out).swapaxes(0, 1)


def new(gates, seqs, close, spectra, omega):
    return ff.sequence_prefix_frequency_shifts(gates, seqs, np.stack(spectra), omega, closing=close, stacked=True)


def difference(curves, b, seqs):
    """The largest relative difference of the new call's curves (one (K, G, ...) array per sequence) from another
    route's result (K, n_index, ...), per sequence and spectrum (over its curve)."""
    worst, at = 0.0, 0
    for s, a in zip(seqs, curves):
        x, y = a.reshape(len(a), -1), b[:, at:at + len(s)].reshape(len(b), -1)
        worst = max(worst, float((np.abs(x - y).max(axis=-1)/np.abs(y).max(axis=-1)).max()))
        at += len(s)
    return worst


def report(times, agreement, seqs):
    others = [name for name in times if name != 'new']
    fastest = min(others, key=lambda name: np.median(times[name]))
    return {'sequences': len(seqs), 'positions': int(sum(len(s) for s in seqs)),
            'positions_as_sequences': int(sum(len(s)*(len(s) + 3)//2 for s in seqs)),
            'seconds': {name: spread(t) for name, t in times.items()}, 'fastest_other_route': fastest,
            'speedup': round(float(np.median(times[fastest])/np.median(times['new'])), 2),
            'speedup_worst_pairing': round(float(min(min(times[name]) for name in others)/max(times['new'])), 2),
            'max_rel_difference': agreement}


def shape(gates, seqs, close, spectra, omega, reps, with_sequences=True, with_loop=False):
    table = np.array(gates, dtype=object)
    routes = {}
    if with_sequences:
        flat = truncations(seqs, close)
        routes['truncations_as_sequences'] = lambda: as_sequences(gates, flat, spectra, omega)
    if with_loop:
        routes['loop'] = lambda: loop(table, seqs, close, spectra, omega)
    routes['new'] = lambda: new(gates, seqs, close, spectra, omega)
    # the results first: nothing is timed before the routes agree
    results = {name: run() for name, run in routes.items()}
    agreement = {name: difference(results['new'], results[name], seqs) for name in routes if name != 'new'}
    for name, found in agreement.items():
        assert found < (AGREE_LOOP if name == 'loop' else AGREE), agreement
    del results
    return report(alternate(routes, reps)[0], agreement, seqs)


def closing_gates(gates, seqs, group):
    """The gate behind every truncation: its inverse in a group, else a drawn one."""
    if not group:
        return [np.random.default_rng(500 + p).integers(0, len(gates), len(s)) for p, s in enumerate(seqs)]
    U = np.array([np.asarray(g.total_propagator) for g in gates])
    return [np.abs(np.einsum('cab,mba->mc', U, total)).argmax(axis=1)
            for total in ff.sequence_prefix_propagators(gates, seqs)]


def measure(reps, stride_loop, stride_sequences, write):
    omega = wl.rb_omega(301, T)
    spectra = [wl.rb_spectrum(omega, 0.0), wl.rb_spectrum(omega, 0.7)]
    cliffords = list(wl.rb_cliffords(ff, omega, T)[1])
    # (the study's draws without the inverting gate it appends: here every truncation gets its own)
    seqs = [s[:-1] for s in study_draws(np.array(cliffords, dtype=object))]
    out = {'n_omega': len(omega), 'repetitions': reps, 'spectra': len(spectra), 'agreement_bar': AGREE,
           'agreement_bar_loop': AGREE_LOOP, 'stride_loop': stride_loop, 'stride_sequences': stride_sequences}
    for name, gates in (('single_qubit', cliffords), ('two_qubit', two_qubit_gate_set(omega))):
        group = name == 'single_qubit'
        close = closing_gates(gates, seqs, group)
        entry = {'gates': len(gates)}
        out[name] = entry
        for G in LENGTHS:
            print(f'{name}: three sequences of {G} gates', file=sys.stderr, flush=True)
            three = [np.random.default_rng(7*G + k).integers(0, 24, G) for k in range(3)]
            entry[f'length_{G}'] = shape(gates, three, closing_gates(gates, three, group), spectra, omega, reps,
                                         with_loop=G < 152)
            write(out)
        print(f'{name}: the whole study', file=sys.stderr, flush=True)
        if group:
            entry['whole_study'] = shape(gates, seqs, close, spectra, omega, reps)
        else:
            # the new call on the whole study, and both routes on every stride_sequences-th sequence
            whole = alternate({'new': lambda: new(gates, seqs, close, spectra, omega)}, reps)[0]
            entry['whole_study'] = {'sequences': len(seqs), 'positions': int(sum(len(s) for s in seqs)),
                                    'seconds': {'new': spread(whole['new'])}}
            write(out)
            entry['whole_study_subset'] = shape(gates, seqs[::stride_sequences], close[::stride_sequences], spectra,
                                                omega, reps)
        write(out)
        print(f'{name}: the loop on every {stride_loop}th sequence', file=sys.stderr, flush=True)
        entry['loop_subset'] = shape(gates, seqs[::stride_loop], close[::stride_loop], spectra, omega, 1,
                                     with_sequences=False, with_loop=True)
        write(out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--stride-loop', type=int, default=350)
    ap.add_argument('--stride-sequences', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sequence_prefix_second_order_time.json'))
    args = ap.parse_args()
    head = {'device': _lib.device_info()[0]}

    def write(out):
        if args.out:
            with open(args.out, 'w') as fh:
                fh.write(json.dumps({**head, **out}, indent=1) + '\n')
    out = measure(args.reps, args.stride_loop, args.stride_sequences, write)
    write(out)
    print(json.dumps({**head, **out}))


if __name__ == '__main__':
    main()

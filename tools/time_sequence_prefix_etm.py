"""Time of ff.sequence_prefix_error_transfer_matrices against the parent's only route to the same matrices, and of the
batched exponential alone against the loop over the single one.  Conventions of
tools/time_sequence_prefix_second_order.py: 301 frequencies, the study's two spectra (white and 1/f^0.7) stacked, the
routes alternating in one process after a warm-up round, medians of --reps rounds with their ranges, host clocks around
synchronous calls, results compared before anything is timed.

  parent  ff.sequence_prefix_cumulant_functions(..., stacked=True), then the Python loop over
          numeric.error_transfer_matrix(cumulant_function=k) for every position and spectrum (one ffk_expm_real each)
  new     ff.sequence_prefix_error_transfer_matrices(..., stacked=True), one call

  single_qubit   the 24 Cliffords of workloads.rb_cliffords (d = 2, N = 4: one matrix per lane)
  two_qubit      the 25 two-qubit gates of tools/time_sequence_infidelities.py (d = 4, N = 16: one matrix per wavefront)

Shapes: three sequences of 16 and of 152 gates, first and second order; the whole study (1050 sequences of 1 to 151
gates) with the new call alone, and both routes alternating on every --stride-sequences-th sequence of it.

The exponential alone: 160 000 tiles of 4 x 4 and 16 000 of 16 x 16 (random, 1-norms between 1e-3 and 3) through
ffk_expm_real_batch, against the loop over ffk_expm_real on every --stride-matrices-th of them; the loop's time is
reported as measured (on the subsample) and per matrix.

Per row: medians with ranges, the ratio parent / new and the worst pairing (fastest round of the parent over slowest
round of the new call).  Writes one JSON object to --out (default profiles/sequence_prefix_etm_time.json), rewritten
after every row, and prints it.

    python tools/time_sequence_prefix_etm.py [--reps 5] [--stride-sequences 50] [--stride-matrices 100] [--out FILE]
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

AGREE = 1e-12          # max|U - U'| against max|U' - I|: the bar of the tests against the loop
LENGTHS = (16, 152)


def parent(gates, seqs, spectra, omega, second_order):
    K = ff.sequence_prefix_cumulant_functions(gates, seqs, np.stack(spectra), omega, second_order=second_order,
                                              stacked=True)
    return [np.array([[numeric.error_transfer_matrix(cumulant_function=k) for k in per_spectrum]
                      for per_spectrum in curve]) for curve in K]


def new(gates, seqs, spectra, omega, second_order):
    return ff.sequence_prefix_error_transfer_matrices(gates, seqs, np.stack(spectra), omega,
                                                      second_order=second_order, stacked=True)


def difference(a, b):
    """The largest max|U - U'| / max|U' - I| over all matrices of two results."""
    worst = 0.0
    for x, y in zip(a, b):
        N = x.shape[-1]
        x, y = x.reshape(-1, N, N), y.reshape(-1, N, N)
        worst = max(worst, float((np.abs(x - y).max(axis=(1, 2))/np.abs(y - np.eye(N)).max(axis=(1, 2))).max()))
    return worst


def report(times, extra):
    return {**extra, 'seconds': {name: spread(t) for name, t in times.items()},
            'speedup': round(float(np.median(times['parent'])/np.median(times['new'])), 2),
            'speedup_worst_pairing': round(float(min(times['parent'])/max(times['new'])), 2)}


def shape(gates, seqs, spectra, omega, reps, second_order):
    routes = {'parent': lambda: parent(gates, seqs, spectra, omega, second_order),
              'new': lambda: new(gates, seqs, spectra, omega, second_order)}
    # the results first: nothing is timed before the routes agree
    agreement = difference(routes['new'](), routes['parent']())
    assert agreement < AGREE, agreement
    positions = int(sum(len(s) for s in seqs))
    return report(alternate(routes, reps)[0], {'sequences': len(seqs), 'positions': positions,
                                               'matrices': positions*len(spectra), 'second_order': second_order,
                                               'max_difference': agreement})


def exponential_alone(n, N, stride, reps):
    rng = np.random.default_rng(N)
    tiles = rng.standard_normal((n, 1, N, N))
    norms = np.exp(rng.uniform(np.log(1e-3), np.log(3.0), n))
    tiles *= (norms/np.abs(tiles[:, 0]).sum(axis=1).max(axis=1))[:, None, None, None]
    lib = _lib.load()
    out, flags = np.empty((n, N, N)), np.empty(n, dtype=np.int32)
    subset = np.ascontiguousarray(tiles[::stride, 0])
    singles = np.empty_like(subset)

    def batched():
        _lib.check(lib.ffk_expm_real_batch(tiles.ctypes.data, n, 1, N, out.ctypes.data, flags.ctypes.data))

    def loop():
        for k, u in zip(subset, singles):
            _lib.check(lib.ffk_expm_real(k.ctypes.data, N, u.ctypes.data))
    batched()
    loop()
    assert not flags.any()
    agreement = difference([out[::stride]], [singles])
    assert agreement < AGREE, agreement
    times = alternate({'parent': loop, 'new': batched}, reps)[0]
    row = report(times, {'matrices': n, 'N': N, 'matrices_in_the_loop': len(subset), 'stride': stride,
                         'max_difference': agreement})
    per = {'parent': float(np.median(times['parent'])/len(subset)), 'new': float(np.median(times['new'])/n)}
    row['seconds_per_matrix'] = per
    row['speedup_per_matrix'] = round(per['parent']/per['new'], 1)
    return row


def measure(reps, stride_sequences, stride_matrices, write):
    omega = wl.rb_omega(301, T)
    spectra = [wl.rb_spectrum(omega, 0.0), wl.rb_spectrum(omega, 0.7)]
    cliffords = list(wl.rb_cliffords(ff, omega, T)[1])
    seqs = [s[:-1] for s in study_draws(np.array(cliffords, dtype=object))]
    out = {'n_omega': len(omega), 'repetitions': reps, 'spectra': len(spectra), 'agreement_bar': AGREE,
           'stride_sequences': stride_sequences, 'stride_matrices': stride_matrices}
    for name, gates in (('single_qubit', cliffords), ('two_qubit', two_qubit_gate_set(omega))):
        entry = {'gates': len(gates)}
        out[name] = entry
        for G in LENGTHS:
            three = [np.random.default_rng(7*G + k).integers(0, 24, G) for k in range(3)]
            for second_order in (False, True):
                print(f'{name}: three sequences of {G} gates, second_order={second_order}', file=sys.stderr, flush=True)
                entry[f'length_{G}' + ('_second_order' if second_order else '')] = shape(gates, three, spectra, omega,
                                                                                        reps, second_order)
                write(out)
        print(f'{name}: the whole study', file=sys.stderr, flush=True)
        whole = alternate({'new': lambda: new(gates, seqs, spectra, omega, True)}, reps)[0]
        entry['whole_study_second_order'] = {'sequences': len(seqs), 'positions': int(sum(len(s) for s in seqs)),
                                             'seconds': {'new': spread(whole['new'])}}
        write(out)
        entry['whole_study_subset_second_order'] = shape(gates, seqs[::stride_sequences], spectra, omega, reps, True)
        write(out)
    for n, N in ((160000, 4), (16000, 16)):
        print(f'the exponential alone: {n} tiles of {N} x {N}', file=sys.stderr, flush=True)
        out[f'exponential_{N}x{N}'] = exponential_alone(n, N, stride_matrices, reps)
        write(out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--stride-sequences', type=int, default=50)
    ap.add_argument('--stride-matrices', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sequence_prefix_etm_time.json'))
    args = ap.parse_args()
    head = {'device': _lib.device_info()[0]}

    def write(out):
        if args.out:
            with open(args.out, 'w') as fh:
                fh.write(json.dumps({**head, **out}, indent=1) + '\n')
    out = measure(args.reps, args.stride_sequences, args.stride_matrices, write)
    write(out)
    print(json.dumps({**head, **out}))


if __name__ == '__main__':
    main()

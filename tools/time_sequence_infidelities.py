"""Time of ff.sequence_infidelities against the two routes it replaces, the loop over ff.infidelity(ff.concatenate(...))
and ff.infidelities(ff.concatenate_sequences(...)), on the randomized-benchmarking study's shape: 1050 sequences of 2
to 152 gates (the 21 lengths 1 ... 151 with the inverting gate appended, 50 draws each), 301 frequencies, two spectra
(white and 1/f^0.7).  Host clocks around synchronous calls, one process, the routes alternating, warm-up first.

  single_qubit   the 24 Cliffords of workloads.rb_cliffords (d = 2): all three routes on the whole study
  two_qubit      the same draws over 25 two-qubit gates in Basis.pauli(2) (d = 4): X/2 and Y/2 on either qubit, a
                 ZZ-coupled entangler and their 20 ordered products by `@`, noise on XI and IX.  The only other route
                 is the loop; it is timed on every --stride-th sequence of the study (105 sequences by default, all
                 lengths), alternating with the new call on the same subset; the new call's time for the whole study
                 is reported next to it.

Per shape and route the median of --reps rounds with its range, the speed-up of the medians, the worst pairing
(fastest other route over slowest new call) and the largest relative difference of the results.  Writes one JSON
object to --out (default profiles/sequence_infidelities_time.json) and prints it.

    python tools/time_sequence_infidelities.py [--reps 5] [--stride 10] [--out FILE]
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

T = wl.CONFIG3['T']


def study_draws(cliffords, draws=50):
    """The study's index arrays: 21 lengths, *draws* each, the inverting Clifford appended."""
    lengths = np.linspace(1, 151, 21).astype(int)
    out = []
    for k, m in enumerate(np.repeat(lengths, draws)):
        draw = np.random.default_rng(100 + k).integers(0, 24, m)
        U = ff.concatenate_without_filter_function(cliffords[draw]).total_propagator
        inverse = int(np.argmax([abs(np.trace(g.total_propagator @ U)) for g in cliffords]))
        out.append(np.append(draw, inverse))
    return out


def two_qubit_gate_set(omega):
    """X/2 and Y/2 on either qubit and a ZZ-coupled entangler, every one with noise on XI and IX, control matrices
    cached at omega, and the 20 ordered products of two different ones by `@`."""
    P = dict(zip('IXYZ', ff.util.paulis))
    op = lambda name: np.kron(P[name[0]], P[name[1]])/2       # noqa: E731
    basis = ff.Basis.pauli(2)
    noise = lambda: [[op('IX'), [1.0], 'IX'], [op('XI'), [1.0], 'XI']]      # noqa: E731
    atoms = [ff.PulseSequence([[op(c), [np.pi/2/T], c]], noise(), [T], basis=basis) for c in ('XI', 'YI', 'IX', 'IY')]
    atoms.append(ff.PulseSequence([[op('ZZ'), [np.pi/T], 'ZZ']], noise(), [T], basis=basis))
    for atom in atoms:
        atom.cache_control_matrix(omega)
    return atoms + [a @ b for a in atoms for b in atoms if a is not b]


def spread(times):
    t = np.asarray(times)
    return {'median': round(float(np.median(t)), 5), 'min': round(float(t.min()), 5), 'max': round(float(t.max()), 5)}


def loop(gates, seqs, spectra, omega):
    out = []
    for s in seqs:
        pulse = ff.concatenate(gates[s], omega=omega)
        out.append([ff.infidelity(pulse, S, omega) for S in spectra])
    return np.array(out).swapaxes(0, 1)


def batched(gates, seqs, spectra, omega):
    pulses = ff.concatenate_sequences([gates[s] for s in seqs])
    return np.array([ff.infidelities(pulses, S, omega) for S in spectra])


def new(gates, seqs, spectra, omega):
    return np.array([ff.sequence_infidelities(gates, seqs, S, omega) for S in spectra])


def alternate(routes, reps):
    """Every route once per round, the first round the warm-up: ({name: seconds per round}, {name: last result})."""
    times, results = {name: [] for name in routes}, {}
    for r in range(reps + 1):
        for name, run in routes.items():
            t0 = time.perf_counter()
            results[name] = run()
            if r:
                times[name].append(time.perf_counter() - t0)
    return times, results


def report(times, results, n):
    others = [name for name in times if name != 'new']
    fastest = min(others, key=lambda name: np.median(times[name]))
    out = {'sequences': n, 'seconds': {name: spread(t) for name, t in times.items()}, 'fastest_other_route': fastest,
           'speedup': round(float(np.median(times[fastest])/np.median(times['new'])), 2),
           'speedup_worst_pairing': round(float(min(min(times[name]) for name in others)/max(times['new'])), 2),
           'max_rel_difference': {name: float(np.abs(results['new'] - results[name]).max()/np.abs(results[name]).max())
                                  for name in others}}
    return out


def measure(reps, stride):
    omega = wl.rb_omega(301, T)
    spectra = [wl.rb_spectrum(omega, 0.0), wl.rb_spectrum(omega, 0.7)]
    cliffords = np.array(wl.rb_cliffords(ff, omega, T)[1], dtype=object)
    seqs = study_draws(cliffords)
    out = {'n_omega': len(omega), 'repetitions': reps, 'spectra': len(spectra),
           'positions': int(sum(len(s) for s in seqs))}
    times, results = alternate({'loop': lambda: loop(cliffords, seqs, spectra, omega),
                                'concatenate_sequences': lambda: batched(cliffords, seqs, spectra, omega),
                                'new': lambda: new(cliffords, seqs, spectra, omega)}, reps)
    out['single_qubit'] = report(times, results, len(seqs))
    gates = two_qubit_gate_set(omega)
    table = np.array(gates, dtype=object)
    some = seqs[::stride]
    times, results = alternate({'loop': lambda: loop(table, some, spectra, omega),
                                'new': lambda: new(gates, some, spectra, omega)}, reps)
    out['two_qubit'] = dict(report(times, results, len(some)), gates=len(gates), stride=stride)
    whole, _ = alternate({'new': lambda: new(gates, seqs, spectra, omega)}, reps)
    out['two_qubit']['whole_study'] = {'sequences': len(seqs), 'seconds': spread(whole['new'])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--stride', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sequence_infidelities_time.json'))
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

"""Time of ff.sequence_infidelity_derivatives and ff.gate_infidelity_derivatives against the routes they replace.
Host clocks around synchronous calls, one process, the routes alternating, warm-up round first.

  loop      [gradient.infidelity_derivative(ff.concatenate(gates[s]), S, omega) for s in sequences]
  batched   sequences of equal length only: ff.infidelity_derivatives([ff.concatenate(gates[s]) for s in sequences],
            S, omega), the only other batched route (the concatenation is part of it)
  new       ff.sequence_infidelity_derivatives(gates, sequences, S, omega)
  new_gate  ff.gate_infidelity_derivatives(gates, sequences, S, omega): the per-gate sums, nothing per position copied

  single_qubit  the 24 Cliffords of the randomized-benchmarking study (workloads.CLIFFORD_WORDS, 1 to 7 segments each)
                at 301 frequencies, every gate carrying the X and the Y control so that the set shares one operator
                table; every --stride-th sequence of the study's 1050 (2 to 152 positions)
  two_qubit     5 two-qubit gates (X/2, Y/2 on either qubit, a ZZ entangler) over one table of five control and two
                noise operators: three sequences each of 16 and of 152 positions, each group a call of its own

Before anything is timed the routes' results are compared and asserted to agree within 1e-10, the bar of the tests.
Per shape: medians of --reps rounds with their ranges, the ratio of the fastest other route to new, the worst pairing
(fastest round of the other route over slowest round of new) and the device bytes of the pass.  Writes one JSON object
to --out (default profiles/sequence_gradients_time.json) and prints it.

    python tools/time_sequence_gradients.py [--reps 5] [--stride 10] [--out FILE]
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
from filter_functions_amd import _lib, gradient, sequence_gradient  # noqa: E402
from time_sequence_infidelities import T, alternate, spread, study_draws  # noqa: E402

AGREE = 1e-10


def cliffords_over_one_table():
    """The study's 24 Cliffords from X/2 and Y/2 atoms that both carry the X and the Y control (noise on X)."""
    X, Y = ff.util.paulis[1], ff.util.paulis[2]
    atoms = {'x': ff.PulseSequence([[X/2, [np.pi/2/T], 'X'], [Y/2, [0.0], 'Y']], [[X/2, [1], 'X']], [T]),
             'y': ff.PulseSequence([[X/2, [0.0], 'X'], [Y/2, [np.pi/2/T], 'Y']], [[X/2, [1], 'X']], [T])}
    gates = []
    for word in wl.CLIFFORD_WORDS:
        gate = atoms[word[0]]
        for letter in word[1:]:
            gate = gate @ atoms[letter]
        gates.append(gate)
    for gate in gates:
        gate.diagonalize()
    return gates


def two_qubit_gates():
    P = dict(zip('IXYZ', ff.util.paulis))
    op = lambda name: np.kron(P[name[0]], P[name[1]])/2       # noqa: E731
    controls = ('XI', 'YI', 'IX', 'IY', 'ZZ')
    angle = dict(XI=np.pi/2, YI=np.pi/2, IX=np.pi/2, IY=np.pi/2, ZZ=np.pi)
    gates = [ff.PulseSequence([[op(c), [angle[c]/T if c == on else 0.0], c] for c in controls],
                              [[op('IX'), [1.0], 'IX'], [op('XI'), [1.0], 'XI']], [T], basis=ff.Basis.pauli(2))
             for on in controls]
    for gate in gates:
        gate.diagonalize()
    return gates


def loop(table, seqs, S, omega):
    return [gradient.infidelity_derivative(ff.concatenate(table[s]), S, omega) for s in seqs]


def batched(table, seqs, S, omega):
    return list(ff.infidelity_derivatives([ff.concatenate(table[s]) for s in seqs], S, omega))


def workspace(gates, seqs, W, A, H, d):
    segments = np.array([len(g.dt) for g in gates])
    n_segments = int(sum(segments[s].sum() for s in seqs))
    return {'walked_segments': n_segments,
            'pass_bytes': int(_lib.load().ffk_sequence_infidelity_derivatives_workspace_bytes(
                len(gates), int(segments.max()), len(seqs), int(sum(len(s) for s in seqs)), n_segments, W, A, H, d, 0))}


def report(times, results, n):
    others = [name for name in times if not name.startswith('new')]
    fastest = min(others, key=lambda name: np.median(times[name]))
    agreement = {}
    for name in others:
        agreement[name] = float(max(np.abs(a - b).max()/np.abs(b).max() for a, b in zip(results['new'], results[name])))
    assert max(agreement.values()) < AGREE, agreement
    return {'sequences': n, 'seconds': {name: spread(t) for name, t in times.items()}, 'fastest_other_route': fastest,
            'speedup': round(float(np.median(times[fastest])/np.median(times['new'])), 2),
            'speedup_worst_pairing': round(float(min(min(times[name]) for name in others)/max(times['new'])), 2),
            'per_gate_sums_over_new': round(float(np.median(times['new_gate'])/np.median(times['new'])), 2),
            'max_rel_difference': agreement}


def shape(gates, seqs, S, omega, reps, with_batched):
    table = np.array(gates, dtype=object)
    assert sequence_gradient.eligibility(gates) is not None
    routes = {'loop': lambda: loop(table, seqs, S, omega)}
    if with_batched:
        routes['batched'] = lambda: batched(table, seqs, S, omega)
    routes['new'] = lambda: ff.sequence_infidelity_derivatives(gates, seqs, S, omega)
    routes['new_gate'] = lambda: ff.gate_infidelity_derivatives(gates, seqs, S, omega)
    times, results = alternate(routes, reps)
    d, A, H = gates[0].d, len(gates[0].n_opers), len(gates[0].c_opers)
    return dict(report(times, results, len(seqs)), gates=len(gates), d=d,
                positions=[min(len(s) for s in seqs), max(len(s) for s in seqs)],
                **workspace(gates, seqs, len(omega), A, H, d))


def measure(reps, stride):
    omega = wl.rb_omega(301, T)
    S = wl.rb_spectrum(omega, 0.7)
    out = {'n_omega': len(omega), 'repetitions': reps, 'agreement_bar': AGREE,
           'clock': 'host, time.perf_counter around synchronous calls'}
    cliffords = cliffords_over_one_table()
    seqs = study_draws(np.array(cliffords, dtype=object))[::stride]
    out['single_qubit'] = dict(shape(cliffords, seqs, S, omega, reps, False), stride=stride)
    gates = two_qubit_gates()
    rng = np.random.default_rng(5)
    for n in (16, 152):
        seqs = [rng.integers(0, len(gates), n) for _ in range(3)]
        out[f'two_qubit_{n}_positions'] = shape(gates, seqs, S, omega, reps, True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--stride', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sequence_gradients_time.json'))
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

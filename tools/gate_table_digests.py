"""Digests and times of every public function that evaluates many gate sequences from one gate table, for comparing
two trees of this project bit by bit: the file uses the public API only, so the same file runs on either tree
(``--tree``), and two runs on one device must print equal digests unless something that computes has changed.

Digests (sha256 of the returned bytes) on seeded inputs, d = 2 and d = 4, A in {1, 4} noise operators, W in {7, 65}
frequencies, sequences of 1, 2, 5 and 64 gates, and two gate sets of equal control matrices: ``host`` (every gate's
control matrix uploaded from the host) and ``mixed`` (every other gate a resident member of one
``ff.get_filter_functions`` call):

  concatenate_sequences + infidelities, correlation_infidelities             (d = 2)
  sequence_infidelities with propagators and filter functions
  sequence_correlation_infidelities
  sequence_decay_amplitudes, sequence_cumulant_functions, sequence_error_transfer_matrices   (stacked, K = 2)
  sequence_frequency_shifts                                                                 (stacked, K = 2)

(the two correlation calls without the sequence of one gate, for which the loop they stand for raises)

``--time`` additionally times those calls (not the loops they replace) on the randomized-benchmarking study's shape --
``study_draws`` of tools/time_sequence_infidelities.py: 1050 sequences of 2 to 152 gates, 301 frequencies -- over the
24 Cliffords (d = 2) and the 25 two-qubit gates of that tool (d = 4), for both gate sets: host clock around the
synchronous call, one warm-up round, then ``--rounds`` rounds.  Writes one JSON object to ``--out`` and prints it.

    python tools/gate_table_digests.py [--tree DIR] [--time] [--rounds 7] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help='root of the tree whose package is imported (default: the tree this file lies in)')
ap.add_argument('--time', action='store_true')
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--out', default=None)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))

import filter_functions_amd as ff  # noqa: E402
import workloads as wl  # noqa: E402

LENGTHS = (1, 2, 5, 64)


def digest(result):
    """sha256 over the arrays of a result (an array, or a tuple or list of them), shapes and types included."""
    h = hashlib.sha256()
    for a in (result if isinstance(result, (tuple, list)) else [result]):
        a = np.ascontiguousarray(a)
        h.update(f'{a.dtype}{a.shape}'.encode())
        h.update(a.tobytes())
    return h.hexdigest()


def pauli_string(name):
    """The Pauli string *name*; 'H' is (X + Z)/sqrt(2)."""
    P = dict(zip('IXYZ', ff.util.paulis))
    P['H'] = (P['X'] + P['Z'])/np.sqrt(2)
    out = np.ones((1, 1))
    for c in name:
        out = np.kron(out, P[c])
    return out


def seeded_gates(d, A, T, seed):
    """T two-segment gates with nothing cached, the same A noise operators on every one."""
    rng = np.random.default_rng(seed)
    controls, noise = (('X', 'Y'), ('X', 'Y', 'Z', 'H')) if d == 2 else (('XI', 'IX', 'ZZ'), ('IX', 'IZ', 'XI', 'ZI'))
    basis = ff.Basis.pauli(1 if d == 2 else 2)
    return [ff.PulseSequence([[pauli_string(c)/2, rng.normal(size=2), c] for c in controls],
                             [[pauli_string(n)/2, 0.5 + rng.random(2), f'n{k}'] for k, n in enumerate(noise[:A])],
                             1.0 + rng.random(2), basis=basis) for _ in range(T)]


def fresh(gate):
    """A new pulse with *gate*'s Hamiltonians and basis and nothing cached."""
    return ff.PulseSequence(list(zip(gate.c_opers, gate.c_coeffs, gate.c_oper_identifiers)),
                            list(zip(gate.n_opers, gate.n_coeffs, gate.n_oper_identifiers)), gate.dt, basis=gate.basis)


def gate_sets(source, omega):
    """{'host', 'mixed'}: copies of *source* with equal control matrices -- computed by one ff.get_filter_functions
    call, whose members keep them in HBM; the host copies carry them as arrays."""
    members = [fresh(g) for g in source]
    ff.get_filter_functions(members, omega)
    host = [fresh(g) for g in source]
    for h, m in zip(host, members):
        h.cache_control_matrix(omega, np.array(m.get_control_matrix(omega)))
        h.total_propagator = np.array(m.total_propagator)
    return {'host': host, 'mixed': [m if k % 2 == 0 else h for k, (m, h) in enumerate(zip(members, host))]}


def calls(gates, seqs, S, stack, omega):
    """{name: thunk} of the calls on one gate set, in the order in which they run."""
    table = np.array(gates, dtype=object)
    pairs = [s for s in seqs if len(s) > 1]           # (a single gate has no pulse correlations: the loop raises)
    out = {}
    if gates[0].d == 2:
        out['concatenate_sequences+infidelities'] = lambda: ff.infidelities(
            ff.concatenate_sequences([table[s] for s in seqs], omega=omega), S, omega)
        out['correlation_infidelities'] = lambda: ff.correlation_infidelities([table[s] for s in pairs], S, omega)
    out['sequence_infidelities'] = lambda: ff.sequence_infidelities(
        gates, seqs, S, omega, return_propagators=True, return_filter_functions=True)
    out['sequence_correlation_infidelities'] = lambda: ff.sequence_correlation_infidelities(gates, pairs, S, omega)
    for name in ('sequence_decay_amplitudes', 'sequence_cumulant_functions', 'sequence_error_transfer_matrices',
                 'sequence_frequency_shifts'):
        out[name] = lambda f=getattr(ff, name): f(gates, seqs, stack, omega, stacked=True)
    return out


def digests():
    out = {}
    for d in (2, 4):
        for A in (1, 4):
            for W in (7, 65):
                omega = np.geomspace(1e-2, 1e2, W)
                S = 1/omega**0.7
                stack = np.stack([S, 0.3 + 1/omega**0.2])
                rng = np.random.default_rng(1000*d + 10*A + W)
                seqs = [rng.integers(0, 5, m) for m in LENGTHS]
                for kind, gates in gate_sets(seeded_gates(d, A, 5, 7*d + A), omega).items():
                    for name, run in calls(gates, seqs, S, stack, omega).items():
                        out[f'd={d} A={A} W={W} {kind} {name}'] = digest(run())
    return out


def times(rounds):
    sys.path.insert(0, os.path.join(os.path.abspath(ARGS.tree), 'tools'))
    from time_sequence_infidelities import study_draws, two_qubit_gate_set
    T = wl.CONFIG3['T']
    omega = wl.rb_omega(301, T)
    S = wl.rb_spectrum(omega, 0.7)
    stack = np.stack([wl.rb_spectrum(omega, 0.0), S])
    cliffords = np.array(wl.rb_cliffords(ff, omega, T)[1], dtype=object)
    seqs = study_draws(cliffords)
    out = {}
    for d, source in ((2, list(cliffords)), (4, two_qubit_gate_set(omega))):
        for kind, gates in gate_sets(source, omega).items():
            runs = calls(gates, seqs, S, stack, omega)
            seconds = {name: [] for name in runs}
            for r in range(rounds + 1):
                for name, run in runs.items():
                    t0 = time.perf_counter()
                    run()
                    if r:
                        seconds[name].append(time.perf_counter() - t0)
            for name, t in seconds.items():
                out[f'd={d} {kind} {name}'] = {'median': float(np.median(t)), 'min': min(t), 'max': max(t),
                                               'rounds': [round(x, 6) for x in t]}
    return out


def main():
    from filter_functions_amd import _lib
    out = {'device': _lib.device_info()[0], 'digests': digests()}
    if ARGS.time:
        out['times'] = times(ARGS.rounds)
    text = json.dumps(out, indent=1)
    if ARGS.out:
        with open(ARGS.out, 'w') as fh:
            fh.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()

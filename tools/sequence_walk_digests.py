"""Digests of every public function behind the forward sequence walk (csrc/sequence_walk.h), for comparing two trees of
this project bit by bit: the file uses the public API only, so the same file runs on either tree (``--tree``), and two
runs on one device must print equal digests unless an operation order has changed.

Digests (sha256 of the returned bytes) of

  sequence_frequency_shifts
  sequence_prefix_infidelities, sequence_prefix_decay_amplitudes (full and diagonal=True),
  sequence_prefix_frequency_shifts                                             (each without and with closing gates)

on seeded inputs, the smallest that reach every branch of the shared code: d = 2 and d = 4; A = 1..4 noise operators
(tiles per block change at A = 3, spectra per walk at A = 4, and at A = 3 with closing gates at d = 4); W = 7 and 65
frequencies (one ragged block; two or three blocks with a ragged last one); sequences of 1, 2, 64, 65 and 130 gates
(the index chunk is 64 positions); a table of 3 gates, which is staged in LDS at every A, under one spectrum (W,), a
stack of 3 spectra (stacked=True: two walks in grid z, the second partly filled), a spectrum per operator (n_idx, W),
and with the operators a proper subset in non-ascending order; and a table of 40 gates, read from L2 at every A, with
sequences that use all of them.

    python tools/sequence_walk_digests.py [--tree DIR] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help='root of the tree whose package is imported (default: the tree this file lies in)')
ap.add_argument('--out', default=None)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))

import filter_functions_amd as ff  # noqa: E402

LENGTHS = (1, 2, 64, 65, 130)


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
    """T two-segment gates, the same A noise operators 'n0', 'n1', ... on every one."""
    rng = np.random.default_rng(seed)
    controls, noise = (('X', 'Y'), ('X', 'Y', 'Z', 'H')) if d == 2 else (('XI', 'IX', 'ZZ'), ('IX', 'IZ', 'XI', 'ZI'))
    basis = ff.Basis.pauli(1 if d == 2 else 2)
    return [ff.PulseSequence([[pauli_string(c)/2, rng.normal(size=2), c] for c in controls],
                             [[pauli_string(n)/2, 0.5 + rng.random(2), f'n{k}'] for k, n in enumerate(noise[:A])],
                             1.0 + rng.random(2), basis=basis) for _ in range(T)]


def seeded_sequences(T, rng):
    """Sequences of LENGTHS gates and closing gates as long; the ones of at least T gates use every gate."""
    seqs = []
    for m in LENGTHS:
        s = rng.integers(0, T, m)
        if m >= T:
            s[:T] = rng.permutation(T)
        seqs.append(s)
    return seqs, [rng.integers(0, T, m) for m in LENGTHS]


def calls(gates, seqs, closing, spectrum, omega, identifiers, stacked):
    """{name: thunk} of the calls under one spectrum, in the order in which they run."""
    kw = dict(n_oper_identifiers=identifiers, stacked=stacked)
    out = {'sequence_frequency_shifts': lambda: ff.sequence_frequency_shifts(gates, seqs, spectrum, omega, **kw)}
    for tag, close in (('', None), (' closing', closing)):
        out['sequence_prefix_infidelities' + tag] = lambda c=close: ff.sequence_prefix_infidelities(
            gates, seqs, spectrum, omega, closing=c, **kw)
        out['sequence_prefix_decay_amplitudes' + tag] = lambda c=close: ff.sequence_prefix_decay_amplitudes(
            gates, seqs, spectrum, omega, closing=c, **kw)
        out['sequence_prefix_decay_amplitudes diagonal' + tag] = lambda c=close: ff.sequence_prefix_decay_amplitudes(
            gates, seqs, spectrum, omega, closing=c, diagonal=True, **kw)
        out['sequence_prefix_frequency_shifts' + tag] = lambda c=close: ff.sequence_prefix_frequency_shifts(
            gates, seqs, spectrum, omega, closing=c, **kw)
    return out


def digests():
    out = {}
    for d in (2, 4):
        for A in (1, 2, 3, 4):
            for W in (7, 65):
                omega = np.geomspace(1e-2, 1e2, W)
                S = 1/omega**0.7
                stack = np.stack([S, 0.3 + 1/omega**0.2, 1/(1 + omega**2)])
                per_operator = np.stack([(a + 1.0)/omega**(0.3*a) for a in range(A)])
                subset = [f'n{a}' for a in range(A - 1, -1, -1) if a != A - 2][:A - 1] if A > 1 else None
                for T in (3, 40):
                    rng = np.random.default_rng(1000*d + 100*A + W + T)
                    gates = seeded_gates(d, A, T, 7*d + A + T)
                    seqs, closing = seeded_sequences(T, rng)
                    spectra = {'single': (S, None, False)}
                    if T == 3:
                        spectra['stacked'] = (stack, None, True)
                        spectra['per operator'] = (per_operator, None, False)
                        if subset:
                            spectra['subset ' + ','.join(subset)] = (stack, subset, True)
                    for kind, (spectrum, identifiers, stacked) in spectra.items():
                        for name, run in calls(gates, seqs, closing, spectrum, omega, identifiers, stacked).items():
                            out[f'd={d} A={A} W={W} T={T} {kind} {name}'] = digest(run())
    return out


def main():
    from filter_functions_amd import _lib
    out = {'device': _lib.device_info()[0], 'digests': digests()}
    text = json.dumps(out, indent=1)
    if ARGS.out:
        with open(ARGS.out, 'w') as fh:
            fh.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()

"""Time of a periodic-driving sweep through ff.periodic_infidelities / ff.periodic_decay_amplitudes against the double
loop over ff.concatenate_periodic; host clocks around synchronous calls, one process, warm-up first, loop and batched
call alternating in the same job:
  (a) [[ff.infidelity(ff.concatenate_periodic(p, n), S, omega) for n in repeats] for p in pulses]
      (and the same with numeric.calculate_decay_amplitudes)
  (b) ff.periodic_infidelities(pulses, repeats, S, omega)   /   ff.periodic_decay_amplitudes(...)
Every repetition of either side gets fresh pulses whose control matrices one ff.get_filter_functions call OUTSIDE the
timed region left resident in HBM.  Shapes:
  qubit      64 single-qubit pulses (a drive of 20 segments, the amplitude swept), 500 frequencies
  two_qubit  16 two-qubit pulses (20 segments, Pauli basis, three noise operators), 500 frequencies
each at 25 logarithmically spaced repeat counts from 1 to 10^6.  Writes one JSON object (medians and ranges of
--reps repetitions, the worst pairing of a loop and a batched time) to --out (default profiles/periodic_time.json) and
prints it.  The loop tiles the segment tables of 10^6 periods on the host for every pulse: --loop-reps (default: --reps)
bounds how often it is repeated, --loop-pulses how many of the pulses it runs over (its time is then scaled to the
whole list and marked as such).

    python tools/time_periodic.py [--reps 5] [--loop-reps N] [--loop-pulses N] [--only qubit|two_qubit] [--out FILE]
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import filter_functions_amd as ff  # noqa: E402
from filter_functions_amd import _lib, numeric  # noqa: E402

REPEATS = np.unique(np.round(np.geomspace(1, 1e6, 25)).astype(int))
PAULI = np.array([[[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]], dtype=complex)


def qubit(P=64, G=20, W=500):
    """A drive about x with a slow envelope, its amplitude swept over the pulses; dephasing and amplitude noise."""
    dt = np.full(G, 0.05)
    envelope = 1.0 + 0.2*np.cos(2*np.pi*np.arange(G)/G)
    amplitudes = np.linspace(0.5, 8.0, P)
    basis = ff.Basis.pauli(1)
    omega = np.geomspace(1e-3, 1e2, W)

    def make():
        pulses = [ff.PulseSequence([[PAULI[0]/2, a*envelope], [PAULI[2]/2, np.full(G, 0.3)]],
                                   [[PAULI[2]/2, np.ones(G)]], dt, basis) for a in amplitudes]
        ff.get_filter_functions(pulses, omega)
        return pulses
    return make, omega, 1e-3/np.maximum(omega, 1e-3)


def two_qubit(P=16, G=20, W=500):
    rng = np.random.default_rng(5)
    dt = np.full(G, 0.05)
    basis = ff.Basis.pauli(2)
    omega = np.geomspace(1e-3, 1e2, W)
    kron = lambda a, b: np.kron(a, b)      # noqa: E731
    eye = np.eye(2)
    c_opers = [kron(PAULI[0], eye)/2, kron(eye, PAULI[0])/2, kron(PAULI[2], PAULI[2])/2]
    n_opers = [kron(PAULI[2], eye)/2, kron(eye, PAULI[2])/2, kron(PAULI[2], PAULI[2])/2]
    coeffs = rng.normal(size=(P, 3, G))

    def make():
        pulses = [ff.PulseSequence([[o, c] for o, c in zip(c_opers, coeffs[p])], [[o, np.ones(G)] for o in n_opers],
                                   dt, basis) for p in range(P)]
        ff.get_filter_functions(pulses, omega)
        return pulses
    return make, omega, 1e-3/np.maximum(omega, 1e-3)


def timed(f):
    gc.collect()
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def spread(seconds):
    s = np.asarray(seconds)
    return dict(median_s=float(np.median(s)), min_s=float(s.min()), max_s=float(s.max()), n=len(s))


def measure(make, omega, S, reps, loop_reps, loop_pulses):
    single = {'infidelity': lambda p, n: ff.infidelity(ff.concatenate_periodic(p, n), S, omega),
              'decay_amplitudes': lambda p, n: numeric.calculate_decay_amplitudes(ff.concatenate_periodic(p, n), S,
                                                                                  omega)}
    many = {'infidelity': ff.periodic_infidelities, 'decay_amplitudes': ff.periodic_decay_amplitudes}
    result = {}
    for name in single:
        many[name](make(), REPEATS, S, omega)                                   # warm-up
        [single[name](p, int(n)) for p in make()[:2] for n in REPEATS[:3]]
        loop_t, batch_t, worst = [], [], 0.0
        for r in range(reps):
            pulses = make()
            P = len(pulses)
            t_batch, got = timed(lambda: many[name](pulses, REPEATS, S, omega))
            batch_t.append(t_batch)
            if r < loop_reps:
                pulses = make()[:loop_pulses or None]
                t_loop, ref = timed(lambda: np.stack([np.stack([single[name](p, int(n)) for n in REPEATS])
                                                      for p in pulses]))
                loop_t.append(t_loop*P/len(pulses))
                worst = max(worst, float(np.abs(got[:len(pulses)] - ref).max()/np.abs(ref).max()))
        result[name] = dict(loop=spread(loop_t), batched=spread(batch_t),
                            ratio_of_medians=float(np.median(loop_t)/np.median(batch_t)),
                            worst_pairing=float(min(loop_t)/max(batch_t)), loop_pulses=loop_pulses or P,
                            max_difference=worst)
    return result


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--reps', type=int, default=5)
    parser.add_argument('--loop-reps', type=int, default=None)
    parser.add_argument('--loop-pulses', type=int, default=0)
    parser.add_argument('--only', choices=['qubit', 'two_qubit'])
    parser.add_argument('--out', default=os.path.join('profiles', 'periodic_time.json'))
    args = parser.parse_args()
    loop_reps = args.reps if args.loop_reps is None else args.loop_reps
    out = dict(repeats=[int(n) for n in REPEATS], device=str(_lib.device_name()) if hasattr(_lib, 'device_name') else '')
    for name, shape in (('qubit', qubit), ('two_qubit', two_qubit)):
        if args.only in (None, name):
            make, omega, S = shape()
            out[name] = measure(make, omega, S, args.reps, loop_reps, args.loop_pulses)
    text = json.dumps(out, indent=1)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()

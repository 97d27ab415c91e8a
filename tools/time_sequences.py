"""The randomized-benchmarking study of the reference's example (examples/randomized_benchmarking.py:70-90) with
the loop of ff.concatenate + ff.infidelity against ff.concatenate_sequences + ff.infidelities, host clocks around
synchronous calls, one process, warm-up first:
  study   21 lengths (1 to 151 Cliffords) x N_G sequences, the inverting Clifford appended, 301 frequencies, two
          spectra; naive and optimised gate sets
  cfg3    64 draws of 1000 Cliffords at 8192 frequencies (config 3 x 64), naive gates
Per batched pass the handle's host clocks (staging, enqueue, wait) are recorded.  Device times per kernel: run the
tool under ``rocprofv3 --kernel-trace --stats``.  Writes one JSON line (and --out FILE).

    python tools/time_sequences.py [--n-g 50] [--reps 3] [--out profiles/sequences_time.json]
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
from filter_functions_amd import sequences  # noqa: E402

PASSES = []
_evaluate = sequences.SequencePass.evaluate


def _timed_evaluate(self, *args, **kwargs):
    out = _evaluate(self, *args, **kwargs)
    clocks = np.zeros(3)
    sequences._lib.check(self._lib.ffk_resident_timing(self._handle, clocks.ctypes.data))
    PASSES.append(dict(sequences=int(self.shape[0]), stage_s=clocks[0], enqueue_s=clocks[1], wait_s=clocks[2]))
    return out


sequences.SequencePass.evaluate = _timed_evaluate


def inverse_of(U, gates):
    return gates[int(np.argmax([abs(np.trace(g.total_propagator @ U)) for g in gates]))]


def study_sequences(cliffords, n_g, seed=0):
    rng = np.random.default_rng(seed)
    seqs = []
    for m in np.linspace(1, 151, 21).astype(int):
        for _ in range(n_g):
            draw = cliffords[rng.integers(0, len(cliffords), m)]
            U = ff.concatenate_without_filter_function(draw).total_propagator
            seqs.append(list(draw) + [inverse_of(U, cliffords)])
    return seqs


def best(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return min(times), times


def study(cliffords, omega, n_g, reps):
    seqs = study_sequences(cliffords, n_g)
    spectra = [wl.rb_spectrum(omega, 0.0), wl.rb_spectrum(omega, 0.7)]

    def looped():
        for s in seqs:
            pulse = ff.concatenate(s)
            for S in spectra:
                ff.infidelity(pulse, S, omega)

    def batched():
        pulses = ff.concatenate_sequences(seqs)
        for S in spectra:
            ff.infidelities(pulses, S, omega)

    looped()
    batched()
    t_loop, all_loop = best(looped, reps)
    del PASSES[:]
    t_batch, all_batch = best(batched, reps)
    passes = PASSES[-1:]          # the last repetition's pass(es)
    device_wait = sum(p['wait_s'] for p in passes)
    P = len(seqs)
    return dict(sequences=P, loop_s=t_loop, batched_s=t_batch, speedup=t_loop/t_batch,
                loop_ms_per_sequence=1e3*t_loop/P, batched_ms_per_sequence=1e3*t_batch/P,
                host_ms_per_sequence=1e3*(t_batch - device_wait)/P, passes=passes, loop_all_s=all_loop,
                batched_all_s=all_batch)


def config3(reps):
    omega = wl.rb_omega(wl.CONFIG3['W'], wl.CONFIG3['T'])
    _, cliffords = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])
    cliffords = np.array(cliffords, dtype=object)
    seqs = [cliffords[wl.rb_draw(1000, s)] for s in range(64)]

    def looped():
        for s in seqs:
            ff.concatenate(s)

    def batched():
        ff.concatenate_sequences(seqs)
    looped()
    batched()
    t_loop, _ = best(looped, reps)
    del PASSES[:]
    t_batch, _ = best(batched, reps)
    return dict(sequences=64, loop_ms_per_sequence=1e3*t_loop/64, batched_ms_per_sequence=1e3*t_batch/64,
                passes=PASSES[-1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-g', type=int, default=50)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    omega = wl.rb_omega(301, wl.CONFIG3['T'])
    _, naive = wl.rb_cliffords(ff, omega, wl.CONFIG3['T'])
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'rb_optimized_gates.npz'))
    gates = {name: (g[f'{name}_eps'], g[f'{name}_t'], g[f'{name}_B']) for name in ('X2', 'Y2')}
    _, optimized = wl.rb_cliffords_optimized(ff, omega, gates)
    result = dict(study_naive=study(np.array(naive, dtype=object), omega, args.n_g, args.reps),
                  study_optimized=study(np.array(optimized, dtype=object), omega, args.n_g, args.reps),
                  config3_x64=config3(args.reps))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()

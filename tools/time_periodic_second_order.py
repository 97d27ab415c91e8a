"""Time of the frequency shifts of a periodic-driving sweep through ff.periodic_frequency_shifts against the two other
routes; host clocks around synchronous calls, one process, warm-up first, the routes alternating in the same job,
results compared before anything is timed:
  (a) ff.periodic_frequency_shifts(pulses, repeats, S, omega)                      -- period doubling, O(log n)
  (b) ff.sequence_prefix_frequency_shifts(pulses, [[p]*n_max for p], S, omega)     -- the forward walk, O(n_max)
      positions per pulse, the only other batched route; timed at --walk-periods (default 1000) and compared with
      (a) at the counts up to there.  Its time at the sweep's 10^6 periods is an EXTRAPOLATION (x 10^6 / n_max, the
      walk is linear in the positions) and is marked as such.
  (c) the loop numeric.calculate_frequency_shifts(ff.concatenate([p]*n, calc_second_order_FF=True, omega=omega), S,
      omega) at the counts <= 16 of the sweep, against (a) on the same counts.
Every repetition of every route gets fresh pulses whose control matrices one ff.get_filter_functions call OUTSIDE the
timed region left resident in HBM; the pulses' own frequency shifts (ff.frequency_shifts) are inside the timed region
of (a) and (b), which both need them.  Shapes: those of tools/time_periodic.py (64 single-qubit pulses, 16 two-qubit
pulses, 20 segments, 500 frequencies, 25 logarithmically spaced repeat counts from 1 to 10^6).  No kernel trace is
taken.  Writes one JSON object (medians and ranges of --reps repetitions) to --out and prints it.

    python tools/time_periodic_second_order.py [--reps 5] [--loop-reps N] [--walk-periods 1000]
                                               [--only qubit|two_qubit] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import filter_functions_amd as ff  # noqa: E402
from filter_functions_amd import numeric  # noqa: E402
from time_periodic import REPEATS, qubit, spread, timed, two_qubit  # noqa: E402


def difference(got, ref):
    return float(np.abs(got - ref).max()/np.abs(ref).max())


def measure(make, omega, S, reps, loop_reps, walk_periods):
    few = REPEATS[REPEATS <= 16]
    within = REPEATS[REPEATS <= walk_periods]

    def doubling(pulses, repeats=REPEATS):
        return ff.periodic_frequency_shifts(pulses, repeats, S, omega)

    def walk(pulses):
        curves = ff.sequence_prefix_frequency_shifts(pulses, [np.full(walk_periods, p) for p in range(len(pulses))],
                                                     S, omega)
        return np.stack([curve[within - 1] for curve in curves])

    def loop(pulses):
        return np.stack([np.stack([numeric.calculate_frequency_shifts(
            ff.concatenate([p]*int(n), calc_second_order_FF=True, omega=omega), S, omega) for n in few])
            for p in pulses])
    # results first (this is the warm-up as well)
    whole = doubling(make())
    differences = dict(walk=difference(whole[:, :len(within)], walk(make())),
                       loop=difference(whole[:, :len(few)], loop(make())))
    assert np.isfinite(whole).all() and max(differences.values()) < 1e-8, differences
    t_doubling, t_walk, t_few, t_loop = [], [], [], []
    for r in range(reps):
        t_doubling.append(timed(lambda pulses=make(): doubling(pulses))[0])
        t_walk.append(timed(lambda pulses=make(): walk(pulses))[0])
        if r < loop_reps:
            t_few.append(timed(lambda pulses=make(): doubling(pulses, few))[0])
            t_loop.append(timed(lambda pulses=make(): loop(pulses))[0])
    scale = float(REPEATS.max())/walk_periods
    return dict(
        doubling=spread(t_doubling), walk=spread(t_walk), walk_periods=walk_periods,
        walk_extrapolated_to_largest_count_s=float(np.median(t_walk)*scale),
        extrapolated_walk_over_doubling=float(np.median(t_walk)*scale/np.median(t_doubling)),
        walk_over_doubling_as_timed=float(np.median(t_walk)/np.median(t_doubling)),
        counts_of_the_loop=[int(n) for n in few], doubling_at_those_counts=spread(t_few), loop=spread(t_loop),
        loop_over_doubling=float(np.median(t_loop)/np.median(t_few)),
        loop_over_doubling_worst_pairing=float(min(t_loop)/max(t_few)), max_difference=differences)


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--reps', type=int, default=5)
    parser.add_argument('--loop-reps', type=int, default=None)
    parser.add_argument('--walk-periods', type=int, default=1000)
    parser.add_argument('--only', choices=['qubit', 'two_qubit'])
    parser.add_argument('--out', default=os.path.join('profiles', 'periodic_second_order_time.json'))
    args = parser.parse_args()
    loop_reps = args.reps if args.loop_reps is None else args.loop_reps
    out = dict(repeats=[int(n) for n in REPEATS], kernel_trace=False,
               note='host clocks around synchronous calls; the walk is timed at walk_periods and extrapolated '
                    'linearly to the largest count')
    for name, shape in (('qubit', qubit), ('two_qubit', two_qubit)):
        if args.only in (None, name):
            make, omega, S = shape()
            out[name] = measure(make, omega, S, args.reps, loop_reps, args.walk_periods)
    text = json.dumps(out, indent=1)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()

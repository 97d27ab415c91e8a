"""The workload of the kernel trace of ff.sequence_prefix_infidelities / ff.sequence_prefix_decay_amplitudes, and the
summary of its statistics (profiles/sequence_prefixes_trace.json).

The workload is the three new calls (infidelities, diagonal, decay amplitudes; the study's two spectra stacked) on the
whole randomized-benchmarking study of tools/time_sequence_prefixes.py, --rounds times, over the 24 Cliffords and over
the 25 two-qubit gates.  Run it under the profiler in a process of its own, then summarise the kernel statistics:

    rocprofv3 --kernel-trace --stats -d DIR -o trace --output-format csv -- python tools/trace_sequence_prefixes.py
    python tools/trace_sequence_prefixes.py --summarise DIR/.../trace_kernel_stats.csv [--out FILE]

The summary keeps the kernels of the pass (front, weights, walk, reduce): launches, total, mean, shortest and longest
duration in microseconds, and the rounds and passes they belong to.
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]

KERNELS = ('seqpre_walk2_kernel', 'seqpre_walk4_kernel', 'seqpre_reduce_kernel', 'sequences_front_kernel',
           'sequences4_front_kernel', 'spectral_weights_kernel')


def workload(rounds):
    import numpy as np

    import filter_functions_amd as ff
    import workloads as wl
    from filter_functions_amd import sequence_prefixes as sx
    from time_sequence_infidelities import T, study_draws, two_qubit_gate_set
    omega = wl.rb_omega(301, T)
    S = np.stack([wl.rb_spectrum(omega, 0.0), wl.rb_spectrum(omega, 0.7)])
    cliffords = list(wl.rb_cliffords(ff, omega, T)[1])
    seqs = study_draws(np.array(cliffords, dtype=object))
    passes = {}
    run_pass = sx._run_pass

    def counting(gates, indices, close, plan, omega, S, idx, mode):
        key = f'd = {plan["d"]}, {mode}'
        passes[key] = passes.get(key, 0) + 1
        return run_pass(gates, indices, close, plan, omega, S, idx, mode)
    sx._run_pass = counting
    for gates in (cliffords, two_qubit_gate_set(omega)):
        for _ in range(rounds):
            ff.sequence_prefix_infidelities(gates, seqs, S, omega, stacked=True)
            ff.sequence_prefix_decay_amplitudes(gates, seqs, S, omega, diagonal=True, stacked=True)
            ff.sequence_prefix_decay_amplitudes(gates, seqs, S, omega, stacked=True)
    print(json.dumps({'rounds': rounds, 'sequences': len(seqs), 'positions': int(sum(len(s) for s in seqs)),
                      'n_omega': len(omega), 'spectra': len(S), 'passes_in_all_rounds': passes}))


def summarise(path, out, note):
    kernels = {}
    with open(path, newline='') as fh:
        for row in csv.DictReader(fh):
            name = next((k for k in KERNELS if k in row['Name']), None)
            if name is None:
                continue
            arguments = row['Name'].split(name, 1)[1]
            label = name + (arguments[:arguments.index('>') + 1] if arguments.startswith('<') else '')
            kernels[label] = {'launches': int(row['Calls']), 'total_us': round(int(row['TotalDurationNs'])/1e3, 1),
                              'mean_us': round(float(row['AverageNs'])/1e3, 1),
                              'min_us': round(int(row['MinNs'])/1e3, 1), 'max_us': round(int(row['MaxNs'])/1e3, 1)}
    result = {'source': 'rocprofv3 --kernel-trace --stats, one process, nothing else traced', 'kernels': kernels}
    if note:
        result['workload'] = json.loads(note)
    text = json.dumps(result, indent=1)
    with open(out, 'w') as fh:
        fh.write(text + '\n')
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--summarise', metavar='CSV', default=None)
    ap.add_argument('--workload-line', default=None, help='the JSON line the workload printed, kept in the summary')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sequence_prefixes_trace.json'))
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise, args.out, args.workload_line)
    else:
        workload(args.rounds)


if __name__ == '__main__':
    main()

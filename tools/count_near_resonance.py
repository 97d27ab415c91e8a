"""Count, on the CPU, how often the d = 4 accumulate kernel's producers meet an entry next to a resonance.

A producer wavefront generates, for one segment and 64 frequencies (lane = frequency), the 13 distinct factors
q_mn = 2 sin((w + dE_mn) dt/2)/(w + dE_mn) in two batches of table records (entries 0-7 and 8-15, the diagonal
once).  Where |w + dE_mn| < 2^-4/dt the entry is evaluated again from the short sine polynomial, and that costs
the whole wavefront as soon as one of its lanes is there (ctrl_pq.hip, ffk_math.h::phased_q).  The diagonal has
dE = 0: every frequency below 2^-4/dt is "near", for every segment.

    python tools/count_near_resonance.py [--seed 42 --G 256 --W 4096] [--omega-lo LO --omega-hi HI]

takes BASELINE config 2's inputs from workloads.py (eigenvalues from numpy.linalg.eigvalsh) and prints, per 64-frequency
tile (blockIdx.x of the kernel), the share of segments whose batch holds a near entry in any lane, and the mean
number of entries evaluated again per segment.  No GPU and no library needed.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import workloads  # noqa: E402

D = 4
BATCHES = ([e for e in range(0, 8) if e == 0 or e//D != e % D],
           [e for e in range(8, 16) if e//D != e % D])


def near_entries(eigvals, dt, omega):
    """(tiles, G, 16) bool: entry e of segment g is near for at least one frequency of the tile."""
    dE = (eigvals[:, :, None] - eigvals[:, None, :]).reshape(len(dt), D*D)
    with np.errstate(divide='ignore'):
        thr = np.where(dt > 0, 0.0625/dt, np.inf)
    n_tiles = (len(omega) + 63)//64
    out = np.zeros((n_tiles, len(dt), D*D), bool)
    for b in range(n_tiles):
        om = omega[64*b:64*b + 64]
        x = om[:, None, None] + dE[None]
        out[b] = (np.abs(x) < thr[None, :, None]).any(axis=0)
    return out


def main():
    ap = argparse.ArgumentParser()
    cfg = workloads.CONFIG2
    ap.add_argument('--seed', type=int, default=cfg['seed'])
    ap.add_argument('--G', type=int, default=cfg['G'])
    ap.add_argument('--W', type=int, default=cfg['W'])
    ap.add_argument('--omega-lo', type=float, default=None)
    ap.add_argument('--omega-hi', type=float, default=None)
    args = ap.parse_args()
    c_opers, c_coeffs, _, _, dt = workloads.random_pulse_inputs(args.seed, D, args.G, cfg['A'], cfg['n_cops'])
    omega = workloads.random_pulse_omega(dt, args.W)
    if args.omega_lo is not None or args.omega_hi is not None:
        omega = np.geomspace(omega[0] if args.omega_lo is None else args.omega_lo,
                             omega[-1] if args.omega_hi is None else args.omega_hi, args.W)
    H = np.einsum('ig,ijk->gjk', c_coeffs, c_opers)
    eigvals = np.linalg.eigvalsh(H)
    near = near_entries(eigvals, dt, omega)
    print(f'd=4 G={args.G} W={args.W} omega=[{omega[0]:.3g}, {omega[-1]:.3g}] '
          f'thr=2^-4/dt in [{0.0625/dt.max():.3g}, {0.0625/dt.min():.3g}]')
    print('tile  omega_lo   omega_hi   batch(0,8)  batch(8,16)  diagonal  redone/segment')
    share = []
    for b in range(near.shape[0]):
        om = omega[64*b:64*b + 64]
        b0 = near[b][:, BATCHES[0]].any(axis=1).mean()
        b1 = near[b][:, BATCHES[1]].any(axis=1).mean()
        diag = near[b][:, 0].mean()
        redone = near[b][:, BATCHES[0] + BATCHES[1]].sum(axis=1).mean()
        share.append((b0, redone))
        print(f'{b:4d}  {om[0]:9.3g}  {om[-1]:9.3g}  {100*b0:9.1f}%  {100*b1:10.1f}%  {100*diag:7.1f}%  {redone:8.2f}')
    share = np.array(share)
    print(f'tiles with batch(0,8) near in more than half of the segments: {(share[:, 0] > 0.5).sum()} of {len(share)}; '
          f'mean entries redone per (tile, segment): {share[:, 1].mean():.2f}')


if __name__ == '__main__':
    main()

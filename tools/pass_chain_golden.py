"""Seeded cases of the fused pass (ffk_pipeline_dev) whose outputs are pinned bit for bit, and their recorder.

    python tools/pass_chain_golden.py [--out tests/golden/pass_chain_bits.npz] [--check-separate]

Run with the library whose bits are to be kept (FFK_LIBRARY selects a build other than the package's own): every
case's D, V, Q, R, F and infidelity go into one .npz, which tests/test_pass_chain_bits.py compares with
np.array_equal.  The cases are the smallest shapes at which each path of the pass's small kernels can go wrong: no
chunk totals, exactly one chunk, a chunk boundary, the prefix tree's odd carry, several operator groups, a partial
frequency tile, forced segment chunks, every size class of the expansion's block, the non-tree prefix with more than
one batch of totals.  --check-separate also reports whether R, F and the infidelity of the fused pass equal the
separate entry points' (control matrix, filter function, infidelity) on the pass's own D, V, Q.
"""
import argparse
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import workloads  # noqa: E402

# name: (seed, d, basis, G, A, W, forced segment chunks or 0)
CASES = {
    'd4_g1_a1_w1': (101, 4, 'pauli', 1, 1, 1, 0),
    'd4_g16_a3_w16': (102, 4, 'pauli', 16, 3, 16, 0),
    'd4_g17_a3_w17': (103, 4, 'pauli', 17, 3, 17, 0),
    'd4_g49_a2_w33': (104, 4, 'pauli', 49, 2, 33, 0),
    'd4_g82_a4_w15': (105, 4, 'pauli', 82, 4, 15, 0),
    'd4_g49_a2_w33_chunks1': (104, 4, 'pauli', 49, 2, 33, 1),
    'd4_g49_a2_w33_chunks3': (104, 4, 'pauli', 49, 2, 33, 3),
    # more operators than the prologue keeps in LDS for the fold of the accumulate kernel's operand
    'd4_g17_a9_w5': (106, 4, 'pauli', 17, 9, 5, 0),
    # the spectral integral's batches of 1024 intervals: an interval that ends on the grid's last point just past
    # a batch, and three batches with a partial last one
    'd4_g3_a1_w1025': (111, 4, 'pauli', 3, 1, 1025, 0),
    'd4_g5_a2_w2500': (112, 4, 'pauli', 5, 2, 2500, 0),
    'd2_g17_a1_w40': (107, 2, 'ggm', 17, 1, 40, 0),
    'd3_g33_a2_w17': (108, 3, 'ggm', 33, 2, 17, 0),
    'd8_g33_a3_w16': (109, 8, 'pauli', 33, 3, 16, 0),
    'd12_g137_a2_w16': (110, 12, 'ggm', 137, 2, 16, 0),
}
OUTPUTS = ('D', 'V', 'Q', 'R', 'F', 'infid')
kDigestAbove = 128*1024


def golden_entry(name, key, array):
    """{fixture key: value} of one output: the array itself, or its SHA-256 where it is larger than kDigestAbove
    bytes (equal digests are equal bits; the d = 12 eigenvectors and propagators alone are 0.6 MB)"""
    array = np.ascontiguousarray(array)
    if array.nbytes > kDigestAbove:
        return {f'{name}__{key}__sha256': np.array(hashlib.sha256(array.tobytes()).hexdigest())}
    return {f'{name}__{key}': array}


def case_inputs(name):
    """(c_opers, c_coeffs, n_opers, n_coeffs, dt, basis, omega, spectrum) of a case"""
    import filter_functions_amd as ff
    seed, d, btype, G, A, W, _ = CASES[name]
    c_opers, c_coeffs, n_opers, n_coeffs, dt = workloads.random_pulse_inputs(seed, d, G, A)
    omega = workloads.random_pulse_omega(dt, W)
    basis = ff.Basis.pauli(int(np.log2(d))) if btype == 'pauli' else ff.Basis.ggm(d)
    return c_opers, c_coeffs, n_opers, n_coeffs, dt, np.asarray(basis), omega, 1e-3/omega


def run_pipeline(name):
    """One pass of the case through DevicePipeline; returns (outputs as NumPy arrays, the pipeline)."""
    import torch

    from filter_functions_amd import _lib
    from filter_functions_amd.device import DevicePipeline
    *args, omega, S = case_inputs(name)
    chunks = CASES[name][6]
    lib = _lib.load()
    try:
        _lib.check(lib.ffk_set_segment_chunks(chunks))
        pipe = DevicePipeline(*args, omega, spectrum=S)
        pipe.launch()
        torch.cuda.synchronize()
        pipe.check_status()
    finally:
        _lib.check(lib.ffk_set_segment_chunks(0))
    out = {'D': pipe.eigvals, 'V': pipe.eigvecs, 'Q': pipe.propagators, 'R': pipe.control_matrix,
           'F': pipe.filter_function, 'infid': pipe.infid}
    return {k: v.cpu().numpy() for k, v in out.items()}, pipe


def run_separate(name, pipe):
    """R, F and infidelity from the separate device entry points on the pipeline's own D, V, Q."""
    import torch

    from filter_functions_amd import _lib
    lib = _lib.load()
    p = pipe._p
    chunks = CASES[name][6]
    kw = dict(device=pipe.device)
    R = torch.empty_like(pipe.control_matrix)
    F = torch.empty_like(pipe.filter_function)
    infid = torch.empty_like(pipe.infid)
    need = lib.ffk_control_matrix_workspace_bytes(pipe.W, pipe.N, pipe.A, pipe.G, pipe.d)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, **kw)
    ineed = lib.ffk_infidelity_workspace_bytes(pipe.W, pipe.n_idx, pipe.s_ndim)
    iws = torch.empty(max(ineed, 16), dtype=torch.uint8, **kw)
    s = ctypes.c_void_p(torch.cuda.current_stream(pipe.device).cuda_stream)
    try:
        _lib.check(lib.ffk_set_segment_chunks(chunks))
        _lib.check(lib.ffk_control_matrix_dev(
            p(pipe.eigvals), p(pipe.eigvecs), p(pipe.propagators), p(pipe.omega), pipe.W, p(pipe.basis), pipe.N,
            p(pipe.n_opers), pipe.A, p(pipe.n_coeffs), p(pipe.dt), p(pipe.t), pipe.G, pipe.d, 0, p(R), None,
            p(ws), need, s))
    finally:
        _lib.check(lib.ffk_set_segment_chunks(0))
    _lib.check(lib.ffk_filter_function_dev(p(R), pipe.A, pipe.N, pipe.W, 0, p(F), s))
    _lib.check(lib.ffk_infidelity_dev(p(F), pipe.A, pipe.W, p(pipe.spectrum), pipe.s_ndim, p(pipe.omega),
                                      p(pipe.idx), pipe.n_idx, pipe.d, p(infid), p(iws), ineed, s))
    torch.cuda.synchronize()
    return {'R': R.cpu().numpy(), 'F': F.cpu().numpy(), 'infid': infid.cpu().numpy()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'pass_chain_bits.npz'))
    ap.add_argument('--check-separate', action='store_true')
    opts = ap.parse_args()
    from filter_functions_amd import _lib
    print('library:', _lib.LIB_PATH)
    record = {}
    for name in CASES:
        out, pipe = run_pipeline(name)
        for k in OUTPUTS:
            record.update(golden_entry(name, k, out[k]))
        line = f'{name:24s} ' + ' '.join(f'{k}{out[k].shape}' for k in OUTPUTS)
        if opts.check_separate:
            sep = run_separate(name, pipe)
            line += '  separate: ' + ' '.join(f'{k}={"equal" if np.array_equal(sep[k], out[k]) else "DIFFERENT"}'
                                               for k in ('R', 'F', 'infid'))
        print(line)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    np.savez_compressed(opts.out, **record)
    print(f'{opts.out}: {os.path.getsize(opts.out)} bytes')


if __name__ == '__main__':
    main()

"""The exponential of many cumulant functions in one call (``ffk_expm_real_batch``, include/ffk.h).

``ff.exponentiate_cumulant_functions(K)[i]`` is ``ff.error_transfer_matrix(cumulant_function=K[i])``: the error
transfer matrix :math:`\\exp\\mathcal{K}` of every member of a stack of cumulant functions -- the positions of many gate
sequences, the members of a parameter sweep.  The single call stages one matrix and enqueues about a dozen
launch-bound kernels between two copies and a synchronisation; the batched entry sums and exponentiates every matrix
of a chunk in one launch, one lane per matrix at N = 4 and one wavefront per matrix on the matrix cores for every other
N <= 16 (csrc/expm_batch.hip).
"""
import numpy as np

from . import _lib
from ._lib import check
from .batch import PASS_BYTES

__all__ = ['exponentiate_cumulant_functions']

#: the largest matrix the batched entry takes
MAX_N = 16


def _single(cumulant_function):
    from . import numeric
    return numeric.error_transfer_matrix(cumulant_function=cumulant_function)


def _loop(cumulant_functions):
    """The loop's expression, with the single function's exceptions; nothing to stack is an empty float array."""
    values = [_single(k) for k in cumulant_functions]
    return np.stack(values) if values else np.empty((0, 0, 0), dtype=np.float64)


def _stack(cumulant_functions):
    """The input as one array (n, ..., N, N) that the batched entry takes, or None: arrays of one shape and of a dtype
    whose sum is the sum of its values as doubles."""
    if isinstance(cumulant_functions, np.ndarray):
        stack = cumulant_functions
    else:
        members = list(cumulant_functions)
        if not members or not all(isinstance(k, np.ndarray) for k in members):
            return None
        if len({(k.shape, k.dtype) for k in members}) != 1:
            return None
        stack = np.stack(members)
    if stack.ndim < 3 or not (stack.dtype == np.float64 or stack.dtype.kind in 'iub'):
        return None
    N = stack.shape[-1]
    if stack.shape[-2] != N or not 1 <= N <= MAX_N or 0 in stack.shape[1:]:
        return None
    return stack


def chunk_length(rows, N, budget=None):
    """Matrices of one call of the entry: what *budget* (default: ``PASS_BYTES``, read at the call) holds of their
    tiles, results and flags, one at least."""
    budget = PASS_BYTES if budget is None else budget
    return max(1, int(budget)//(8*rows*N*N + 8*N*N + 4))


def _run(tiles):
    """``ffk_expm_real_batch`` over tiles (n, rows, N, N) f64, C-contiguous, in chunks: (result (n, N, N), not_finite
    (n,) int32)."""
    n, rows, N = tiles.shape[:3]
    out = np.empty((n, N, N), dtype=np.float64)
    flags = np.empty(n, dtype=np.int32)
    entry = _lib.load().ffk_expm_real_batch
    step = chunk_length(rows, N)
    for lo in range(0, n, step):
        part, res, bad = tiles[lo:lo + step], out[lo:lo + step], flags[lo:lo + step]
        check(entry(part.ctypes.data, len(part), rows, N, res.ctypes.data, bad.ctypes.data))
    return out, flags


def exponentiate_cumulant_functions(cumulant_functions):
    r"""Error transfer matrices :math:`\exp\mathcal{K}` of many cumulant functions: for an input of shape
    (n, ..., N, N) an array (n, N, N) whose entry i is

    ``ff.error_transfer_matrix(cumulant_function=cumulant_functions[i])``

    -- every member summed over all but its last two axes, in order, and exponentiated --, that is
    ``np.stack([ff.error_transfer_matrix(cumulant_function=k) for k in cumulant_functions])``, with that function's
    exceptions for members of a bad type or shape.  An empty input gives an empty float array.

    Real input (float64 or integers) with N <= 16, as one array or a sequence of arrays of one shape, is flattened to
    (n, rows, N, N) and goes through ``ffk_expm_real_batch`` in chunks of what ``batch.PASS_BYTES`` holds: one H2D
    copy, one launch and the copies of the results and flags back per chunk, one lane per matrix at N = 4, one
    wavefront per matrix on the matrix cores else.  The arithmetic plan is that of the single function (1-norm,
    halvings, Taylor polynomial of degree 18, squarings) with another order of the sums inside the products: the
    values agree with it to rounding, not bit for bit.  A matrix's result is the same bits alone or among others, at
    any place of the stack and in any split into chunks.  Complex input, other dtypes, N > 16, members of several
    shapes and every matrix whose sum is not finite evaluate the single function per matrix inside the call."""
    stack = _stack(cumulant_functions)
    if stack is None:
        return _loop(cumulant_functions)
    n, N = stack.shape[0], stack.shape[-1]
    if n == 0:
        return np.empty((0, N, N), dtype=np.float64)
    tiles = np.ascontiguousarray(stack.reshape(n, -1, N, N), dtype=np.float64)
    out, flags = _run(tiles)
    for i in np.flatnonzero(flags):
        out[i] = _single(stack[i])
    return out

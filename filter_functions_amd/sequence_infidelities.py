"""Infidelities of many gate sequences given as index arrays into one gate set (``ffk_sequence_infidelities``,
include/ffk.h).

``ff.sequence_infidelities(gates, sequences, spectrum, omega)`` is the loop ``np.stack([ff.infidelity(ff.concatenate(
gates[s], omega=omega), spectrum, omega) for s in sequences])`` of a randomized-benchmarking study that wants one
number per sequence: no ``PulseSequence`` is built for a sequence, so none of the bookkeeping of ``ff.concatenate``
(merged control Hamiltonians, identifiers, segment tables) runs.  The infidelity needs each gate's control matrix,
total propagator and duration only, and whether the gates' noise operators line up is a property of the gate set:
it is checked once per call.  An eligible gate set -- single-qubit (d = 2) or two-qubit (d = 4) gates, see
:func:`eligibility` -- runs in passes of one H2D copy, three launches whatever the number of sequences and one D2H
copy; the sequences' control matrices are never written to memory.  Every other gate set runs the loop's expression.
"""
import numpy as np

from . import _lib, util
from ._gate_table import PassTable, _on_grid, batched_plan, eligibility, index_arrays, validated  # noqa: F401
from ._lib import as_f64, check
from ._resident import spectrum_arguments
from .batch import MAX_PULSES, PASS_BYTES, split_passes

__all__ = ['sequence_infidelities']


def pass_bytes(max_length, d, A, W, n_out):
    """Device bytes one sequence adds to a pass at most: its filter function, results and positions."""
    return 16*A*A*W + 8*n_out + 16*d*d + 8 + 4*max_length + 4*64


def table_bytes(n_gates, d, A, W):
    """Device bytes of what a pass holds once whatever its sequences: the gate table and the gates' phases,
    propagators and Liouville representations."""
    N = d*d
    return n_gates*(16*A*N*W + 16*W + 8*N*N + 16*N + 16 + 64) + 16*N*N + 16*A*A*W + 8*W + 4096


def _run_pass(gates, indices, plan, omega, S, idx, want_U, want_F):
    """One pass over the sequences *indices* (int32 arrays into *gates*): (infidelities or None, total propagators or
    None, filter functions or None)."""
    d, A = plan['d'], plan['A']
    W, P = len(omega), len(indices)
    table = PassTable(gates, indices, plan, omega)
    infid = total = F = None
    args = [None, 0, 0, None, 0]
    if S is not None:
        S, real, idx, out_shape = spectrum_arguments(S, idx)
        infid = np.empty((P,) + out_shape, dtype=np.float64)
        args = [S.ctypes.data, S.ndim, real, idx.ctypes.data, len(idx)]
    if want_U:
        total = np.empty((P, d, d), dtype=np.complex128)
    if want_F:
        F = np.empty((P, A, A, W), dtype=np.complex128)
    check(_lib.load().ffk_sequence_infidelities(
        *table.c_arguments(), *args, d, None if infid is None else infid.ctypes.data,
        None if total is None else total.ctypes.data, None if F is None else F.ctypes.data))
    return infid, total, F


def _loop(gates, indices, spectrum, omega, n_oper_identifiers, want_U, want_F):
    """The loop's expression for every sequence."""
    import filter_functions_amd as ff         # (the public names, as a caller's loop reads them)
    table = np.empty(len(gates), dtype=object)
    table[:] = gates
    infid, total, F = [], [], []
    for i in indices:
        pulse = ff.concatenate(table[i], omega=omega)
        infid.append(ff.infidelity(pulse, spectrum, omega, n_oper_identifiers=n_oper_identifiers))
        if want_U:
            total.append(np.array(pulse.total_propagator))
        if want_F:
            F.append(np.array(pulse.get_filter_function(omega)))
    return np.stack(infid), np.stack(total) if want_U else None, np.stack(F) if want_F else None


def sequence_infidelities(gates, sequences, spectrum, omega, n_oper_identifiers=None, return_propagators=False,
                          return_filter_functions=False):
    r"""Infidelities of many sequences of gates drawn from one gate set:

    ``np.stack([ff.infidelity(ff.concatenate(np.asarray(gates, dtype=object)[s], omega=omega), spectrum, omega,
    n_oper_identifiers=n_oper_identifiers) for s in sequences])``

    with the loop's values and its exceptions for a bad spectrum or bad identifiers: shape (P, n_idx), or (P, n_idx,
    n_idx) for a cross-spectrum (n_idx, n_idx, n_omega).

    *gates* is a sequence of T ``PulseSequence`` objects, *sequences* a list of P one-dimensional integer arrays of
    indices into it, with the rules of indexing an object array: negative indices wrap, others out of range raise
    IndexError.  An empty sequence (or no sequence at all) raises ValueError, an index that is no integer TypeError.
    With *return_propagators* and *return_filter_functions* the total propagators (P, d, d) and the fidelity filter
    functions (P, n_nops, n_nops, n_omega) are returned as well, as host arrays the caller owns: ``(infidelities[,
    propagators][, filter_functions])``.

    The gate set takes the batched route if all gates have d = 2 or all have d = 4, share one Hermitian, traceless
    basis of d^2 elements, carry identical noise-operator identifiers -- one to four, unique, in sorted order --
    with equal operator arrays, and every gate knows its total propagator.  This is checked once per call, not per
    sequence.  Then no ``PulseSequence`` is created and no gate's cache is touched, with one exception: gates whose
    control matrix is not cached on *omega* are completed first by ONE ``ff.get_filter_functions(missing, omega)``
    call, which leaves in their caches what ``gate.get_filter_function(omega)`` leaves.  Gates whose control matrix
    is resident in HBM (a single resident result, a member of an ``ff.get_filter_functions`` batch, for d = 2 a
    result of ``ff.concatenate_sequences``) are read in place, the others' control matrices are uploaded once per
    pass.  A pass is one H2D copy, three launches whatever the number of sequences and one D2H copy; a sequence's
    result is the same bits whatever else is in the call.  Single-qubit sequences run the kernels and the arithmetic
    of ``ff.infidelities(ff.concatenate_sequences(...))``; two-qubit sequences run the 16 x 16 product of the
    concatenation rule on the FP64 matrix cores.

    Every other gate set evaluates the loop's expression for every sequence inside this call.
    """
    gates, indices = validated(gates, sequences)
    want_U, want_F = bool(return_propagators), bool(return_filter_functions)

    def answer(infid, total, F):
        extras = ([total] if want_U else []) + ([F] if want_F else [])
        return (infid, *extras) if extras else infid
    plan = batched_plan(gates, omega)
    if plan is None:
        return answer(*_loop(gates, indices, spectrum, omega, n_oper_identifiers, want_U, want_F))
    omega = as_f64(omega)
    d, A, W, P = plan['d'], plan['A'], len(omega), len(indices)
    idx = np.asarray(util.get_indices_from_identifiers(gates[0].n_oper_identifiers, n_oper_identifiers))
    S = util.parse_spectrum(np.asanyarray(spectrum), omega, idx)
    n_idx = len(idx)
    out_shape = (n_idx, n_idx) if S.ndim == 3 else (n_idx,)
    infid = np.zeros((P,) + out_shape, dtype=np.float64)
    if W < 2 or n_idx < 1:
        S = None                                  # (no integral: zeros, as ff.infidelity gives them)
        if not (want_U or want_F):
            return infid
    total = np.empty((P, d, d), dtype=np.complex128) if want_U else None
    F = np.empty((P, A, A, W), dtype=np.complex128) if want_F else None
    longest = max(len(i) for i in indices)
    per_sequence = pass_bytes(longest, d, A, W, int(np.prod(out_shape)))
    budget = max(PASS_BYTES - table_bytes(len(gates), d, A, W), 2*per_sequence)
    for chunk in split_passes(list(range(P)), per_sequence, budget, MAX_PULSES):
        part = _run_pass(gates, [indices[i] for i in chunk], plan, omega, S, idx, want_U, want_F)
        for whole, piece in zip((infid, total, F), part):
            if piece is not None:
                whole[chunk[0]:chunk[-1] + 1] = piece
    return answer(infid, total, F)

"""Pulse-correlation infidelities of many gate sequences given as index arrays into one gate set
(``ffk_sequence_correlation_infidelities`` and ``ffk_sequence_correlation_infidelities4``, include/ffk.h).

``ff.sequence_correlation_infidelities(gates, sequences, spectrum, omega)`` is the loop ``[ff.infidelity(ff.concatenate(
gates[s], calc_pulse_correlation_FF=True, omega=omega), spectrum, omega, which='correlations') for s in sequences]``
of a randomized-benchmarking study that asks what every gate pair of a sequence contributes to its infidelity: one
array ``I[g, h, a]`` per sequence.  As in :mod:`filter_functions_amd.sequence_infidelities` no ``PulseSequence`` is
built for a sequence and whether the gates' noise operators line up is checked once per call; an eligible gate set --
single-qubit (d = 2) or two-qubit (d = 4) gates -- runs in passes of one H2D copy, five to eight launches whatever the
number of sequences and one D2H copy.  Neither the summands of the concatenation rule nor the pulse-correlation
filter function (G, G, A, A, W) exist anywhere.  Everything else runs the loop's expression.
"""
import numpy as np

from . import _lib, util
from ._gate_table import PassTable, batched_plan, validated
from ._lib import as_f64, check
from ._resident import spectrum_arguments
from .batch import MAX_PULSES, PASS_BYTES, split_passes
from .correlations import MAX_LENGTH, output_offsets, slabs
from .sequence_infidelities import eligibility, index_arrays  # noqa: F401

__all__ = ['sequence_correlation_infidelities']


def pass_bytes(max_length, d, A, W, n_idx):
    """Device bytes one sequence of *max_length* positions adds to a pass at most: its CSR entry and total
    propagator, per position the gate number and the accumulated d^2 x d^2 Liouville propagator, and its output with
    one partial result per frequency slab.  The output is counted as the workspace query counts it, which does not
    know the lengths: ``MAX_LENGTH`` cells per position."""
    N = d*d
    return (16 + 16*N + (4 + 8*N*N)*max_length + 8*max_length*MAX_LENGTH*n_idx*(1 + slabs(W)))


def table_bytes(n_gates, d, A, W):
    """Device bytes of what a pass holds once whatever its sequences: the gate table, the gates' durations, phases,
    propagators and Liouville representations, the grid, the basis, the spectrum and its weights, and the padding
    between the arrays."""
    N = d*d
    return n_gates*(16*A*N*W + 16*W + 8*N*N + 16*N + 16) + 8*W + 16*N*N + 32*A*W + 16 + 8192


def _loop(table, index, spectrum, omega, n_oper_identifiers):
    """The loop's expression for one sequence."""
    import filter_functions_amd as ff         # (the public names, as a caller's loop reads them)
    seq = ff.concatenate(table[index], calc_pulse_correlation_FF=True, omega=omega)
    return ff.infidelity(seq, spectrum, omega, n_oper_identifiers=n_oper_identifiers, which='correlations')


def _run_pass(gates, indices, plan, omega, S, idx):
    """One pass over the sequences *indices* (int32 arrays into *gates*): the list of their (G, G, n_idx) arrays."""
    d = plan['d']
    lengths = [len(i) for i in indices]
    if len(omega) < 2:
        return [np.zeros((G, G, len(idx))) for G in lengths]
    table = PassTable(gates, indices, plan, omega)
    out_offsets = output_offsets(lengths)
    S, real, idx, _ = spectrum_arguments(S, idx)
    out = np.empty((int(out_offsets[-1]), len(idx)), dtype=np.float64)
    lib = _lib.load()
    entry = lib.ffk_sequence_correlation_infidelities if d == 2 else lib.ffk_sequence_correlation_infidelities4
    check(entry(*table.c_arguments(), S.ctypes.data, S.ndim, real, idx.ctypes.data, len(idx), d,
                out_offsets.ctypes.data, out.ctypes.data))
    return [out[a:b].reshape(G, G, len(idx)) for a, b, G in zip(out_offsets[:-1], out_offsets[1:], lengths)]


def _real_spectrum(gates, spectrum, omega, n_oper_identifiers):
    """(idx, S) for the batched route -- the selected noise operators and the validated spectrum of one or two
    dimensions as float64 --, or None if the loop's expression is to run (cross-spectra, an imaginary part, no
    operator selected).  Raises what the loop raises for unknown identifiers or a spectrum that does not fit."""
    idx = np.asarray(util.get_indices_from_identifiers(gates[0].n_oper_identifiers, n_oper_identifiers))
    S = util.parse_spectrum(np.asanyarray(spectrum), omega, idx)
    if len(idx) < 1 or S.ndim > 2 or S.dtype.kind not in 'fiuc':
        return None
    if np.iscomplexobj(S):
        if np.any(S.imag != 0):      # Re(S F) then needs the imaginary part of the Gram matrix as well
            return None
        S = S.real
    return np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(S, dtype=np.float64)


def sequence_correlation_infidelities(gates, sequences, spectrum, omega, n_oper_identifiers=None):
    r"""Pulse-correlation infidelities of many sequences of gates drawn from one gate set: the list

    ``[ff.infidelity(ff.concatenate(np.asarray(gates, dtype=object)[s], calc_pulse_correlation_FF=True, omega=omega),
    spectrum, omega, n_oper_identifiers=n_oper_identifiers, which='correlations') for s in sequences]``

    with the loop's values and its exceptions for a bad spectrum or bad identifiers: one array ``I[g, h, a]`` of shape
    (G, G, n_idx) per sequence, in input order, :math:`I_{gh\alpha} = \frac{1}{2\pi d}\int d\omega\,
    S_\alpha(\omega)\,\mathrm{Re}\sum_k \bar X_g[\alpha,k,\omega] X_h[\alpha,k,\omega]` over the summands
    :math:`X_g` of the concatenation rule; its sum over (g, h) is the sequence's infidelity.

    *gates* and *sequences* are those of :func:`ff.sequence_infidelities <filter_functions_amd.sequence_infidelities.
    sequence_infidelities>`, with its index rules: negative indices wrap, others out of range raise IndexError, an
    empty sequence (or no sequence at all) raises ValueError, an index that is no integer TypeError.  So are the
    eligibility of the gate set, checked once per call -- all gates d = 2 or all d = 4, one Hermitian, traceless
    basis of d^2 elements, identical sorted noise identifiers, one to four, with equal operator arrays, every gate's
    total propagator known -- and the completion step: gates whose control matrix is not cached on *omega* are
    completed first by ONE ``ff.get_filter_functions(missing, omega)`` call.  Beyond that no gate's cache is touched
    and no ``PulseSequence`` is created on the batched route, which a sequence of an eligible set takes if it has 2 to
    256 gates and *spectrum* has one or two dimensions and no imaginary part.  Gates whose control matrix is resident
    in HBM are read in place, the others' are uploaded once per pass, and only the gates a pass uses are in its
    table.  Single-qubit sequences run the kernels of ``ff.correlation_infidelities`` and return its bits; two-qubit
    sequences generate the summands in LDS and accumulate the Gram matrix of the positions on the FP64 matrix
    cores, eight steps of 16 x 16 x 4 per tile pair and frequency.  A sequence's result is the same bits whatever
    else is in the call, and exactly symmetric in (g, h).

    Every other sequence -- one gate, more than 256 gates, cross-spectra (n_idx, n_idx, n_omega) --, and every
    sequence of an ineligible gate set, evaluates the loop's expression inside this call.
    """
    gates, indices = validated(gates, sequences)
    table = np.empty(len(gates), dtype=object)
    table[:] = gates
    plan = batched_plan(gates, omega)
    selected = None
    if plan is not None:
        grid = as_f64(omega)
        selected = _real_spectrum(gates, spectrum, grid, n_oper_identifiers)
    if selected is None:
        return [_loop(table, i, spectrum, omega, n_oper_identifiers) for i in indices]
    idx, S = selected
    d, A, W = plan['d'], plan['A'], len(grid)
    out = [None]*len(indices)
    batched = [p for p, i in enumerate(indices) if 2 <= len(i) <= MAX_LENGTH]
    for p, i in enumerate(indices):
        if not 2 <= len(i) <= MAX_LENGTH:
            out[p] = _loop(table, i, spectrum, omega, n_oper_identifiers)
    if batched:
        longest = max(len(indices[p]) for p in batched)
        per_sequence = pass_bytes(longest, d, A, W, len(idx))
        budget = max(PASS_BYTES - table_bytes(len(gates), d, A, W), 2*per_sequence)
        for chunk in split_passes(batched, per_sequence, budget, MAX_PULSES):
            for p, result in zip(chunk, _run_pass(gates, [indices[p] for p in chunk], plan, grid, S, idx)):
                out[p] = result
    return out

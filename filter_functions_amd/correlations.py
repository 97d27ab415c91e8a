"""Pulse-correlation infidelities of many gate sequences in one pass (``ffk_sequence_correlation_infidelities``,
include/ffk.h).

``ff.correlation_infidelities(sequences, spectrum)`` is the loop ``[ff.infidelity(ff.concatenate(s,
calc_pulse_correlation_FF=True), spectrum, omega, which='correlations') for s in sequences]``: for every sequence the
array ``I[g, h, a]`` of what its gate pair (g, h) contributes to its infidelity on noise operator a.  Sequences that
:func:`filter_functions_amd.sequences._plan` accepts, of 2 to :data:`MAX_LENGTH` gates, with a spectrum of one or two
dimensions, are grouped by frequency grid, basis, number of noise operators and selected operators; every group runs
in passes: one H2D copy of the sequences (CSR), the gate table rows that are not resident and the small inputs, at most
eight launches whatever the number of sequences, one D2H copy of the ragged result.  Neither the summands of the
concatenation rule nor the pulse-correlation filter function (G, G, A, A, W) exist anywhere.  Every other sequence
runs the loop's expression.
"""
import numpy as np

from . import _lib, util
from ._gate_table import staged_gates
from ._lib import as_c128, as_f64, check
from ._resident import spectrum_arguments
from .batch import MAX_PULSES, PASS_BYTES, split_passes
from .sequences import _plan, group_plans, pack_sequences

__all__ = ['correlation_infidelities']

#: The longest sequence of the batched route: sixteen tiles of sixteen positions, whose 136 upper tile pairs are the
#: accumulators one block keeps in registers.
MAX_LENGTH = 256


def output_offsets(lengths):
    """(P + 1) int64 prefix sums of G_p^2: where each sequence's (G_p, G_p, n_idx) block starts in the ragged output."""
    out = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lengths, dtype=np.int64)**2, out=out[1:])
    return out


def slabs(W):
    """Number of frequency slabs whose partial results a pass keeps per sequence (a function of W alone)."""
    width = 16*(-(-W//512))
    return -(-W//width)


def pass_bytes(max_length, A, W, n_gates, n_idx):
    """Device bytes one sequence adds to a pass at most: its output G^2 n_idx doubles, one partial result of that size
    per frequency slab, its positions (CSR entry, the accumulated 4 x 4 Liouville propagator) and a share of the gate
    table (the table of a pass holds at most this sequence's own distinct gates more)."""
    return (8*max_length**2*n_idx*(1 + slabs(W)) + (4 + 8*16)*max_length
            + 16*A*4*W*min(n_gates, max_length) + 128)


def _loop(pulses, spectrum, omega, n_oper_identifiers):
    """The loop's expression for one sequence."""
    import filter_functions_amd as ff         # (the public names, as a caller's loop reads them)
    seq = ff.concatenate(pulses, calc_pulse_correlation_FF=True, omega=omega)
    return ff.infidelity(seq, spectrum, seq.omega if omega is None else omega,
                         n_oper_identifiers=n_oper_identifiers, which='correlations')


def _batched_plan(pulses, distinct, first, index, spectrum, omega, n_oper_identifiers):
    """What the batched route needs of one validated sequence (the plan of ``sequences._plan`` with ``idx`` and the
    validated real ``spectrum``), or None if the loop's expression is to run it."""
    if not 2 <= len(pulses) <= MAX_LENGTH or np.ndim(spectrum) > 2:
        return None
    plan = _plan(pulses, distinct, first, index, True, 'fidelity', omega)
    if plan is None:
        return None
    try:
        idx = util.get_indices_from_identifiers(plan['pulse'].n_oper_identifiers, n_oper_identifiers)
        S = util.parse_spectrum(spectrum, as_f64(plan['omega']), idx)
    except ValueError:
        return None                  # (the loop raises it)
    if len(idx) < 1 or S.ndim > 2 or S.dtype.kind not in 'fiuc':
        return None
    if np.iscomplexobj(S):
        if np.any(S.imag != 0):      # Re(S F) then needs the imaginary part of the Gram matrix as well
            return None
        S = S.real
    plan.update(idx=np.ascontiguousarray(idx, dtype=np.int32), spectrum=np.ascontiguousarray(S, dtype=np.float64))
    return plan


def _run_pass(plans, members):
    """One pass over ``plans[i] for i in members``: the list of their (G, G, n_idx) arrays."""
    group = [plans[i] for i in members]
    first = group[0]
    omega, A, idx = as_f64(first['omega']), first['A'], first['idx']
    W = len(omega)
    lengths = [len(plan['index']) for plan in group]
    if W < 2:
        return [np.zeros((G, G, len(idx))) for G in lengths]
    slot_of, gates = {}, []
    for plan in group:
        for gate in plan['distinct']:
            if id(gate) not in slot_of:
                slot_of[id(gate)] = len(gates)
                gates.append(gate)
    handles, slots, table, U, tau = staged_gates(gates, omega, 2, 4, A)
    indices = [np.array([slot_of[id(g)] for g in plan['distinct']], dtype=np.int32)[plan['index']] for plan in group]
    offsets, index, _ = pack_sequences(indices)
    out_offsets = output_offsets(lengths)
    S, real, idx, _ = spectrum_arguments(first['spectrum'], idx)
    basis = as_c128(np.asarray(first['basis']))
    out = np.empty((int(out_offsets[-1]), len(idx)), dtype=np.float64)
    check(_lib.load().ffk_sequence_correlation_infidelities(
        handles, slots.ctypes.data, None if table is None else table.ctypes.data, U.ctypes.data, tau.ctypes.data,
        len(gates), offsets.ctypes.data, index.ctypes.data, len(group), omega.ctypes.data, W, basis.ctypes.data, 1,
        basis.shape[-1], A, len(basis), S.ctypes.data, S.ndim, real, idx.ctypes.data, len(idx), int(first['pulse'].d),
        out_offsets.ctypes.data, out.ctypes.data))
    return [out[a:b].reshape(G, G, len(idx)) for a, b, G in zip(out_offsets[:-1], out_offsets[1:], lengths)]


def _group_by_idx(plans):
    """``group_plans`` groups, split further by the selected noise operators, each in input order."""
    groups = []
    for members in group_plans(plans):
        by_idx = {}
        for i in members:
            by_idx.setdefault(tuple(plans[i]['idx']), []).append(i)
        groups.extend(by_idx.values())
    return groups


def correlation_infidelities(sequences, spectrum, omega=None, n_oper_identifiers=None):
    r"""Pulse-correlation infidelities of many sequences of pulses: the list

    ``[ff.infidelity(ff.concatenate(s, calc_pulse_correlation_FF=True, omega=omega), spectrum, <that pulse's omega>,
    n_oper_identifiers=n_oper_identifiers, which='correlations') for s in sequences]``

    with the same results and exceptions: one array ``I[g, h, a]`` of shape (G, G, n_idx) per sequence, in input
    order, :math:`I_{gh\alpha} = \frac{1}{2\pi d}\int d\omega\, S_\alpha(\omega)\,\mathrm{Re}\sum_k
    \bar X_g[\alpha,k,\omega] X_h[\alpha,k,\omega]` over the summands :math:`X_g` of the concatenation rule; its sum
    over (g, h) is the sequence's infidelity.

    A sequence takes the batched route if ``ff.concatenate_sequences`` would take it for the fidelity filter
    function -- single-qubit gates (d = 2) in a Hermitian basis, at most four noise operators, every gate carrying
    every noise operator of the new pulse in its order, every gate's control matrix and total propagator known on the
    grid --, if it has 2 to 256 gates and if *spectrum* has one or two dimensions and no imaginary part.  Such
    sequences are grouped by frequency grid, basis, noise operators and *n_oper_identifiers* and evaluated in passes
    of at most eight launches whatever their number; gates whose control matrix is resident in HBM are read in place.  The
    summands and the pulse-correlation filter function are never formed.

    Every other sequence -- cross-spectra (n_idx, n_idx, n_omega) among them -- runs the loop's expression inside
    this call, which materialises the pulse-correlation filter function (G, G, n_nops, n_nops, n_omega) on the host
    and integrates it one gate pair at a time.
    """
    from .pulse_sequence import _validated_sequence
    out, plans, where = [], [], []
    for sequence in sequences:
        pulses, distinct, first, index = _validated_sequence(sequence)
        plan = _batched_plan(pulses, distinct, first, index, spectrum, omega, n_oper_identifiers)
        if plan is None:
            out.append(_loop(pulses, spectrum, omega, n_oper_identifiers))
        else:
            out.append(None)
            where.append(len(out) - 1)
            plans.append(plan)
    for members in _group_by_idx(plans):
        first = plans[members[0]]
        longest = max(len(plans[i]['index']) for i in members)
        per_sequence = pass_bytes(longest, first['A'], len(first['omega']), len(first['distinct']), len(first['idx']))
        for chunk in split_passes(members, per_sequence, PASS_BYTES, MAX_PULSES):
            for i, result in zip(chunk, _run_pass(plans, chunk)):
                out[where[i]] = result
    return out

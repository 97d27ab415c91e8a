"""Infidelities and decay amplitudes along many gate sequences given as index arrays into one gate set: the result
after 1, 2, ..., G gates of every sequence, optionally with a closing gate behind each truncation
(``ffk_sequence_prefix_processes``, include/ffk.h).

``ff.sequence_prefix_infidelities(gates, sequences, spectrum, omega)[p][m - 1]`` is ``ff.infidelity`` of
``ff.concatenate(gates[s_p[:m]], omega=omega)``, ``ff.sequence_prefix_decay_amplitudes`` the same for
``numeric.calculate_decay_amplitudes``: the decay curve of a randomized-benchmarking or dynamical-decoupling sequence.
The loop over the truncations, and the truncations handed to :mod:`~filter_functions_amd.sequence_infidelities` or
:mod:`~filter_functions_amd.sequence_processes` as separate sequences, walk G (G + 1) / 2 positions per sequence.  The
concatenation rule is a sum over the positions, so the control matrix of a truncation is the partial sum that a forward
walk holds in registers: the batched route walks every sequence once and adds one epilogue per position.
"""
import numpy as np

from . import _lib, util
from ._gate_table import PassTable, batched_plan, index_arrays, validated
from ._lib import as_f64, check
from .batch import MAX_PULSES, PASS_BYTES
from .sequence_processes import _real_weights, stacked_spectra

__all__ = ['sequence_prefix_infidelities', 'sequence_prefix_decay_amplitudes', 'sequence_prefix_propagators']

_MODES = {'infidelities': 0, 'diagonal': 1, 'decay_amplitudes': 2}
#: Spectra that share one walk of the sequences (``sequence_prefix_spectra_per_walk``); further ones repeat it.
SPECTRA_PER_WALK = 2


def block_width(d, A):
    """Frequencies of one block of the walk (``sequence_prefix_block_width``): a function of d and A alone."""
    return 64 if d == 2 or A <= 2 else 32


def _tiles(N, mode):
    """Doubles of one (position, spectrum, operator): (in the result, in a frequency block's partial sums)."""
    return {0: (1, N), 1: (N, N), 2: (N*N, N*N)}[_MODES[mode]]


def pass_bytes(d, A, W, n_idx, n_spectra, mode, closing):
    """Device bytes one POSITION adds to a pass: its index (and closing index), its part of the result and of the
    frequency blocks' partial sums."""
    out, partial = _tiles(d*d, mode)
    blocks = -(-W//block_width(d, A))
    return 4 + (4 if closing else 0) + 8*n_spectra*n_idx*(out + blocks*partial)


def sequence_bytes(d):
    """Device bytes one sequence adds to a pass whatever its length: its offset, its place in the dealing order and
    its total propagator."""
    return 8 + 16*d*d


def table_bytes(n_gates, d, A, W, n_idx, n_spectra, s_ndim):
    """Device bytes of what a pass holds once whatever its sequences: the gate table, the gates' phases, propagators
    and Liouville representations, the spectra and their weights, the basis."""
    N, dd = d*d, d*d
    rows = n_spectra*(1 if s_ndim == 1 else n_idx)
    return (n_gates*(16*A*N*W + 16*W + 8*N*N + 16*dd + 16) + 16*N*dd + 8*W + 32*rows*W + 4*n_idx + 4 + 20*256)


def staged(d, n_gates, A):
    """Whether a pass over *n_gates* gates keeps their tables in LDS (``sequence_prefix_staged``): the control matrices
    and phases of one block's frequencies, at d = 4 with the block's weights in front, in at most 150 KiB.  Else the
    walk reads them from L2.  The arithmetic is the same either way."""
    width = block_width(d, A)
    weights = 0 if d == 2 else 8*SPECTRA_PER_WALK*A*width
    return 16*n_gates*(A*d*d + 1)*width + weights <= 150*1024


def split_sequences(lengths, per_position, per_sequence, budget, max_sequences=MAX_PULSES):
    """The sequences 0 ... len(lengths) - 1 in consecutive passes, whole sequences each: a pass takes sequences while
    ``sum(per_sequence + length*per_position)`` stays within *budget* and their number within *max_sequences*, and at
    least one.  A list of lists of sequence numbers."""
    passes, used = [], 0
    for p, length in enumerate(lengths):
        need = per_sequence + length*per_position
        if not passes or used + need > budget or len(passes[-1]) >= max_sequences:
            passes.append([])
            used = 0
        passes[-1].append(p)
        used += need
    return passes


def _closing_arrays(closing, indices, n_gates):
    """*closing* as int32 arrays in [0, n_gates), one per sequence and as long as it, or None."""
    if closing is None:
        return None
    closing = list(closing)
    if len(closing) != len(indices):
        raise ValueError(f'closing holds {len(closing)} arrays for {len(indices)} sequences.')
    for p, (c, i) in enumerate(zip(closing, indices)):
        if np.ndim(c) != 1 or len(c) != len(i):
            raise ValueError(f'closing[{p}]: expected {len(i)} gate indices, one behind every position of sequence '
                             f'{p}, not shape {np.shape(c)}.')
    out = []
    for p, c in enumerate(closing):
        try:
            out.extend(index_arrays([c], n_gates))
        except (IndexError, TypeError, ValueError) as error:
            # (the rules and texts of the index arrays, naming the argument that is wrong)
            raise type(error)(str(error).replace('Sequence 0', f'closing[{p}]', 1)) from None
    return out


def _products(U, indices, close):
    """The propagators of every truncation from the gates' propagators U (T, d, d): a loop over the positions,
    vectorised over the sequences."""
    P, d = len(indices), U.shape[-1]
    lengths = np.array([len(i) for i in indices])
    longest = int(lengths.max())
    padded = np.zeros((P, longest), dtype=np.int64)
    closers = np.zeros((P, longest), dtype=np.int64)
    for p, i in enumerate(indices):
        padded[p, :len(i)] = i
        if close is not None:
            closers[p, :len(i)] = close[p]
    out = np.empty((P, longest, d, d), dtype=np.complex128)
    current = np.broadcast_to(np.eye(d, dtype=np.complex128), (P, d, d)).copy()
    for g in range(longest):
        alive = np.flatnonzero(lengths > g)
        current[alive] = U[padded[alive, g]] @ current[alive]
        out[alive, g] = current[alive] if close is None else U[closers[alive, g]] @ current[alive]
    return [out[p, :n].copy() for p, n in enumerate(lengths)]


def sequence_prefix_propagators(gates, sequences, closing=None):
    """The total propagators of every truncation of many sequences of gates drawn from one gate set: a list of P
    arrays (G_p, d, d) whose row m - 1 is the propagator of ``gates[s_p[:m]]``, the gate ``gates[closing[p][m - 1]]``
    applied behind it if *closing* is given.  Computed on the host from the gates' ``total_propagator``; what a
    user needs to pick the inverting gates of a randomized-benchmarking sequence.  *gates*, *sequences* and *closing*
    are read as :func:`sequence_prefix_infidelities` reads them."""
    gates, indices = validated(gates, sequences)
    close = _closing_arrays(closing, indices, len(gates))
    return _products(np.array([np.asarray(g.total_propagator) for g in gates], dtype=np.complex128), indices, close)


def _run_pass(gates, indices, close, plan, omega, S, idx, mode):
    """One call of ``ffk_sequence_prefix_processes`` over the sequences *indices* (int32 arrays into *gates*), their
    closing gates *close* (the same, or None) and the spectra S (K, W) or (K, n_idx, W): the values of every global
    position, (K, n_index, n_idx[, N[, N]])."""
    N, K = plan['N'], len(S)
    table = PassTable(gates, indices, plan, omega, extra=close)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    n_idx = len(idx)
    n_index = int(table.offsets[-1])
    shape = {0: (), 1: (N,), 2: (N, N)}[_MODES[mode]]
    out = np.empty((K, n_index, n_idx) + shape, dtype=np.float64)
    check(_lib.load().ffk_sequence_prefix_processes(
        *table.c_arguments(), None if table.extra is None else table.extra.ctypes.data, S.ctypes.data, S.ndim - 1, K,
        idx.ctypes.data, n_idx, _MODES[mode], out.ctypes.data))
    return out


def _concatenated(gates, sequence, closer, omega):
    """The loop's pulse of one truncation (*closer*: the gate appended behind it, or None)."""
    import filter_functions_amd as ff         # (the public names, as a caller's loop reads them)
    table = np.empty(len(gates), dtype=object)
    table[:] = gates
    return ff.concatenate(list(table[sequence]) + ([gates[closer]] if closer is not None else []), omega=omega)


def _single(mode, pulse, spectrum, omega, n_oper_identifiers):
    from . import numeric
    if mode == 'infidelities':
        import filter_functions_amd as ff
        return ff.infidelity(pulse, spectrum, omega, n_oper_identifiers)
    gamma = numeric.calculate_decay_amplitudes(pulse, spectrum, omega, n_oper_identifiers)
    return np.diagonal(gamma, axis1=-2, axis2=-1) if mode == 'diagonal' else gamma


def _pulses(gates, sequence, closers, omega):
    """The loop's pulses of every truncation of one sequence."""
    return [_concatenated(gates, sequence[:m], None if closers is None else closers[m - 1], omega)
            for m in range(1, len(sequence) + 1)]


def _loop(mode, gates, indices, close, spectra, omega, n_oper_identifiers, want_U):
    """The loop's expression for every truncation of every sequence under every spectrum: (a list of P arrays (K, G_p,
    ...), the propagators (G_p, d, d) or None)."""
    values, total = [], []
    for p, sequence in enumerate(indices):
        pulses = _pulses(gates, sequence, None if close is None else close[p], omega)
        values.append(np.stack([np.stack([_single(mode, pulse, S, omega, n_oper_identifiers) for pulse in pulses])
                                for S in spectra]))
        if want_U:
            total.append(np.stack([np.array(pulse.total_propagator) for pulse in pulses]))
    return values, total if want_U else None


def _results(mode, gates, sequences, spectrum, omega, n_oper_identifiers, closing, stacked, return_propagators):
    gates, indices = validated(gates, sequences)
    close = _closing_arrays(closing, indices, len(gates))
    spectra = stacked_spectra(spectrum, stacked)
    want_U = bool(return_propagators)

    def answer(values, total):
        values = values if stacked else [v[0] for v in values]
        return (values, total) if want_U else values
    # routing, once per call: the gate set, then the spectra
    plan = batched_plan(gates, omega) if all(S.ndim in (1, 2) for S in spectra) and len(omega) >= 2 else None
    S = None
    if plan is not None:
        omega = as_f64(omega)
        idx = np.asarray(util.get_indices_from_identifiers(gates[0].n_oper_identifiers, n_oper_identifiers))
        if len(idx) and len(set(idx.tolist())) == len(idx):
            S = _real_weights([util.parse_spectrum(one, omega, idx) for one in spectra])
    if S is None:
        return answer(*_loop(mode, gates, indices, close, spectra, omega, n_oper_identifiers, want_U))
    d, A, W, K, n_idx = plan['d'], plan['A'], len(omega), len(S), len(idx)
    budget = PASS_BYTES - table_bytes(len(gates), d, A, W, n_idx, K, S.ndim - 1)
    values = []
    for chunk in split_sequences([len(i) for i in indices], pass_bytes(d, A, W, n_idx, K, mode, close is not None),
                                 sequence_bytes(d), budget):
        members = [indices[i] for i in chunk]
        got = _run_pass(gates, members, None if close is None else [close[i] for i in chunk], plan, omega, S, idx,
                        mode)
        ends = np.cumsum([len(i) for i in members])
        curves = [got[:, end - len(i):end] for i, end in zip(members, ends)]
        # (the decay amplitudes stay views of the pass's result -- a second copy of it costs a quarter of the call --;
        # the small results are arrays of their own, so that keeping one curve does not keep a pass alive)
        values.extend(curves if mode == 'decay_amplitudes' else [curve.copy() for curve in curves])
    # the sequences whose curve is not finite under a spectrum: what the loop does
    for p, curve in enumerate(values):
        bad = ~np.isfinite(curve.reshape(K, -1)).all(axis=1)
        if bad.any():
            pulses = _pulses(gates, indices[p], None if close is None else close[p], omega)
            for k in np.flatnonzero(bad):
                curve[k] = np.stack([_single(mode, pulse, spectra[k], omega, n_oper_identifiers) for pulse in pulses])
    total = None
    if want_U:
        total = _products(np.array([np.asarray(g.total_propagator) for g in gates], dtype=np.complex128), indices,
                          close)
    return answer(values, total)


_SHARED = r"""

    *gates* is a sequence of T ``PulseSequence`` objects, *sequences* a list of P one-dimensional integer arrays of
    indices into it, read as :func:`ff.sequence_infidelities <filter_functions_amd.sequence_infidelities.
    sequence_infidelities>` reads them (negative indices wrap, others out of range raise IndexError, an empty sequence
    ValueError, an index that is no integer TypeError).  *closing* is None or P integer arrays read by the same rules,
    array p as long as sequence p (else ValueError): ``pulse_m`` is then

    ``ff.concatenate(list(table[s[:m]]) + [gates[closing[p][m - 1]]], omega=omega)``

    with ``table = np.asarray(gates, dtype=object)`` -- the truncation closed by a gate of its own, as randomized
    benchmarking closes every truncation by its inverse (:func:`sequence_prefix_propagators` gives the propagators to
    pick it from).  Values and exceptions are the loop's.  With *stacked* the spectrum carries a leading axis of K
    spectra -- (K, n_omega), (K, n_idx, n_omega) or (K, n_idx, n_idx, n_omega); K = 0 raises ValueError -- and every
    returned array a leading axis K.  With *return_propagators* a list of (G_p, d, d) arrays is returned as well: the
    total propagator of every ``pulse_m``, closing gate included.

    Routing, once per call.  The batched route is taken by the gate sets :func:`ff.sequence_infidelities` takes (all
    gates d = 2 or all d = 4, one Hermitian traceless basis of d^2 elements, the same one to four noise operators,
    total propagators known) under spectra of one or two dimensions without imaginary part, on at least two
    frequencies, with at least one operator selected and none selected twice.  Gates without a control matrix on the
    grid are completed first by one ``ff.get_filter_functions`` call; otherwise no ``PulseSequence`` is created and no
    gate's cache is touched; resident gates are read in place.  A pass is one H2D copy, four launches whatever P, the
    lengths and K, and one D2H copy: every sequence is walked once, forward, and every position adds one epilogue on
    the partial sum of the concatenation rule that the walk holds in registers -- G positions per sequence, not
    G (G + 1) / 2.  A position's result is the same bits alone or among others, in any pass split, stacked or one
    spectrum at a time, and whatever lies behind it: ``curve(s)[:m]`` equals ``curve(s[:m])`` bit for bit.  Everything
    else -- cross-spectra, other dimensions, ineligible gate sets -- and every sequence whose curve is not finite
    evaluates the loop's expression inside the call.  Pulse correlations are not offered."""


def sequence_prefix_infidelities(gates, sequences, spectrum, omega, n_oper_identifiers=None, closing=None,
                                 stacked=False, return_propagators=False):
    r"""Infidelities along many sequences of gates drawn from one gate set: a list of P arrays, entry p of shape
    (G_p, n_idx), or (G_p, n_idx, n_idx) for a cross-spectrum, whose row m - 1 is

    ``ff.infidelity(pulse_m, spectrum, omega, n_oper_identifiers)``

    with ``pulse_m = ff.concatenate(np.asarray(gates, dtype=object)[s[:m]], omega=omega)``, the first m gates of
    sequence p."""
    return _results('infidelities', gates, sequences, spectrum, omega, n_oper_identifiers, closing, stacked,
                    return_propagators)


def sequence_prefix_decay_amplitudes(gates, sequences, spectrum, omega, n_oper_identifiers=None, closing=None,
                                     diagonal=False, stacked=False, return_propagators=False):
    r"""Decay amplitudes :math:`\Gamma_{\alpha\beta,kl}` along many sequences of gates drawn from one gate set: a list
    of P arrays, entry p of shape (G_p, n_idx, N, N), or (G_p, n_idx, n_idx, N, N) for a cross-spectrum, whose row
    m - 1 is

    ``numeric.calculate_decay_amplitudes(pulse_m, spectrum, omega, n_oper_identifiers)``

    with ``pulse_m = ff.concatenate(np.asarray(gates, dtype=object)[s[:m]], omega=omega)``, the first m gates of
    sequence p.  With *diagonal* only ``np.diagonal(..., axis1=-2, axis2=-1)`` of it is formed and returned, shape
    (G_p, n_idx[, n_idx], N): what a state infidelity needs.

    **Memory.**  On the batched route the full decay amplitudes (``diagonal=False``) of the sequences of one pass are
    VIEWS of that pass's one result array (hundreds of MB on a study's shape): a curve that is kept keeps the whole
    array alive.  Copy (``curve.copy()``) what is to outlive the rest.  Infidelities and diagonals are arrays of
    their own."""
    return _results('diagonal' if diagonal else 'decay_amplitudes', gates, sequences, spectrum, omega,
                    n_oper_identifiers, closing, stacked, return_propagators)


for _function in (sequence_prefix_infidelities, sequence_prefix_decay_amplitudes):
    _function.__doc__ += _SHARED
del _function

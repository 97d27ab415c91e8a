"""Frequency shifts and cumulant functions along many gate sequences given as index arrays into one gate set: the
second-order result after 1, 2, ..., G gates of every sequence, optionally with a closing gate behind each truncation
(``ffk_sequence_prefix_frequency_shifts``, include/ffk.h).

``ff.sequence_prefix_frequency_shifts(gates, sequences, spectrum, omega)[p][m - 1]`` is
``numeric.calculate_frequency_shifts`` of ``ff.concatenate(gates[s_p[:m]], calc_second_order_FF=True, omega=omega)``:
the coherent half of the error along a randomized-benchmarking or dynamical-decoupling sequence, next to the decay of
:mod:`~filter_functions_amd.sequence_prefixes`.  The forward walk of :mod:`~filter_functions_amd.sequence_second_order`
holds the frequency shift of the first m gates in its accumulators after position m, and a closing gate adds one more
summand of the same form from the state the walk holds: the batched route walks every sequence once and adds one
epilogue per position, G positions per sequence instead of the G (G + 1) / 2 of the truncations taken as sequences.
``ff.sequence_prefix_cumulant_functions`` composes the decay amplitudes along the sequences, these frequency shifts
and the two batched cumulant entries on the host.
"""
import numpy as np

from . import _lib, util
from ._gate_table import PassTable, batched_plan, validated
from ._lib import as_c128, as_f64, check
from .batch import PASS_BYTES
from .sequence_prefixes import (_closing_arrays, _products, sequence_prefix_decay_amplitudes, split_sequences)
from .sequence_processes import MAX_CUMULANTS, _real_weights, stacked_spectra

__all__ = ['sequence_prefix_frequency_shifts', 'sequence_prefix_cumulant_functions',
           'sequence_prefix_error_transfer_matrices']


def block_width(d, A):
    """Frequencies of one block of the walk (``sequence_prefix_second_order_block_width``): a function of d and A
    alone."""
    return 64 if d == 2 or A <= 2 else 32


def spectra_per_walk(d, A, closing):
    """Spectra that share one walk of the sequences (``sequence_prefix_second_order_spectra_per_walk``); further ones
    repeat it inside the same launch.  A function of d, A and whether closing gates are given alone: what the
    registers of the walk hold without spills."""
    return 1 if A >= 4 or (d == 4 and closing and A >= 3) else 2


def pass_bytes(d, A, W, n_idx, n_spectra, closing):
    """Device bytes one POSITION adds to a pass: its index (and closing index), its tiles of the result and of the
    frequency blocks' partial tiles."""
    N = d*d
    blocks = -(-W//block_width(d, A))
    return 4 + (4 if closing else 0) + 8*n_spectra*n_idx*N*N*(1 + blocks)


def sequence_bytes(d):
    """Device bytes one sequence adds to a pass whatever its length: its offset, its place in the dealing order and
    its total propagator."""
    return 8 + 16*d*d


def table_bytes(n_gates, d, A, W, n_idx, n_spectra, s_ndim):
    """Device bytes of what a pass holds once whatever its sequences: the gate table, the gates' phases, propagators,
    Liouville representations and frequency shifts, the spectra and their weights, the basis."""
    N, dd = d*d, d*d
    rows = n_spectra*(1 if s_ndim == 1 else n_idx)
    return (n_gates*(16*A*N*W + 16*W + 8*N*N + 16*dd + 16 + 8*N*N*n_spectra*n_idx) + 16*N*dd + 8*W + 32*rows*W
            + 4*n_idx + 4 + 20*256)


def staged(d, n_gates, A, closing):
    """Whether a pass over *n_gates* gates keeps their tables in LDS (``sequence_prefix_second_order_staged``): the
    control matrices and phases of one block's frequencies, at d = 4 with the block's weights in front, in at most
    150 KiB.  Else the walk reads them from L2.  The arithmetic is the same either way."""
    width = block_width(d, A)
    weights = 0 if d == 2 else 8*spectra_per_walk(d, A, closing)*A*width
    return 16*n_gates*(A*d*d + 1)*width + weights <= 150*1024


def _run_pass(gates, indices, close, plan, omega, S, idx, shifts):
    """One call of ``ffk_sequence_prefix_frequency_shifts`` over the sequences *indices* (int32 arrays into *gates*),
    their closing gates *close* (the same, or None), the spectra S (K, W) or (K, n_idx, W) and the gates' own
    frequency shifts (K, T, n_idx, N, N): the tiles of every global position, (K, n_index, n_idx, N, N)."""
    N, K = plan['N'], len(S)
    table = PassTable(gates, indices, plan, omega, extra=close)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    n_idx = len(idx)
    n_index = int(table.offsets[-1])
    own = as_f64(np.ascontiguousarray(np.asarray(shifts)[:, table.used]))
    out = np.empty((K, n_index, n_idx, N, N), dtype=np.float64)
    check(_lib.load().ffk_sequence_prefix_frequency_shifts(
        *table.c_arguments(), None if table.extra is None else table.extra.ctypes.data, S.ctypes.data, S.ndim - 1, K,
        idx.ctypes.data, n_idx, own.ctypes.data, out.ctypes.data))
    return out


def _concatenated(gates, sequence, closer, omega):
    """The loop's pulse of one truncation (*closer*: the gate appended behind it, or None)."""
    import filter_functions_amd as ff         # (the public names, as a caller's loop reads them)
    table = np.empty(len(gates), dtype=object)
    table[:] = gates
    return ff.concatenate(list(table[sequence]) + ([gates[closer]] if closer is not None else []),
                          calc_second_order_FF=True, omega=omega)


def _pulses(gates, sequence, closers, omega):
    """The loop's pulses of every truncation of one sequence."""
    return [_concatenated(gates, sequence[:m], None if closers is None else closers[m - 1], omega)
            for m in range(1, len(sequence) + 1)]


def _single(pulse, spectrum, omega, n_oper_identifiers):
    from . import numeric
    return numeric.calculate_frequency_shifts(pulse, spectrum, omega, n_oper_identifiers)


def _single_cumulant(pulse, spectrum, omega, n_oper_identifiers, second_order):
    from . import numeric
    return numeric.calculate_cumulant_function(pulse, spectrum, omega, n_oper_identifiers, second_order=second_order)


def _loop(gates, indices, close, spectra, omega, n_oper_identifiers, want_U, single=_single):
    """The loop's expression for every truncation of every sequence under every spectrum: (a list of P arrays (K, G_p,
    ...), the propagators (G_p, d, d) or None)."""
    values, total = [], []
    for p, sequence in enumerate(indices):
        pulses = _pulses(gates, sequence, None if close is None else close[p], omega)
        values.append(np.stack([np.stack([single(pulse, S, omega, n_oper_identifiers) for pulse in pulses])
                                for S in spectra]))
        if want_U:
            total.append(np.stack([np.array(pulse.total_propagator) for pulse in pulses]))
    return values, total if want_U else None


def _gate_shifts(gates, spectrum, omega, n_oper_identifiers):
    """The gates' own frequency shifts under one spectrum, (T, n_idx, N, N)."""
    from .batch_second_order import frequency_shifts
    return frequency_shifts(gates, spectrum, omega, n_oper_identifiers)


_SHARED = r"""

    *gates* is a sequence of T ``PulseSequence`` objects, *sequences* a list of P one-dimensional integer arrays of
    indices into it and *closing* None or P integer arrays, array p as long as sequence p (else ValueError), all read
    as :func:`ff.sequence_prefix_infidelities <filter_functions_amd.sequence_prefixes.sequence_prefix_infidelities>`
    reads them (negative indices wrap, others out of range raise IndexError, an empty sequence ValueError, an index
    that is no integer TypeError): ``pulse_m`` is

    ``ff.concatenate(list(table[s[:m]]) + [gates[closing[p][m - 1]]], calc_second_order_FF=True, omega=omega)``

    with ``table = np.asarray(gates, dtype=object)``, without the appended gate when *closing* is None
    (:func:`ff.sequence_prefix_propagators` gives the propagators to pick an inverting gate from).  Values and
    exceptions are the loop's.  With *stacked* the spectrum carries a leading axis of K spectra -- (K, n_omega),
    (K, n_idx, n_omega) or (K, n_idx, n_idx, n_omega); K = 0 raises ValueError -- and every returned array a leading
    axis K.  With *return_propagators* a list of (G_p, d, d) arrays is returned as well: the total propagator of every
    ``pulse_m``, closing gate included."""


def sequence_prefix_frequency_shifts(gates, sequences, spectrum, omega, n_oper_identifiers=None, closing=None,
                                     stacked=False, return_propagators=False):
    r"""Frequency shifts :math:`\Delta_{\alpha\beta,kl}` along many sequences of gates drawn from one gate set: a list
    of P arrays, entry p of shape (G_p, n_idx, N, N), or (G_p, n_idx, n_idx, N, N) for a cross-spectrum, whose row
    m - 1 is

    ``numeric.calculate_frequency_shifts(pulse_m, spectrum, omega, n_oper_identifiers)``

    with ``pulse_m`` the first m gates of sequence p, concatenated with their second-order filter function.
    SHARED

    Routing, once per call.  The batched route is taken by the gate sets :func:`ff.sequence_infidelities` takes (all
    gates d = 2 or all d = 4, one Hermitian traceless basis of d^2 elements, the same one to four noise operators,
    total propagators known) under spectra of one or two dimensions without imaginary part, on at least two
    frequencies, with at least one operator selected and none selected twice.  Gates without a control matrix on the
    grid are completed first by one ``ff.get_filter_functions`` call.  The gates' own frequency shifts come from
    ``ff.frequency_shifts(gates, spectrum[k], omega, n_oper_identifiers)``, one call per spectrum, whose routing and
    cache behaviour apply: batched members of that call end WITHOUT ``filter_function_2`` cached (their eigensystems
    are cached and ``gate.omega`` is set), where the loop would leave every gate with it.  No ``PulseSequence`` is
    created for a truncation and resident gates are read in place.  A pass is one H2D copy, four launches whatever P,
    the lengths and K, and one D2H copy: every sequence is walked once, forward, and every position adds one epilogue
    on copies of the running sums the walk holds in registers -- G positions per sequence, not G (G + 1) / 2; neither
    a second-order filter function nor a control matrix is written to memory.  One or two spectra share a walk (a
    function of d, the number of noise operators and whether *closing* is given), further ones repeat it inside the
    same launch.  A position's result is the same bits alone or among others, in any pass split, stacked or one
    spectrum at a time, and whatever lies behind it: ``curve(s, closing)[:m]`` equals ``curve(s[:m], closing[:m])``
    bit for bit, and without *closing* row 0 is the first gate's row of ``ff.frequency_shifts``.  Everything else --
    cross-spectra, other dimensions, ineligible gate sets -- and every (spectrum, sequence) whose curve is not finite
    evaluates the loop's expression inside the call.  Pulse correlations are not offered."""
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
        return answer(*_loop(gates, indices, close, spectra, omega, n_oper_identifiers, want_U))
    d, A, W, K, n_idx = plan['d'], plan['A'], len(omega), len(S), len(idx)
    shifts = np.stack([_gate_shifts(gates, one, omega, n_oper_identifiers) for one in spectra])
    budget = PASS_BYTES - table_bytes(len(gates), d, A, W, n_idx, K, S.ndim - 1)
    values = []
    for chunk in split_sequences([len(i) for i in indices], pass_bytes(d, A, W, n_idx, K, close is not None),
                                 sequence_bytes(d), budget):
        members = [indices[i] for i in chunk]
        got = _run_pass(gates, members, None if close is None else [close[i] for i in chunk], plan, omega, S, idx,
                        shifts)
        ends = np.cumsum([len(i) for i in members])
        # (views of the pass's result, as the decay amplitudes of sequence_prefixes: a second copy of it costs a
        # quarter of the call)
        values.extend(got[:, end - len(i):end] for i, end in zip(members, ends))
    # the (spectrum, sequence) whose curve is not finite: what the loop does
    for p, curve in enumerate(values):
        bad = ~np.isfinite(curve.reshape(K, -1)).all(axis=1)
        if bad.any():
            pulses = _pulses(gates, indices[p], None if close is None else close[p], omega)
            for k in np.flatnonzero(bad):
                curve[k] = np.stack([_single(pulse, spectra[k], omega, n_oper_identifiers) for pulse in pulses])
    total = None
    if want_U:
        total = _products(np.array([np.asarray(g.total_propagator) for g in gates], dtype=np.complex128), indices,
                          close)
    return answer(values, total)


def _cumulants(gamma, delta, basis):
    """The cumulant functions of the tiles *gamma* (n, N, N), with the second-order term of the frequency shifts
    *delta* (n, N, N) or None: ``ffk_cumulant_function`` and ``ffk_cumulant_function_second_order`` in chunks of what
    one launch takes."""
    from . import numeric
    N, d = np.shape(basis)[:2]
    numeric._check_d(d)
    single_qubit = int(d == 2 and getattr(basis, 'btype', None) in ('Pauli', 'GGM'))
    C = as_c128(np.asarray(basis))
    out = np.empty((len(gamma), N, N), dtype=np.float64)
    lib = _lib.load()
    for lo in range(0, len(gamma), MAX_CUMULANTS):
        part = np.ascontiguousarray(gamma[lo:lo + MAX_CUMULANTS], dtype=np.float64)
        res = np.empty_like(part)
        check(lib.ffk_cumulant_function(part.ctypes.data, len(part), N, d, C.ctypes.data, single_qubit,
                                        res.ctypes.data))
        if delta is not None:
            shifts = np.ascontiguousarray(delta[lo:lo + MAX_CUMULANTS], dtype=np.float64)
            check(lib.ffk_cumulant_function_second_order(shifts.ctypes.data, len(shifts), N, d, C.ctypes.data,
                                                         res.ctypes.data))
        out[lo:lo + MAX_CUMULANTS] = res
    return out


def sequence_prefix_cumulant_functions(gates, sequences, spectrum, omega, n_oper_identifiers=None, closing=None,
                                       second_order=False, stacked=False, return_propagators=False):
    r"""Cumulant functions :math:`\mathcal{K}_{\alpha\beta}` along many sequences of gates drawn from one gate set: a
    list of P arrays, entry p of shape (G_p, n_idx, N, N), or (G_p, n_idx, n_idx, N, N) for a cross-spectrum, whose
    row m - 1 is

    ``numeric.calculate_cumulant_function(pulse_m, spectrum, omega, n_oper_identifiers, second_order=second_order)``

    with ``pulse_m`` the first m gates of sequence p (concatenated with ``calc_second_order_FF=True`` when
    *second_order* is set).
    SHARED

    A composition on the host: the decay amplitudes come from :func:`ff.sequence_prefix_decay_amplitudes
    <filter_functions_amd.sequence_prefixes.sequence_prefix_decay_amplitudes>` and, with *second_order*, the frequency
    shifts from :func:`sequence_prefix_frequency_shifts` -- the routing, cache behaviour and same-bits properties of
    both apply --, and every tile goes through ``ffk_cumulant_function`` (and ``ffk_cumulant_function_second_order``)
    in chunks of what one launch takes, without a loop over the positions.  ``second_order=False`` runs no
    second-order code and gives the bits of the call without the keyword.  Gates of several bases evaluate the loop's
    expression.  :func:`sequence_prefix_error_transfer_matrices` exponentiates the result of this call, every position
    in one launch."""
    from .batch_second_order import _same_basis
    gates, sequences = list(gates), list(sequences)
    closing = None if closing is None else list(closing)
    want_U = bool(return_propagators)
    checked, indices = validated(gates, sequences)
    if not all(_same_basis(checked[0].basis, g.basis) for g in checked[1:]):
        # (gates of several bases: no single basis to contract with -- the loop's expression)
        def single(pulse, S, omega, identifiers):
            return _single_cumulant(pulse, S, omega, identifiers, bool(second_order))
        values, total = _loop(checked, indices, _closing_arrays(closing, indices, len(checked)),
                              stacked_spectra(spectrum, stacked), omega, n_oper_identifiers, want_U, single)
        values = values if stacked else [v[0] for v in values]
        return (values, total) if want_U else values
    first = sequence_prefix_decay_amplitudes(gates, sequences, spectrum, omega, n_oper_identifiers, closing=closing,
                                             stacked=stacked, return_propagators=want_U)
    gamma, total = first if want_U else (first, None)
    delta = None
    if second_order:
        delta = sequence_prefix_frequency_shifts(gates, sequences, spectrum, omega, n_oper_identifiers,
                                                 closing=closing, stacked=stacked)
        if [np.shape(one) for one in delta] != [np.shape(one) for one in gamma]:
            raise ValueError('Frequency shifts not same shape as decay amplitudes')
    basis = checked[0].basis
    N = np.shape(basis)[0]
    tiles = np.concatenate([as_f64(one).reshape(-1, N, N) for one in gamma])
    shifts = None if delta is None else np.concatenate([as_f64(one).reshape(-1, N, N) for one in delta])
    flat = _cumulants(tiles, shifts, basis)
    ends = np.cumsum([np.size(one)//(N*N) for one in gamma])
    values = [flat[end - np.size(one)//(N*N):end].reshape(np.shape(one)) for one, end in zip(gamma, ends)]
    return (values, total) if want_U else values


def sequence_prefix_error_transfer_matrices(gates, sequences, spectrum, omega, n_oper_identifiers=None, closing=None,
                                            second_order=False, stacked=False, return_propagators=False):
    r"""Error transfer matrices :math:`\langle\tilde{\mathcal{U}}\rangle = \exp\mathcal{K}` along many sequences of
    gates drawn from one gate set: a list of P arrays, entry p of shape (G_p, N, N), whose row m - 1 is

    ``ff.error_transfer_matrix(pulse_m, spectrum, omega, n_oper_identifiers, second_order=second_order)``

    with ``pulse_m`` the first m gates of sequence p (concatenated with ``calc_second_order_FF=True`` when
    *second_order* is set): what tells depolarising from dephasing and a rotation from a contraction after every gate.
    SHARED

    A composition on the host: the cumulant functions come from :func:`sequence_prefix_cumulant_functions`, called
    with the same arguments -- its routing, fallbacks, cache behaviour and same-bits properties all apply --, the
    tiles of every position of every sequence under every spectrum are concatenated into one array, and that array
    goes through :func:`ff.exponentiate_cumulant_functions
    <filter_functions_amd.expm_batch.exponentiate_cumulant_functions>` once: the sum over the noise operators (over
    both operator axes of a cross-spectrum, as the single function sums), the norm, the choice of the squarings and
    the exponential of every position run in one launch per chunk, without a loop over the positions.  The values
    agree with the loop's to rounding (the sums inside the matrix products are ordered differently from the single
    function's); a position's matrix is the same bits alone or among others, stacked or one spectrum at a time, and
    ``curve(s, closing)[:m]`` equals ``curve(s[:m], closing[:m])`` bit for bit.  Positions whose summed cumulant
    function is not finite, complex cumulant functions and N > 16 evaluate the single function per position."""
    from .expm_batch import exponentiate_cumulant_functions
    want_U = bool(return_propagators)
    first = sequence_prefix_cumulant_functions(gates, sequences, spectrum, omega, n_oper_identifiers,
                                               closing=closing, second_order=second_order, stacked=stacked,
                                               return_propagators=want_U)
    cumulants, total = first if want_U else (first, None)
    N = np.shape(cumulants[0])[-1]
    lead = 2 if stacked else 1            # ([K,] G_p, operators ..., N, N): one matrix per leading index
    heads = [np.shape(one)[:lead] for one in cumulants]
    tiles = np.concatenate([np.reshape(one, (int(np.prod(head)), -1, N, N)) for one, head in zip(cumulants, heads)])
    flat = exponentiate_cumulant_functions(tiles)
    ends = np.cumsum([int(np.prod(head)) for head in heads])
    values = [flat[end - int(np.prod(head)):end].reshape(tuple(head) + (N, N)) for head, end in zip(heads, ends)]
    return (values, total) if want_U else values


for _function in (sequence_prefix_frequency_shifts, sequence_prefix_cumulant_functions,
                  sequence_prefix_error_transfer_matrices):
    _function.__doc__ = _function.__doc__.replace('\n    SHARED\n', _SHARED + '\n')
del _function

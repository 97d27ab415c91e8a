"""Periodic driving, second order: the frequency shifts of many pulses at many repeat counts in one pass, by period
doubling (``ffk_resident_periodic_shifts``, include/ffk.h).

``ff.periodic_frequency_shifts(pulses, repeats, S, omega)`` is ``np.stack`` over the pulses and the repeat counts of
``numeric.calculate_frequency_shifts(ff.concatenate([p]*n, calc_second_order_FF=True, omega=omega), S, omega)``: the
coherent half of the error of a drive against the number of periods, next to the decay of
:mod:`~filter_functions_amd.periodic`.  The concatenation rule of the second-order filter function, integrated and
applied to an atom of m periods followed by one of m' periods of the same pulse, reads

    Delta_{m+m'} = Delta_m + Q_m^T Delta_{m'} Q_m + X(m, m'),

with Q_m the Liouville matrix of U^m and X a Gram matrix over the frequencies of two operands that are element-wise
in the propagator's eigenbasis (the control matrix of m periods, and that of m' periods carried behind them).  A
count n is reached in at most 2 log2 n such steps (:func:`step_plan`), so that the cost grows with log n and no
second-order filter function is ever formed.  ``ff.periodic_cumulant_functions`` and
``ff.periodic_error_transfer_matrices`` compose the decay amplitudes of :mod:`~filter_functions_amd.periodic`, these
frequency shifts, the two batched cumulant entries and the batched exponential on the host.
"""
import ctypes

import numpy as np

from . import _lib, batch, numeric, periodic, processes, util
from ._lib import as_c128, as_f64, check

__all__ = ['periodic_frequency_shifts', 'periodic_cumulant_functions', 'periodic_error_transfer_matrices']

#: Steps of one pass at most (a grid axis).
MAX_STEPS = 65535
#: Repeat counts of one pass at most: their plan has at most 30 + 30 MAX_COUNTS <= MAX_STEPS steps.
MAX_COUNTS = 2000


def step_plan(repeats):
    """The steps that reach every count of *repeats* (integers 1 .. 2^31 - 1) by period doubling:
    ``(steps, count_slots)`` with *steps* (S, 4) int32, row s = (m, m', slot of Delta_m, slot of Delta_m'), whose
    result Delta_{m + m'} lies in slot s + 1 -- slot 0 is Delta_1 --, and *count_slots* (K,) int32 the slot each
    count reads.  The steps of a count n are a function of n alone: the doubling chain (1, 1), (2, 2), ... up to the
    top bit of n, then the lower set bits added from the top down, (cur, 2^j) with cur += 2^j; n = 7 gives (1, 1),
    (2, 2), (4, 2), (6, 1), and n = 1 needs no step.  The plan is the union over the counts in their order, every
    (m, m') once: the chain is shared, and so is every common run of leading bits."""
    counts = [int(n) for n in np.asarray(repeats).reshape(-1)]
    slot = {1: 0}
    steps = []

    def reach(m, mp):
        if m + mp not in slot:
            steps.append((m, mp, slot[m], slot[mp]))
            slot[m + mp] = len(steps)

    for n in counts:
        if not 1 <= n <= np.iinfo(np.int32).max:
            raise ValueError(f'a repeat count must lie in [1, 2^31 - 1], not be {n}.')
        top = n.bit_length() - 1
        for j in range(top):
            reach(1 << j, 1 << j)
        cur = 1 << top
        for j in range(top - 1, -1, -1):
            if n >> j & 1:
                reach(cur, 1 << j)
                cur += 1 << j
    return (np.array(steps, dtype=np.int32).reshape(-1, 4),
            np.array([slot[n] for n in counts], dtype=np.int32))


def _up(nbytes):
    return -(-nbytes//256)*256


def fixed_bytes(K, S, A, N, W, d, n_idx, s_ndim):
    """Device bytes of a pass that do not grow with its members (``ffk_periodic_shifts_workspace_bytes`` without
    them)."""
    rows = 1 if s_ndim == 1 else n_idx
    return _up(8*W) + _up(16*N*d*d) + _up(16*S) + _up(4*K) + _up(4*n_idx) + 2*_up(16*rows*W) + 9*256


def member_bytes(K, S, A, N, W, d, n_idx, host):
    """Device bytes one member adds to a pass at most: pointer, eigensystem, period, its own frequency shifts, the
    steps' tiles, the result table, the result and -- for a control matrix held as a host array (*host*) -- its row
    of the uploaded table."""
    return 8 + 16*d*d + 16*d*d + 8 + 8*n_idx*N*N*(1 + S + (S + 1) + K) + (16*A*N*W if host else 0)


def split_group(group, is_host, K, S, A, N, W, d, n_idx, s_ndim, budget=None):
    """*group* in consecutive passes under ``batch.PASS_BYTES``, every member counted as the largest of the group."""
    budget = batch.PASS_BYTES if budget is None else budget
    per_member = member_bytes(K, S, A, N, W, d, n_idx, any(is_host))
    room = max(per_member, budget - fixed_bytes(K, S, A, N, W, d, n_idx, s_ndim))
    return batch.split_passes(group, per_member, room, periodic.MAX_MEMBERS)


def _run_pass(pulses, members, sources, systems, omega, steps, count_slots, spectrum, idx, delta1):
    """One call of ``ffk_resident_periodic_shifts`` over ``pulses[i] for i in members`` with their own frequency
    shifts *delta1* (P, n_idx, N, N): the result (P, K, n_idx, N, N)."""
    first = pulses[members[0]]
    N, A, d = processes.shape_of(first)
    P, W, K, S = len(members), len(omega), len(count_slots), len(steps)
    handles = (ctypes.c_void_p*P)(*(None if sources[i][0] == 'host' else sources[i][1].value for i in members))
    slots = np.array([-1 if sources[i][0] == 'host' else sources[i][2] for i in members], dtype=np.int32)
    host = [sources[i][1] for i in members if sources[i][0] == 'host']
    table = as_c128(np.stack(host)) if host else None
    omega = as_f64(omega)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    B = as_c128(np.asarray(first.basis))
    V = as_c128(np.stack([systems[i][0] for i in members]))
    phi = as_f64(np.stack([systems[i][1] for i in members]))
    T = as_f64(np.array([pulses[i].tau for i in members], dtype=np.float64))
    steps = np.ascontiguousarray(steps, dtype=np.int32)
    count_slots = np.ascontiguousarray(count_slots, dtype=np.int32)
    spectrum = as_c128(spectrum)
    delta1 = as_f64(np.ascontiguousarray(delta1))
    n_idx = len(idx)
    out = np.empty((P, K, n_idx, N, N), dtype=np.float64)
    check(_lib.load().ffk_resident_periodic_shifts(
        handles, slots.ctypes.data, None if table is None else table.ctypes.data, P, A, W, d, omega.ctypes.data,
        B.ctypes.data, V.ctypes.data, phi.ctypes.data, T.ctypes.data, steps.ctypes.data if S else None, S,
        count_slots.ctypes.data, K, spectrum.ctypes.data, spectrum.ndim, idx.ctypes.data, n_idx, delta1.ctypes.data,
        out.ctypes.data))
    return out


def _repeated(pulse, repeats, omega):
    """{n: n periods of *pulse* with their second-order filter function} for the counts of *repeats*, by binary
    doubling of ``ff.concatenate(..., calc_second_order_FF=True)``: O(log n) concatenations per count, the powers of
    two shared."""
    from .pulse_sequence import concatenate
    power = {0: pulse}
    made = {}
    for n in sorted({int(n) for n in repeats}):
        top = n.bit_length() - 1
        for j in range(1, top + 1):
            if j not in power:
                power[j] = concatenate([power[j - 1]]*2, calc_second_order_FF=True, omega=omega)
        parts = [power[j] for j in range(top, -1, -1) if n >> j & 1]
        made[n] = parts[0] if len(parts) == 1 else concatenate(parts, calc_second_order_FF=True, omega=omega)
    return made


def _fallback(pulse, repeats, spectrum, omega, n_oper_identifiers):
    """The loop's values for one pulse, (K, ...)."""
    made = _repeated(pulse, repeats if len(repeats) else [1], omega)
    rows = [numeric.calculate_frequency_shifts(made[int(n)], spectrum, omega, n_oper_identifiers) for n in repeats]
    if not rows:
        one = numeric.calculate_frequency_shifts(made[1], spectrum, omega, n_oper_identifiers)
        return np.empty((0,) + np.shape(one), dtype=np.float64)
    return np.stack(rows)


def periodic_frequency_shifts(pulses, repeats, spectrum, omega, n_oper_identifiers=None):
    r"""Frequency shifts :math:`\Delta_{\alpha\alpha,kl}` of *repeats[k]* periods of every pulse, shape (n_pulses,
    n_repeats, n_idx, N, N), or (n_pulses, n_repeats, n_idx, n_idx, N, N) for a cross-spectrum:

    ``numeric.calculate_frequency_shifts(ff.concatenate([p]*n, calc_second_order_FF=True, omega=omega), spectrum,
    omega, n_oper_identifiers)``

    stacked over pulses and repeat counts.  Arguments and exceptions as :func:`ff.periodic_decay_amplitudes
    <filter_functions_amd.periodic.periodic_decay_amplitudes>`: *repeats* is a one-dimensional array of integers in
    [1, 2^31 - 1] shared by all pulses.

    Routing, per pulse.  d = 2, 3, 4 with a complete, Hermitian, traceless basis, one to four noise operators and a
    propagator whose eigensystem leaves a residue of at most ``periodic.MAX_RESIDUE`` takes the batched route under a
    real spectrum of one or two dimensions on at least two frequencies.  Pulses whose control matrix is not known on
    the grid are completed first by ONE ``ff.get_filter_functions`` call; resident control matrices are read in place
    and deferred cache entries stay deferred.  The pulses' own frequency shifts :math:`\Delta_1` come from ONE
    ``ff.frequency_shifts(eligible_pulses, spectrum, omega, n_oper_identifiers)`` call, whose routing and cache
    behaviour apply: batched members of that call end WITHOUT ``filter_function_2`` cached (their eigensystems are
    cached and ``pulse.omega`` is set), where the loop would leave it on every pulse.  Groups of one shape, basis and
    selection are split under ``batch.PASS_BYTES``.  A pass is one H2D copy, at most three launches whatever the
    numbers of pulses, counts and steps, and one D2H copy: every count is reached by period doubling
    (:func:`step_plan`), at most 2 log2 n steps of a d^2 x d^2 Gram matrix over the frequencies each (d = 4: on the
    FP64 matrix cores), and no second-order filter function is formed.  A result is the same bits alone or among
    other pulses, at any place in *repeats* and whatever else is in it, in any pass split, resident or uploaded; row
    n = 1 is the pulse's row of ``ff.frequency_shifts`` bit for bit.

    Every other pulse, every pulse whose batched result is not finite, and cross-spectra and complex spectra run the
    fallback inside the call: the n periods are built by binary doubling of ``ff.concatenate(...,
    calc_second_order_FF=True)`` -- O(log n) concatenations -- and go through ``numeric.calculate_frequency_shifts``.
    Its values equal the flat loop's to rounding (the concatenation rule is associative; the sums are ordered
    differently)."""
    from .batch_second_order import frequency_shifts
    from .pulse_sequence import PulseSequence
    pulses = list(pulses)
    for pulse in pulses:
        if not isinstance(pulse, PulseSequence):
            raise TypeError('Can only concatenate PulseSequences!')
    repeats = periodic._checked_repeats(repeats)
    if not pulses:
        return np.empty((0,), dtype=np.float64)
    idx_of = [util.get_indices_from_identifiers(p.n_oper_identifiers, n_oper_identifiers) for p in pulses]
    spectrum = np.asanyarray(spectrum)
    shapes = {(len(idx), len(p.basis)) for idx, p in zip(idx_of, pulses)}
    if len(shapes) > 1:
        raise ValueError('Every pulse must give the same output shape: the pulses have (selected noise operators, '
                         f'basis elements) = {sorted(shapes)}.')
    K, W = len(repeats), len(omega)
    out = [None]*len(pulses)
    # cross-spectra and spectra with an imaginary part: the fallback (which also raises what a bad spectrum raises)
    batched = K > 0 and spectrum.ndim <= 2 and W >= 2 and not (np.iscomplexobj(spectrum) and np.any(spectrum.imag))
    if batched:
        periodic._prepare(pulses, omega)
        sources, systems = {}, {}
        for i, pulse in enumerate(pulses):
            source = processes._source(pulse, omega, W) if periodic._eligible(pulse) else None
            if source is None:
                continue
            V, phi, residue = periodic.eigensystem(pulse.total_propagator)
            if residue <= periodic.MAX_RESIDUE:
                sources[i], systems[i] = source, (V, periodic.phase_differences(pulse.total_propagator, V))
        taken = sorted(sources)
        own = {}
        if taken:
            first_order = frequency_shifts([pulses[i] for i in taken], spectrum, omega, n_oper_identifiers)
            own = {i: first_order[j] for j, i in enumerate(taken)}
        for group in processes.group_members(pulses, taken, idx_of):
            first = pulses[group[0]]
            N, A, d = processes.shape_of(first)
            idx = idx_of[group[0]]
            parsed = util.parse_spectrum(spectrum, as_f64(omega), np.asarray(idx))
            is_host = [sources[i][0] == 'host' for i in group]
            for start in range(0, K, MAX_COUNTS):
                steps, count_slots = step_plan(repeats[start:start + MAX_COUNTS])
                for members in split_group(group, is_host, len(count_slots), len(steps), A, N, W, d, len(idx),
                                           parsed.ndim):
                    delta1 = np.stack([own[i] for i in members])
                    values = _run_pass(pulses, members, sources, systems, omega, steps, count_slots, parsed, idx,
                                       delta1)
                    for j, i in enumerate(members):
                        if out[i] is None:
                            out[i] = np.empty((K,) + values.shape[2:], dtype=np.float64)
                        out[i][start:start + len(count_slots)] = values[j]
        for i in sources:
            if not np.isfinite(out[i]).all():
                out[i] = None
    for i, pulse in enumerate(pulses):
        if out[i] is None:
            out[i] = _fallback(pulse, repeats, spectrum, omega, n_oper_identifiers)
    return np.stack(out)


def periodic_cumulant_functions(pulses, repeats, spectrum, omega, n_oper_identifiers=None, second_order=False):
    r"""Cumulant functions :math:`\mathcal{K}_{\alpha\alpha}` of *repeats[k]* periods of every pulse, shape (n_pulses,
    n_repeats, n_idx, N, N), or (n_pulses, n_repeats, n_idx, n_idx, N, N) for a cross-spectrum:

    ``numeric.calculate_cumulant_function(pulse_n, spectrum, omega, n_oper_identifiers, second_order=second_order)``

    stacked over pulses and repeat counts, with ``pulse_n = ff.concatenate([p]*n, calc_second_order_FF=second_order,
    omega=omega)``.  A composition on the host: the decay amplitudes come from :func:`ff.periodic_decay_amplitudes
    <filter_functions_amd.periodic.periodic_decay_amplitudes>` and, with *second_order*, the frequency shifts from
    :func:`periodic_frequency_shifts` -- the routing, cache behaviour and same-bits properties of both apply --, and
    every tile goes through ``ffk_cumulant_function`` (and ``ffk_cumulant_function_second_order``) in chunks of what
    one launch takes, without a loop over pulses or counts.  ``second_order=False`` runs no second-order code.  The
    pulses must share one basis (else ValueError)."""
    from .batch_second_order import _same_basis
    from .sequence_prefix_second_order import _cumulants
    pulses = list(pulses)
    gamma = periodic.periodic_decay_amplitudes(pulses, repeats, spectrum, omega, n_oper_identifiers)
    if not pulses:
        return gamma
    if not all(_same_basis(pulses[0].basis, p.basis) for p in pulses[1:]):
        raise ValueError('The pulses of one call must share one basis.')
    delta = None
    if second_order:
        delta = periodic_frequency_shifts(pulses, repeats, spectrum, omega, n_oper_identifiers)
        if np.shape(delta) != np.shape(gamma):
            raise ValueError('Frequency shifts not same shape as decay amplitudes')
    basis = pulses[0].basis
    N = np.shape(basis)[0]
    flat = _cumulants(as_f64(gamma).reshape(-1, N, N), None if delta is None else as_f64(delta).reshape(-1, N, N),
                      basis)
    return flat.reshape(np.shape(gamma))


def periodic_error_transfer_matrices(pulses, repeats, spectrum, omega, n_oper_identifiers=None, second_order=False):
    r"""Error transfer matrices :math:`\langle\tilde{\mathcal{U}}\rangle = \exp\mathcal{K}` of *repeats[k]* periods of
    every pulse, shape (n_pulses, n_repeats, N, N):

    ``ff.error_transfer_matrix(pulse_n, spectrum, omega, n_oper_identifiers, second_order=second_order)``

    stacked over pulses and repeat counts, ``pulse_n`` as in :func:`periodic_cumulant_functions`: with
    *second_order* a rotation as well as a contraction.  A composition on the host: the cumulant functions come from
    :func:`periodic_cumulant_functions`, called with the same arguments -- its routing, fallbacks and cache behaviour
    apply --, and all n_pulses x n_repeats matrices go through ONE :func:`ff.exponentiate_cumulant_functions
    <filter_functions_amd.expm_batch.exponentiate_cumulant_functions>` call, which sums over the noise operators and
    chooses the squarings per matrix.  The values agree with the loop's to rounding."""
    from .expm_batch import exponentiate_cumulant_functions
    cumulants = periodic_cumulant_functions(pulses, repeats, spectrum, omega, n_oper_identifiers,
                                            second_order=second_order)
    if cumulants.ndim < 4:
        return cumulants
    P, K, N = cumulants.shape[0], cumulants.shape[1], cumulants.shape[-1]
    if P*K == 0:
        return np.empty((P, K, N, N), dtype=np.float64)
    return exponentiate_cumulant_functions(cumulants.reshape(P*K, -1, N, N)).reshape(P, K, N, N)

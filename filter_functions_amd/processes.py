"""Quantum processes of many pulses in one pass (``ffk_resident_batch_processes``, include/ffk.h).

``ff.decay_amplitudes(pulses, S, omega)``, ``ff.cumulant_functions(pulses, S, omega)`` and
``ff.error_transfer_matrices(pulses, S, omega)`` are ``np.stack`` of the loops over
``numeric.calculate_decay_amplitudes``, ``numeric.calculate_cumulant_function`` and ``ff.error_transfer_matrix``
(``which='total'``; first order, or with ``second_order=True`` the frequency-shift terms of
``ff.frequency_shifts`` added).  A pulse whose control matrix is known on the grid -- resident in HBM behind a
:class:`~filter_functions_amd._resident.Deferred` entry after ``ff.get_filter_functions``,
``ff.concatenate_sequences`` or its own resident pass, or a host array -- is evaluated in batched passes: the
resident control matrices are read where they lie (nothing is fetched, the deferred entries stay deferred), host
arrays are uploaded once per pass, and one launch per stage serves every pulse of the pass.
"""
import ctypes

import numpy as np

from . import _lib, batch, numeric, util
from ._lib import as_c128, as_f64, check
from ._resident import Deferred

__all__ = ['decay_amplitudes', 'cumulant_functions', 'error_transfer_matrices']

#: The batched kernels' shapes: at most this many basis elements (one 16 x 16 tile; d = 2, 3, 4) ...
MAX_BASIS_ELEMENTS = 16
MAX_DIMENSION = 4
#: ... and noise operators in the control matrix.
MAX_NOISE_OPERATORS = 4
#: Members of one pass at most (the pulse is a grid axis; the cumulant functions of a pass share one launch).
MAX_MEMBERS = 65535

_STAGES = ('decay_amplitudes', 'cumulant_function', 'error_transfer_matrix')


def pairs_of(n_idx, s_ndim):
    """Noise-operator rows of one pulse's decay amplitudes: n_idx, or n_idx**2 for cross-spectra."""
    return n_idx*n_idx if s_ndim == 3 else n_idx


def decay_chunks(W):
    """Frequency chunks of the decay-amplitudes launch (``processes_decay_chunks``, processes.hip: about 256
    frequencies each, whole steps of 32, at most 64; a function of W alone)."""
    n = min(64, max(1, -(-W//256)))
    length = -(-(-(-W//n))//32)*32
    return -(-W//length)


def _up(nbytes):
    return -(-nbytes//256)*256


def fixed_bytes(A, N, W, d, n_idx, s_ndim):
    """Device bytes of a pass that do not grow with its members: grid, basis, spectrum and weights, indices, the
    basis lists of the cumulant function (an upper bound of the C layout's share)."""
    rows = 1 if s_ndim == 1 else pairs_of(n_idx, s_ndim)
    dd = d*d
    lists = _up(4) + _up(4*N) + _up(4*N*dd) + _up(16*N*dd) + _up(4*dd) + _up(4*dd*N) + _up(16*dd*N)
    return _up(8*W) + _up(16*N*dd) + 2*_up(16*rows*W) + _up(4*n_idx) + lists + 16*256


def member_bytes(A, N, W, d, n_idx, s_ndim, host):
    """Device bytes one member adds to a pass at most: its pointer, results, flag, the partial sums of the
    frequency chunks, the workspace of its cumulant functions and -- for a control matrix held as a host array
    (*host*) -- its row of the uploaded table."""
    pairs = pairs_of(n_idx, s_ndim)
    chunks = decay_chunks(W)
    dd = d*d
    cumulant = pairs*(2*_up(16*N*dd) + 2*_up(16*dd*dd))
    return (8 + 4 + 8*N*N*(pairs*(2 + (chunks if chunks > 1 else 0)) + 1) + cumulant
            + (16*A*N*W if host else 0))


def max_members(n_idx, s_ndim, single_qubit):
    """Members one pass can hold whatever their size: 65535 grid rows, and 65535 cumulant functions per launch
    unless the single-qubit expression serves them."""
    return MAX_MEMBERS if single_qubit else max(1, MAX_MEMBERS//pairs_of(n_idx, s_ndim))


def shape_of(pulse):
    """(N, A, d) of *pulse*'s control matrix and basis."""
    return len(pulse.basis), len(pulse.n_opers), np.shape(pulse.basis)[-1]


def batchable_shape(N, A, d):
    return N <= MAX_BASIS_ELEMENTS and 2 <= d <= MAX_DIMENSION and 1 <= A <= MAX_NOISE_OPERATORS


def group_members(pulses, members, idx_of):
    """Indices *members* of *pulses* grouped by (N, A, d, selected indices) and basis, each group in input order
    (every member is on the frequency grid of the call, so the grid is no part of the key)."""
    groups = {}
    for i in members:
        key = shape_of(pulses[i]) + (tuple(int(k) for k in idx_of[i]),)
        candidates = groups.setdefault(key, [])
        basis = pulses[i].basis
        for group in candidates:
            first = pulses[group[0]].basis
            if first is basis or (getattr(first, 'btype', None) == getattr(basis, 'btype', None)
                                  and np.array_equal(np.asarray(first), np.asarray(basis))):
                group.append(i)
                break
        else:
            candidates.append([i])
    return [group for candidates in groups.values() for group in candidates]


def split_group(group, is_host, A, N, W, d, n_idx, s_ndim, single_qubit, budget=None):
    """*group* in consecutive passes under ``batch.PASS_BYTES`` (every member counted as the largest of the
    group: with its table row if any member is a host array) and of at most :func:`max_members` members."""
    budget = batch.PASS_BYTES if budget is None else budget
    per_member = member_bytes(A, N, W, d, n_idx, s_ndim, any(is_host))
    room = max(per_member, budget - fixed_bytes(A, N, W, d, n_idx, s_ndim))
    return batch.split_passes(group, per_member, room, max_members(n_idx, s_ndim, single_qubit))


def _source(pulse, omega, W):
    """How the batched route reads *pulse*'s control matrix: ('resident', handle, slot), ('host', array) or None
    (not known on this grid, or of a shape the batched kernels do not take)."""
    from .pulse_sequence import _same_grid
    from .sequences import resident_source
    known = pulse._frequency_data
    if 'control_matrix' not in known or not _same_grid(pulse.omega, omega):
        return None
    N, A, d = shape_of(pulse)
    if not batchable_shape(N, A, d):
        return None
    entry = known.peek('control_matrix')
    resident = resident_source(pulse, d, W, N, A)
    if resident is not None:
        return ('resident',) + resident
    if type(entry) is Deferred or np.shape(entry) != (A, N, W):
        return None
    return 'host', entry


def _prepare(pulses, omega):
    """Pulses with nothing cached and a shape the batched route takes go through ``batch._run_pass`` (groups of
    one: their own resident pass), leaving what ``pulse.cache_control_matrix(omega)`` leaves."""
    fresh = [i for i, p in enumerate(pulses)
             if 'control_matrix' not in p._frequency_data and batchable_shape(*shape_of(p))
             and p.nothing_cached_for(omega)]
    everything = [np.arange(len(p.n_opers)) for p in pulses]
    grouped = set()
    for members in batch.group_pulses(pulses, fresh, everything):
        first = pulses[members[0]]
        per_pulse = batch.pass_bytes(len(first.dt), first.d, len(first.n_opers), len(first.basis), len(first.omega),
                                     len(first.c_opers))
        for chunk in batch.split_passes(members, per_pulse):
            batch._run_pass(pulses, chunk, first.omega, np.asarray(first.basis), keep_filter_function=False)
            grouped.update(chunk)
    for i in fresh:
        if i not in grouped:
            pulses[i].cache_control_matrix(omega)


def _run_pass(pulses, members, sources, omega, spectrum, idx, stage):
    """One call of ``ffk_resident_batch_processes`` over ``pulses[i] for i in members``; returns the requested
    array (P, ...) and the flags of the members whose result is not finite."""
    first = pulses[members[0]]
    N, A, d = shape_of(first)
    basis = first.basis
    P, W = len(members), len(omega)
    handles = (ctypes.c_void_p*P)(*(None if sources[i][0] == 'host' else sources[i][1].value for i in members))
    slots = np.array([-1 if sources[i][0] == 'host' else sources[i][2] for i in members], dtype=np.int32)
    host = [sources[i][1] for i in members if sources[i][0] == 'host']
    table = as_c128(np.stack(host)) if host else None
    S, idx, omega = as_c128(spectrum), np.ascontiguousarray(idx, dtype=np.int32), as_f64(omega)
    B = as_c128(np.asarray(basis))
    single_qubit = int(d == 2 and N == 4 and getattr(basis, 'btype', None) in ('Pauli', 'GGM'))
    n_idx = len(idx)
    rows = (n_idx, n_idx) if S.ndim == 3 else (n_idx,)
    out = np.empty((P, N, N) if stage == 'error_transfer_matrix' else (P,) + rows + (N, N), dtype=np.float64)
    flags = np.zeros(P, dtype=np.int32)
    outputs = [out.ctypes.data if stage == name else None for name in _STAGES]
    check(_lib.load().ffk_resident_batch_processes(
        handles, slots.ctypes.data, None if table is None else table.ctypes.data, P, A, N, W, d, omega.ctypes.data,
        B.ctypes.data, single_qubit, S.ctypes.data, S.ndim, idx.ctypes.data, n_idx, *outputs, flags.ctypes.data))
    if stage == 'error_transfer_matrix':
        bad = flags != 0
    else:
        bad = ~np.isfinite(out.reshape(P, -1)).all(axis=1)
    return out, bad


def _single(stage, pulse, spectrum, omega, n_oper_identifiers):
    if stage == 'decay_amplitudes':
        return numeric.calculate_decay_amplitudes(pulse, spectrum, omega, n_oper_identifiers)
    if stage == 'cumulant_function':
        return numeric.calculate_cumulant_function(pulse, spectrum, omega, n_oper_identifiers)
    return numeric.error_transfer_matrix(pulse, spectrum, omega, n_oper_identifiers)


def _results(stage, pulses, spectrum, omega, n_oper_identifiers):
    pulses = list(pulses)
    if not pulses:
        return np.empty((0,), dtype=np.float64)
    idx_of = [util.get_indices_from_identifiers(p.n_oper_identifiers, n_oper_identifiers) for p in pulses]
    shapes = {(len(idx), len(p.basis)) for idx, p in zip(idx_of, pulses)}
    if len(shapes) > 1:
        raise ValueError('Every pulse must give the same output shape: the pulses have (selected noise operators, '
                         f'basis elements) = {sorted(shapes)}.')
    spectrum = np.asanyarray(spectrum)
    _prepare(pulses, omega)
    W = len(omega)
    sources = {}
    for i, pulse in enumerate(pulses):
        source = _source(pulse, omega, W)
        if source is not None:
            sources[i] = source
    out = [None]*len(pulses)
    for group in group_members(pulses, sorted(sources), idx_of):
        first = pulses[group[0]]
        N, A, d = shape_of(first)
        idx = idx_of[group[0]]
        parsed = util.parse_spectrum(spectrum, as_f64(omega), np.asarray(idx))
        single_qubit = d == 2 and N == 4 and getattr(first.basis, 'btype', None) in ('Pauli', 'GGM')
        is_host = [sources[i][0] == 'host' for i in group]
        for members in split_group(group, is_host, A, N, W, d, len(idx), parsed.ndim, single_qubit):
            values, bad = _run_pass(pulses, members, sources, omega, parsed, idx, stage)
            for j, i in enumerate(members):
                if not bad[j]:
                    out[i] = values[j]
    # everything else, and the members whose result is not finite: what the loop does
    for i, pulse in enumerate(pulses):
        if out[i] is None:
            out[i] = _single(stage, pulse, spectrum, omega, n_oper_identifiers)
    return np.stack(out)


def decay_amplitudes(pulses, spectrum, omega, n_oper_identifiers=None):
    r"""Decay amplitudes :math:`\Gamma_{\alpha\beta,kl}` of many pulses on one spectrum and frequency grid, shape
    (n_pulses, n_idx, N, N) or, for a spectrum of shape (n_idx, n_idx, n_omega), (n_pulses, n_idx, n_idx, N, N):
    ``np.stack([numeric.calculate_decay_amplitudes(p, spectrum, omega, n_oper_identifiers) for p in pulses])``.

    Routing, per pulse.  A pulse whose control matrix is cached on this grid, with at most 16 basis elements
    (d = 2, 3, 4) and at most four noise operators, takes the batched route: a control matrix resident in HBM (a
    single resident result, a member of an ``ff.get_filter_functions`` pass, a result of
    ``ff.concatenate_sequences``) is read in place -- its deferred cache entry is NOT produced --, a host array
    is uploaded once per pass.  Pulses of such shapes with nothing cached first run the batched pass of
    ``ff.get_filter_functions`` and are left as ``pulse.cache_control_matrix(omega)`` leaves them (no filter
    function).  Every other pulse (more basis elements or noise operators, a control matrix cached on another
    grid, pulses the batched pass cannot take), and every pulse whose result is not finite, runs the single
    function inside the call: correct results, the caches as the loop leaves them, no speed-up.

    Input order is kept.  The pulses must agree on the number of selected noise operators and of basis elements
    (else ValueError); an empty list gives an empty float array.  Pulse correlations and precomputed inputs are not
    offered: use the single functions.
    """
    return _results('decay_amplitudes', pulses, spectrum, omega, n_oper_identifiers)


def _second_order_cumulants(pulses, spectrum, omega, n_oper_identifiers):
    """First-order cumulant functions from the batched pass, frequency shifts from ``ff.frequency_shifts``, and
    the second-order term of all pulses (of one basis) added by one call of ``ffk_cumulant_function_second_order``:
    what ``numeric.calculate_cumulant_function(..., second_order=True)`` does for one pulse."""
    from .batch_second_order import _same_basis, frequency_shifts
    pulses = list(pulses)
    K = _results('cumulant_function', pulses, spectrum, omega, n_oper_identifiers)
    if not pulses:
        return K
    delta = frequency_shifts(pulses, spectrum, omega, n_oper_identifiers)
    if np.shape(delta) != np.shape(K):
        raise ValueError('Frequency shifts not same shape as decay amplitudes')
    K = np.ascontiguousarray(K, dtype=np.float64)
    todo = list(range(len(pulses)))
    while todo:
        basis = pulses[todo[0]].basis
        same = [i for i in todo if _same_basis(basis, pulses[i].basis)]
        todo = [i for i in todo if i not in same]
        N, d = np.shape(basis)[:2]
        numeric._check_d(d)
        C = as_c128(np.asarray(basis))
        part = np.ascontiguousarray(K[same]).reshape(-1, N, N)
        shifts = np.ascontiguousarray(as_f64(delta[same]).reshape(-1, N, N))
        check(_lib.load().ffk_cumulant_function_second_order(shifts.ctypes.data, len(shifts), N, d, C.ctypes.data,
                                                             part.ctypes.data))
        K[same] = part.reshape((len(same),) + K.shape[1:])
    return K


def cumulant_functions(pulses, spectrum, omega, n_oper_identifiers=None, second_order=False):
    r"""Cumulant functions :math:`\mathcal{K}_{\alpha\beta}` of many pulses, same shape as
    :func:`decay_amplitudes`: ``np.stack([numeric.calculate_cumulant_function(p, spectrum, omega,
    n_oper_identifiers, second_order=second_order) for p in pulses])``.  Routing, shapes and exceptions as
    :func:`decay_amplitudes`.  With *second_order* the frequency shifts come from :func:`ff.frequency_shifts
    <filter_functions_amd.batch_second_order.frequency_shifts>` (whose routing and caches apply) and their
    contribution to every pulse's cumulant function is added in one call."""
    if second_order:
        return _second_order_cumulants(pulses, spectrum, omega, n_oper_identifiers)
    return _results('cumulant_function', pulses, spectrum, omega, n_oper_identifiers)


def error_transfer_matrices(pulses, spectrum, omega, n_oper_identifiers=None, second_order=False):
    r"""Error transfer matrices :math:`\exp\mathcal{K}` of many pulses, shape (n_pulses, N, N):
    ``np.stack([ff.error_transfer_matrix(p, spectrum, omega, n_oper_identifiers, second_order=second_order) for p in
    pulses])``.  The sum over the noise operators, the norm, the choice of the squarings and the exponential run on
    the device, one wavefront per pulse.  Routing, shapes and exceptions as :func:`decay_amplitudes`.  With
    *second_order* the cumulant functions are those of :func:`cumulant_functions` with ``second_order=True``, each
    exponentiated as ``ff.error_transfer_matrix(cumulant_function=...)`` does."""
    if second_order:
        K = _second_order_cumulants(pulses, spectrum, omega, n_oper_identifiers)
        if not len(K):
            return K
        return np.stack([numeric.error_transfer_matrix(cumulant_function=k) for k in K])
    return _results('error_transfer_matrix', pulses, spectrum, omega, n_oper_identifiers)

"""Many pulses of one shape in one pass (``ffk_resident_batch_*``, include/ffk.h).

``ff.get_filter_functions(pulses, omega)`` and ``ff.infidelities(pulses, S, omega)`` are the loops
``[p.get_filter_function(omega) for p in pulses]`` and ``[ff.infidelity(p, S, omega) for p in pulses]``,
with the pulses that have nothing cached grouped by shape and every group evaluated in batched passes:
one H2D copy of the packed inputs, one launch per stage with the pulse as a grid axis, one D2H copy of
the eigensystems, propagators, filter functions and infidelities of all pulses.  Afterwards every member
holds in its caches what its own resident pass would have left (the control matrix stays in HBM behind
a :class:`~filter_functions_amd._resident.Deferred` entry that fetches that pulse's slice).
"""
import ctypes
import functools

import numpy as np

from . import numeric, util
from ._lib import as_c128, as_f64, check
from ._resident import Deferred, ResidentHandle, _view, spectrum_arguments

__all__ = ['get_filter_functions', 'infidelities']

#: Device bytes one batched pass may hold (inputs, results, workspace): a larger group is split into passes.
PASS_BYTES = 1 << 30
#: Pulses per pass at most (the pulse is a grid axis of at most 65535 blocks).
MAX_PULSES = 8192


class BatchResult(ResidentHandle):
    """Owns one ``ffk_resident`` handle filled by a batched pass: the device-resident control matrices
    and the pinned host block the per-pulse results live in.  Shared by the members of the pass, freed
    when the last of them lets go."""

    def evaluate(self, c_opers, c_coeffs, dt, t, omega, basis, n_opers, n_coeffs, spectrum=None, idx=None,
                 d_infidelity=None):
        """One batched pass over the stacked per-pulse arrays (leading axis P).  Returns (eigvals,
        eigvecs, propagators, filter_function, infidelities or None, n_failed); the first four view
        the handle's pinned memory.  Raises LinAlgError if a segment did not converge (n_failed says
        where: ``err.n_failed``)."""
        C, c, dt, t, omega = as_c128(c_opers), as_f64(c_coeffs), as_f64(dt), as_f64(t), as_f64(omega)
        B, s, basis = as_c128(n_opers), as_f64(n_coeffs), as_c128(basis)
        P, n_c, d = C.shape[:3]
        G, W, N, A = dt.shape[1], len(omega), len(basis), B.shape[1]
        out = [ctypes.c_void_p() for _ in range(4)]
        n_failed = np.zeros(P, dtype=np.int32)
        infid = S = None
        s_ndim = real = n_idx = 0
        if spectrum is not None:
            S, real, idx, out_shape = spectrum_arguments(spectrum, idx)
            s_ndim, n_idx = S.ndim, len(idx)
            infid = np.empty((P,) + out_shape, dtype=np.float64)
        status = self._lib.ffk_resident_batch_filter_function_infidelity(
            self._handle, P, C.ctypes.data, n_c, c.ctypes.data, dt.ctypes.data, t.ctypes.data, G, d,
            omega.ctypes.data, W, basis.ctypes.data, N, B.ctypes.data, A, s.ctypes.data,
            None if S is None else S.ctypes.data, s_ndim, real, None if S is None else idx.ctypes.data, n_idx,
            int(d_infidelity or d), *(ctypes.byref(p) for p in out),
            None if infid is None else infid.ctypes.data, n_failed.ctypes.data)
        try:
            check(status)
        except np.linalg.LinAlgError as err:
            err.n_failed = n_failed
            raise
        self.shape = (P, G, d, W, N, A)
        D = _view(out[0].value, P*G*d, np.float64, (P, G, d), self)
        V = _view(out[1].value, 2*P*G*d*d, np.complex128, (P, G, d, d), self)
        Q = _view(out[2].value, 2*P*(G + 1)*d*d, np.complex128, (P, G + 1, d, d), self)
        F = _view(out[3].value, 2*P*A*A*W, np.complex128, (P, A, A, W), self)
        F.flags.writeable = False      # (as the single resident pass: a view of pinned memory)
        return D, V, Q, F, infid

    def control_matrix(self, pulse):
        """Pulse *pulse*'s control matrix (n_nops, n_basis, n_omega), copied to the host now."""
        P, G, d, W, N, A = self.shape
        R = np.empty((A, N, W), dtype=np.complex128)
        check(self._lib.ffk_resident_batch_control_matrix(self._handle, int(pulse), R.ctypes.data))
        return R


class _Member:
    """``pulse._resident`` of a batch member: keeps the batch alive, but is no single-pulse resident
    result (no ``shape``, no resident filter function), so the integral of a later ``ff.infidelity`` and
    ``concatenate`` take their array routes (``ff.concatenate_sequences`` reads member ``slot`` in place).  Copies
    of the pulse drop it, as they drop a resident result."""
    __slots__ = ('batch', 'slot')
    shape = None
    filter_function = None

    def __init__(self, batch, slot=None):
        self.batch, self.slot = batch, slot      # (slot: the pulse's index in the pass)

    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (type(None), ())


def _shape_key(pulse, idx):
    """Pulses with equal keys (and equal bases) can share a pass."""
    return (pulse.d, len(pulse.dt), len(pulse.c_opers), len(pulse.n_opers), len(pulse.basis), tuple(idx))


def group_pulses(pulses, eligible, idx_of):
    """Indices of the *eligible* pulses grouped by shape and basis, each group in input order; the
    groups of one pulse are left out (they take the single route)."""
    groups = {}
    for i in eligible:
        key = _shape_key(pulses[i], idx_of[i])
        candidates = groups.setdefault(key, [])
        basis = np.asarray(pulses[i].basis)
        for members in candidates:
            first = np.asarray(pulses[members[0]].basis)
            if first is basis or np.array_equal(first, basis):
                members.append(i)
                break
        else:
            candidates.append([i])
    return [members for candidates in groups.values() for members in candidates if len(members) > 1]


def pass_bytes(G, d, A, N, W, n_cops):
    """Device bytes one pulse adds to a batched pass: inputs, results, the control matrix and the
    workspace of the stages (an upper bound of ``ffk_pipeline_batch_workspace_bytes`` per pulse)."""
    dd = d*d
    segments = G*(16*dd*(n_cops + 8 + 2*A) + 8*(4 + 4*dd) + 8*(n_cops + A + 2) + 8*d + 16*A*512)
    frequencies = 16*A*W*(N + A + dd)
    return segments + frequencies + 4096


def split_passes(members, per_pulse, budget=PASS_BYTES, max_pulses=MAX_PULSES):
    """*members* in consecutive passes of at most *budget* bytes (but at least two pulses) and at most
    *max_pulses* pulses, their sizes differing by one at most."""
    n = len(members)
    if n == 0:
        return []
    per_pass = max(2, min(max_pulses, budget//max(1, per_pulse)))
    n_pass = -(-n//per_pass)
    bounds = [n*k//n_pass for k in range(n_pass + 1)]
    return [members[a:b] for a, b in zip(bounds[:-1], bounds[1:])]


def _run_pass(pulses, members, omega, basis, spectrum=None, idx=None, keep_filter_function=True):
    """One batched pass over ``pulses[i] for i in members``; fills their caches.  Returns the filter functions
    (P, A, A, W) and the infidelities (P, ...) or None.  *keep_filter_function* False leaves the filter function
    out of the members' caches: what ``pulse.cache_control_matrix(omega)`` leaves."""
    group = [pulses[i] for i in members]
    stack = lambda f: np.stack([f(p) for p in group])      # noqa: E731
    batch = BatchResult()
    integral = {} if spectrum is None else dict(spectrum=spectrum, idx=idx, d_infidelity=group[0].d)
    try:
        D, V, Q, F, infid = batch.evaluate(stack(lambda p: p.c_opers), stack(lambda p: p.c_coeffs),
                                           stack(lambda p: p.dt), stack(lambda p: p.t), omega, basis,
                                           stack(lambda p: p.n_opers), stack(lambda p: p.n_coeffs), **integral)
    except np.linalg.LinAlgError as err:
        failed = [members[j] for j in np.flatnonzero(getattr(err, 'n_failed', []))]
        if not failed:
            raise
        raise np.linalg.LinAlgError(f'Eigensolver did not converge for pulse {failed[0]} of the list '
                                    f'({int(err.n_failed[members.index(failed[0])])} segment(s)); '
                                    f'pulses that failed: {failed}') from err
    nbytes = 16*F.shape[1]*len(basis)*F.shape[3]
    for j, pulse in enumerate(group):
        pulse._data.update(eigvals=D[j], eigvecs=V[j], propagators=Q[j], total_propagator=Q[j][-1])
        pulse._frequency_data['control_matrix'] = Deferred(functools.partial(batch.control_matrix, j), nbytes)
        if keep_filter_function:
            pulse._frequency_data['filter_function'] = F[j]
        pulse._defer_by_products()
        pulse._resident = _Member(batch, j)
    return F, infid


def _sequence_pass_integrals(pulses, spectrum, omega, idx_of, eligible, out):
    """The infidelities of results of ``ff.concatenate_sequences`` whose resident filter function ``ff.infidelity``
    would integrate in place: the members of one pass (same selected operators and dimension) in ONE launch."""
    from .sequences import _SequenceMember
    skip = set(eligible)
    groups = {}
    for i, pulse in enumerate(pulses):
        member = pulse._resident
        if i in skip or not isinstance(member, _SequenceMember) or not pulse.basis.istraceless:
            continue
        # (what ff.infidelity reads before it asks pulse.resident_infidelity)
        if pulse.get_filter_function(omega, which='fidelity') is not member.filter_function \
                or pulse._resident is not member:
            continue
        key = (id(member.batch), tuple(int(k) for k in idx_of[i]), pulse.d)
        groups.setdefault(key, (member.batch, []))[1].append(i)
    for (_, idx, d), (batch, members) in groups.items():
        parsed = util.parse_spectrum(spectrum, as_f64(omega), np.asarray(idx))
        values = batch.infidelities([pulses[i]._resident.slot for i in members], parsed, idx, d)
        for i, value in zip(members, values):
            out[i] = value


def _results(pulses, omega, spectrum, n_oper_identifiers):
    """Per input pulse its filter function (spectrum None) or infidelity, batched where possible."""
    from .pulse_sequence import WRITABLE_RESULTS
    with_integral = spectrum is not None
    idx_of = [util.get_indices_from_identifiers(p.n_oper_identifiers, n_oper_identifiers) if with_integral
              else np.arange(len(p.n_opers)) for p in pulses]
    lengths = {len(idx) for idx in idx_of}
    if len(lengths) > 1:
        raise ValueError('Every pulse must give the same output shape: the pulses have '
                         f'{sorted(lengths)} selected noise operators.')
    eligible = [i for i, p in enumerate(pulses)
                if p.nothing_cached_for(omega) and (not with_integral or p.basis.istraceless)]
    out = [None]*len(pulses)
    if with_integral:
        _sequence_pass_integrals(pulses, spectrum, omega, idx_of, eligible, out)
    whole = None          # F of a single pass that covers the whole list in input order: returned as it is
    for members in group_pulses(pulses, eligible, idx_of):
        first = pulses[members[0]]
        parsed = (util.parse_spectrum(spectrum, as_f64(omega), np.asarray(idx_of[members[0]]))
                  if with_integral else None)
        per_pulse = pass_bytes(len(first.dt), first.d, len(first.n_opers), len(first.basis), len(omega),
                               len(first.c_opers))
        # (the limits as they stand at the call: the defaults of split_passes are those of import time)
        for chunk in split_passes(members, per_pulse, PASS_BYTES, MAX_PULSES):
            F, infid = _run_pass(pulses, chunk, first.omega, np.asarray(first.basis), parsed, idx_of[members[0]])
            if len(chunk) == len(pulses):
                whole = F
            for j, i in enumerate(chunk):
                out[i] = infid[j] if with_integral else F[j]
    for i, pulse in enumerate(pulses):
        if out[i] is None:
            out[i] = (numeric.infidelity(pulse, spectrum, omega, n_oper_identifiers=n_oper_identifiers)
                      if with_integral else pulse.get_filter_function(omega, writable=False))
    if not with_integral:
        shapes = {f.shape for f in out}
        if len(shapes) > 1:
            raise ValueError(f'Every pulse must give the same output shape, got filter functions of shapes '
                             f'{sorted(shapes)}.')
        result = whole if whole is not None else np.stack(out)
        if WRITABLE_RESULTS and not result.flags.writeable:
            result = np.array(result)
        elif not WRITABLE_RESULTS:
            result.flags.writeable = False
        return result
    return np.stack(out)


def get_filter_functions(pulses, omega):
    r"""Fidelity filter functions of many pulses on one frequency grid, shape
    (n_pulses, n_nops, n_nops, n_omega): ``np.stack([p.get_filter_function(omega) for p in pulses])``.

    Pulses with nothing cached are grouped by shape (dimension, number of segments, of control and noise
    operators, basis) and each group is evaluated in batched passes, one launch per stage for all its
    pulses.  Afterwards every pulse's caches hold what ``pulse.get_filter_function(omega)`` would have left
    (eigensystem, propagators, the filter function, a deferred control matrix).  Every pulse must have the
    same number of noise operators (else ValueError); an empty list gives an empty complex array.
    """
    pulses = list(pulses)
    if not pulses:
        return np.empty((0,), dtype=np.complex128)
    return _results(pulses, omega, None, None)


def infidelities(pulses, spectrum, omega, n_oper_identifiers=None, which='total'):
    r"""Leading-order entanglement infidelities of many pulses on one spectrum and frequency grid,
    shape (n_pulses, n_idx) or, for a spectrum of shape (n_idx, n_idx, n_omega), (n_pulses, n_idx, n_idx):
    ``np.stack([ff.infidelity(p, spectrum, omega, n_oper_identifiers) for p in pulses])``.

    Pulses with nothing cached are grouped by shape and selected noise operators and evaluated in
    batched passes (filter functions and integrals of a whole group in one round trip to the device); the
    caches are left as ``ff.infidelity`` leaves them.  Every pulse must select the same number of noise
    operators (else ValueError); an empty list gives an empty float array.  Only ``which='total'``: other
    values raise what ``ff.infidelity`` raises.
    """
    pulses = list(pulses)
    if which != 'total':
        # (pulse correlations: not batched; the same exceptions and results as the loop)
        return np.array([numeric.infidelity(p, spectrum, omega, n_oper_identifiers, which=which) for p in pulses])
    if not pulses:
        return np.empty((0,), dtype=np.float64)
    return _results(pulses, omega, np.asarray(spectrum), n_oper_identifiers)

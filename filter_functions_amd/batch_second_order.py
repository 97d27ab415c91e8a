"""Frequency shifts of many pulses in one pass (``ffk_batch_frequency_shifts``, include/ffk.h).

``ff.frequency_shifts(pulses, S, omega)`` is the loop ``[numeric.calculate_frequency_shifts(p, S, omega) for p in
pulses]``, stacked.  Pulses of a shape for which the single pass runs its matrix-core kernel
(``ffk_batch_frequency_shifts_chunk(...) > 0``) and with no second-order filter function cached are grouped by
(dimension, segments, noise operators, basis, selected operators), and every group of two or more is evaluated in
batched passes: the eigensystems and operators of all members cross once, a fixed number of launches with the pulse
as a grid axis follows (``csrc/second.hip``: ``so_shift_kernel``), one copy brings the result back.  The
second-order filter function -- ``(n_nops, n_nops, d**2, d**2, n_omega)`` complex numbers per pulse on the single
path -- is never in memory: every block integrates its frequencies against the spectrum itself, and only the tiles of
the output that hold a selected operator pair are computed.  Every other pulse -- another shape, the second-order
filter function already cached, a group of one, an operator selected twice -- runs the single function inside the
call.

One deviation from the loop.  A batched member ends diagonalised (see ``batch_gradient``: through the batched pass of
``ff.get_filter_functions`` where nothing was cached, ``pulse.diagonalize()`` otherwise) and with ``pulse.omega`` set,
but WITHOUT ``filter_function_2`` in its cache: the single function caches it, which for a population would be the
batch size times its bytes (151 MB each at d = 4, three noise operators, 4096 frequencies).  A later
``pulse.get_filter_function(omega, order=2)`` computes it as before.
"""
import ctypes

import numpy as np

from . import _lib, batch, numeric, util
from ._lib import as_c128, as_f64, check, ptr
from .batch_gradient import _diagonalize, dimension_of

__all__ = ['frequency_shifts']

#: Pulses per pass at most (the pulse is a grid axis).
MAX_PULSES = 65535


def shape_of(pulse):
    """(W-independent) shape of a pulse's second-order pass: (d, G, A, N)."""
    return dimension_of(pulse), len(pulse.dt), len(pulse.n_opers), len(pulse.basis)


def chunk(W, N, A, G, d):
    """Frequencies one block of the fused kernel walks; 0: the batched pass does not take the shape."""
    return int(_lib.load().ffk_batch_frequency_shifts_chunk(W, N, A, G, d))


def batchable(pulse, W, idx):
    """The shape is one of the matrix-core kernel's, every operator is selected once, and there is no second-order
    filter function to reuse."""
    d, G, A, N = shape_of(pulse)
    return (len(set(int(k) for k in idx)) == len(idx) >= 1 and chunk(W, N, A, G, d) > 0
            and not pulse.is_cached('filter_function_2'))


def _same_basis(first, basis):
    return first is basis or (getattr(first, 'btype', None) == getattr(basis, 'btype', None)
                              and np.array_equal(np.asarray(first), np.asarray(basis)))


def group_members(pulses, eligible, idx_of):
    """The *eligible* indices grouped by (d, G, A, N, selected noise indices) and basis, each group in input order,
    the groups in order of their first member; groups of one included."""
    groups = {}
    for i in eligible:
        key = shape_of(pulses[i]) + (tuple(int(k) for k in idx_of[i]),)
        candidates = groups.setdefault(key, [])
        for group in candidates:
            if _same_basis(pulses[group[0]].basis, pulses[i].basis):
                group.append(i)
                break
        else:
            candidates.append([i])
    return sorted((group for candidates in groups.values() for group in candidates), key=lambda g: g[0])


def pulse_bytes(W, N, A, G, d, n_idx, s_ndim):
    """(device bytes every pulse adds to a pass, bytes of a pass that do not depend on P)."""
    query = _lib.load().ffk_batch_frequency_shifts_workspace_bytes
    one, two = query(1, W, N, A, G, d, n_idx, s_ndim), query(2, W, N, A, G, d, n_idx, s_ndim)
    return two - one, 2*one - two


def split_group(members, W, N, A, G, d, n_idx, s_ndim, budget=None):
    """*members* in consecutive passes under ``batch.PASS_BYTES`` (at least two pulses each) and of at most
    :data:`MAX_PULSES` pulses."""
    budget = batch.PASS_BYTES if budget is None else budget
    per_pulse, fixed = pulse_bytes(W, N, A, G, d, n_idx, s_ndim)
    return batch.split_passes(members, per_pulse, max(per_pulse, budget - fixed), MAX_PULSES)


def _run_pass(pulses, members, idx, S):
    """One call of ``ffk_batch_frequency_shifts`` over ``pulses[i] for i in members``."""
    group = [pulses[i] for i in members]
    stack = lambda f, conv: conv(np.stack([f(p) for p in group]))      # noqa: E731
    D = stack(lambda p: p.eigvals, as_f64)
    V = stack(lambda p: p.eigvecs, as_c128)
    Q = stack(lambda p: p.propagators, as_c128)
    B = stack(lambda p: p.n_opers, as_c128)
    s = stack(lambda p: p.n_coeffs, as_f64)
    dt = stack(lambda p: p.dt, as_f64)
    t = as_f64(np.concatenate((np.zeros((len(group), 1)), dt.cumsum(axis=1)), axis=1))
    omega = as_f64(group[0].omega)
    C = as_c128(np.asarray(group[0].basis))
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    S = as_c128(S)
    P, G, d = D.shape
    A, N, W, n_idx = B.shape[1], len(C), len(omega), len(idx)
    out = np.empty((P, n_idx, n_idx, N, N) if S.ndim == 3 else (P, n_idx, N, N), dtype=np.float64)
    check(_lib.load().ffk_batch_frequency_shifts(
        P, ptr(D), ptr(V), ptr(Q), ptr(omega), W, ptr(C), N, ptr(B), A, ptr(s), ptr(dt), ptr(t), G, d, ptr(S), S.ndim,
        idx.ctypes.data_as(ctypes.c_void_p), n_idx, ptr(out)))
    return out


def frequency_shifts(pulses, spectrum, omega, n_oper_identifiers=None):
    r"""Frequency shifts :math:`\Delta_{\alpha\beta,kl}` of many pulses on one spectrum and frequency grid, shape
    (n_pulses, n_idx, N, N) or, for a spectrum of shape (n_idx, n_idx, n_omega), (n_pulses, n_idx, n_idx, N, N):
    ``np.stack([numeric.calculate_frequency_shifts(p, spectrum, omega, n_oper_identifiers) for p in pulses])``.

    Pulses of a shape the matrix-core kernel of the second-order pass takes, with no ``filter_function_2`` cached,
    are grouped by shape, basis and selected operators, and each group of two or more runs in batched passes in which
    the second-order filter function is never stored.  Everything else runs the single function inside the call, and
    the exceptions are those of the loop.  Input order is kept.  The pulses must agree on the output shape (else
    ValueError); an empty list gives an empty float array.

    Unlike the loop, a batched member ends without ``filter_function_2`` in its cache (its eigensystem is cached and
    ``pulse.omega`` is set); see the module's docstring.
    """
    pulses = list(pulses)
    if not pulses:
        return np.empty((0,), dtype=np.float64)
    idx_of = [util.get_indices_from_identifiers(p.n_oper_identifiers, n_oper_identifiers) for p in pulses]
    shapes = {(len(idx), len(p.basis)) for idx, p in zip(idx_of, pulses)}
    if len(shapes) > 1:
        raise ValueError('Every pulse must give the same output shape: the pulses have (selected noise operators, '
                         f'basis elements) = {sorted(shapes)}.')
    W = len(as_f64(omega))
    eligible = [i for i, p in enumerate(pulses) if batchable(p, W, idx_of[i])]
    out = [None]*len(pulses)
    for members in group_members(pulses, eligible, idx_of):
        if len(members) < 2:
            continue
        first = members[0]
        idx = np.asarray(idx_of[first])
        for i in members:
            pulses[i].omega = omega
        S = util.parse_spectrum(spectrum, as_f64(pulses[first].omega), idx)
        _diagonalize(pulses, members, omega)
        d, G, A, N = shape_of(pulses[first])
        for part in split_group(members, W, N, A, G, d, len(idx), S.ndim):
            values = _run_pass(pulses, part, idx, S)
            for j, i in enumerate(part):
                out[i] = values[j]
    for i, pulse in enumerate(pulses):
        if out[i] is None:
            out[i] = numeric.calculate_frequency_shifts(pulse, spectrum, omega, n_oper_identifiers)
    return np.stack(out)

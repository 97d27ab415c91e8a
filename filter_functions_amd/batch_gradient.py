"""Gradients of many pulses in one pass (``ffk_batch_filter_function_derivative``, include/ffk.h).

``ff.infidelity_derivatives(pulses, S, omega)`` and ``ff.filter_function_derivatives(pulses, omega)`` are the loops
``[gradient.infidelity_derivative(p, S, omega) for p in pulses]`` and
``[gradient.filter_function_derivative(p, omega) for p in pulses]``, stacked.  Pulses of dimension 2 to 4 with at
most 4 selected noise and 8 selected control operators are grouped by (dimension, number of segments, selected
control indices, selected noise indices) and every group of two or more is evaluated in batched passes: one H2D
copy of the packed eigensystems and operators, a fixed number of launches with the pulse as a grid axis
(``csrc/grad_batch.hip``), one D2H copy of the result.  Every other pulse, and a group of one, runs the single
function inside the call.

Eigensystems.  A pulse that is diagonalised contributes its cached ``eigvals``, ``eigvecs`` and ``propagators``;
they are read, not rewritten.  Pulses of a batched group that are not diagonalised and have nothing cached first go
through the batched pass of ``ff.get_filter_functions`` (``batch._run_pass(..., keep_filter_function=False)``, as
``ff.decay_amplitudes`` does): they end up diagonalised AND with the deferred control matrix that pass leaves.  What
is left over is diagonalised by ``pulse.diagonalize()``.  Every pulse ends with ``pulse.omega`` set, as the loop
leaves it.

An optimiser that wants the infidelity and its gradient of a population calls ``ff.infidelities`` first and
``ff.infidelity_derivatives`` second: the first call diagonalises every member in its batched pass, the second
reads those eigensystems -- both are batched and nothing is diagonalised twice.
"""
import numpy as np

from . import _lib, batch, gradient, util
from ._lib import as_c128, as_f64, check, ptr

__all__ = ['filter_function_derivatives', 'infidelity_derivatives']

#: Pulses per pass at most (the pulse is a grid axis).
MAX_PULSES = 65535
MAX_D, MAX_NOISE_OPERS, MAX_CONTROL_OPERS = 4, 4, 8


def batchable_shape(d, n_nops, n_ctrl):
    """The shapes the batched kernels take: dimension, selected noise operators, selected control operators."""
    return 2 <= d <= MAX_D and 1 <= n_nops <= MAX_NOISE_OPERS and 1 <= n_ctrl <= MAX_CONTROL_OPERS


def dimension_of(pulse):
    return int(np.shape(pulse.c_opers)[-1])


def group_members(pulses, eligible, c_idx_of, n_idx_of):
    """The *eligible* indices grouped by (d, G, selected control indices, selected noise indices), each group in
    input order, the groups in order of their first member; groups of one included."""
    groups = {}
    for i in eligible:
        key = (dimension_of(pulses[i]), len(pulses[i].dt), tuple(int(k) for k in c_idx_of[i]),
               tuple(int(k) for k in n_idx_of[i]))
        groups.setdefault(key, []).append(i)
    return list(groups.values())


def pulse_bytes(W, A, H, G, d, want_dF):
    """(device bytes every pulse adds to a pass, bytes of a pass that do not depend on P)."""
    query = _lib.load().ffk_batch_filter_function_derivative_workspace_bytes
    one, two = query(1, W, A, H, G, d, int(want_dF)), query(2, W, A, H, G, d, int(want_dF))
    return two - one, 2*one - two


def split_group(members, W, A, H, G, d, want_dF, budget=None):
    """*members* in consecutive passes under ``batch.PASS_BYTES`` (at least two pulses each) and of at most
    :data:`MAX_PULSES` pulses."""
    budget = batch.PASS_BYTES if budget is None else budget
    per_pulse, fixed = pulse_bytes(W, A, H, G, d, want_dF)
    return batch.split_passes(members, per_pulse, max(per_pulse, budget - fixed), MAX_PULSES)


def _validate(pulse, omega, control_identifiers, n_oper_identifiers, n_coeffs_deriv, spectrum):
    """What ``gradient._derivative`` checks before it computes, in its order; sets ``pulse.omega``.  Returns the
    selected control and noise indices and the parsed spectrum (or None)."""
    c_idx = util.get_indices_from_identifiers(pulse.c_oper_identifiers, control_identifiers)
    n_idx = util.get_indices_from_identifiers(pulse.n_oper_identifiers, n_oper_identifiers)
    if n_coeffs_deriv is not None:
        actual_shape = np.shape(n_coeffs_deriv)
        required_shape = (len(n_idx), len(c_idx), len(pulse))
        if actual_shape != required_shape:
            raise ValueError(f'Expected n_coeffs_deriv to be of shape {required_shape}, '
                             f'not {actual_shape}. Did you forget to specify identifiers?')
    pulse.omega = omega
    d = dimension_of(pulse)
    if not 2 <= d <= 8:
        raise ValueError(f'The gradient kernels support 2 <= d <= 8, not d={d}.')
    S = None
    if spectrum is not None:
        S = util.parse_spectrum(spectrum, as_f64(pulse.omega), range(len(pulse.n_opers)))
        if S.ndim == 3:
            raise ValueError('Expected spectrum of shape (n_omega,) or (n_nops, n_omega) for the '
                             'infidelity derivative.')
        if S.ndim == 2 and len(n_idx) != len(pulse.n_opers):
            raise ValueError(f'Spectrum of shape {S.shape} does not match {len(n_idx)} selected '
                             'noise operators.')
    return c_idx, n_idx, S


def _diagonalize(pulses, members, omega):
    """The members that are not diagonalised: through the batched pass of ``ff.get_filter_functions`` where it
    applies (groups of two or more with nothing cached), ``pulse.diagonalize()`` otherwise."""
    from .pulse_sequence import _DIAGONALIZATION
    todo = [i for i in members if any(key not in pulses[i]._data for key in _DIAGONALIZATION)]
    fresh = [i for i in todo if pulses[i].nothing_cached_for(omega)]
    everything = [np.arange(len(p.n_opers)) for p in pulses]
    done = set()
    for group in batch.group_pulses(pulses, fresh, everything):
        first = pulses[group[0]]
        per_pulse = batch.pass_bytes(len(first.dt), first.d, len(first.n_opers), len(first.basis), len(first.omega),
                                     len(first.c_opers))
        for chunk in batch.split_passes(group, per_pulse):
            batch._run_pass(pulses, chunk, first.omega, np.asarray(first.basis), keep_filter_function=False)
            done.update(chunk)
    for i in todo:
        if i not in done:
            pulses[i].diagonalize()


def _run_pass(pulses, members, c_idx, n_idx, ratios, S, want_dF):
    """One call of ``ffk_batch_filter_function_derivative`` over ``pulses[i] for i in members``."""
    group = [pulses[i] for i in members]
    stack = lambda f, conv: conv(np.stack([f(p) for p in group]))      # noqa: E731
    D = stack(lambda p: p.eigvals, as_f64)
    V = stack(lambda p: p.eigvecs, as_c128)
    Q = stack(lambda p: p.propagators, as_c128)
    B = stack(lambda p: p.n_opers[n_idx], as_c128)
    s = stack(lambda p: p.n_coeffs[n_idx], as_f64)
    C = stack(lambda p: p.c_opers[c_idx], as_c128)
    dt = stack(lambda p: p.dt, as_f64)
    t = as_f64(np.concatenate((np.zeros((len(group), 1)), dt.cumsum(axis=1)), axis=1))
    omega = as_f64(group[0].omega)
    P, G, d = D.shape
    A, H, W = B.shape[1], C.shape[1], len(omega)
    ratio = None
    if ratios is not None:
        ratio = as_f64(np.stack([np.asarray(ratios[i], dtype=float) for i in members])/s[:, :, None, :])
    dF = np.empty((P, A, G, H, W), dtype=np.float64) if want_dF else None
    dI = np.empty((P, A, G, H), dtype=np.float64) if not want_dF else None
    S = as_c128(S) if S is not None else None
    check(_lib.load().ffk_batch_filter_function_derivative(
        P, ptr(D), ptr(V), ptr(Q), ptr(omega), W, ptr(B), A, ptr(s), ptr(C), H,
        ptr(ratio) if ratio is not None else None, ptr(dt), ptr(t), G, d,
        ptr(S) if S is not None else None, S.ndim if S is not None else 0,
        ptr(dF) if dF is not None else None, ptr(dI) if dI is not None else None))
    return dF if want_dF else dI


def _derivatives(pulses, omega, control_identifiers, n_oper_identifiers, n_coeffs_deriv, spectrum):
    want_dF = spectrum is None
    if n_coeffs_deriv is not None and len(n_coeffs_deriv) != len(pulses):
        raise ValueError(f'Expected n_coeffs_deriv for {len(pulses)} pulses, of shape (n_pulses, n_nops, n_ctrl, '
                         f'n_dt), not {len(n_coeffs_deriv)} entries.')
    ncd_of = [None if n_coeffs_deriv is None else n_coeffs_deriv[i] for i in range(len(pulses))]
    checked = [_validate(p, omega, control_identifiers, n_oper_identifiers, ncd_of[i], spectrum)
               for i, p in enumerate(pulses)]
    c_idx_of, n_idx_of = [c[0] for c in checked], [c[1] for c in checked]
    eligible = [i for i, p in enumerate(pulses)
                if batchable_shape(dimension_of(p), len(n_idx_of[i]), len(c_idx_of[i]))]
    out = [None]*len(pulses)
    W = len(as_f64(omega))
    for members in group_members(pulses, eligible, c_idx_of, n_idx_of):
        if len(members) < 2:
            continue
        _diagonalize(pulses, members, omega)
        first = members[0]
        d, G = dimension_of(pulses[first]), len(pulses[first].dt)
        A, H = len(n_idx_of[first]), len(c_idx_of[first])
        for chunk in split_group(members, W, A, H, G, d, want_dF):
            values = _run_pass(pulses, chunk, c_idx_of[first], n_idx_of[first],
                               None if n_coeffs_deriv is None else ncd_of, checked[first][2], want_dF)
            for j, i in enumerate(chunk):
                out[i] = values[j]
    for i, pulse in enumerate(pulses):
        if out[i] is None:
            out[i] = (gradient.filter_function_derivative(pulse, omega, control_identifiers, n_oper_identifiers,
                                                          ncd_of[i]) if want_dF else
                      gradient.infidelity_derivative(pulse, spectrum, omega, control_identifiers, n_oper_identifiers,
                                                     ncd_of[i]))
    shapes = {np.shape(v) for v in out}
    if len(shapes) > 1:
        raise ValueError(f'Every pulse must give the same output shape, got derivatives of shapes {sorted(shapes)}.')
    return np.stack(out)


def infidelity_derivatives(pulses, spectrum, omega, control_identifiers=None, n_oper_identifiers=None,
                           n_coeffs_deriv=None):
    r"""Derivatives of the entanglement infidelities of many pulses by their control amplitudes, shape
    ``(n_pulses, n_nops, n_dt, n_ctrl)``: ``np.stack([gradient.infidelity_derivative(p, spectrum, omega,
    control_identifiers, n_oper_identifiers, n_coeffs_deriv[i]) for i, p in enumerate(pulses)])``.

    *n_coeffs_deriv* is None or array-like of shape ``(n_pulses, n_nops, n_ctrl, n_dt)``.  Pulses of dimension 2 to
    4 with at most 4 selected noise and 8 selected control operators are grouped by (dimension, segments, selected
    indices) and each group of two or more runs in batched passes; the filter-function derivative is never stored.
    Everything else runs the single function inside the call, and the exceptions are those of the loop.  Pulses of a
    batched group that are not diagonalised yet are diagonalised in a batched pass as well and end up with the
    deferred control matrix of ``ff.get_filter_functions`` (see the module's docstring: call ``ff.infidelities``
    first, then this).  Every pulse must give the same output shape (else ValueError); an empty list gives an empty
    float array.
    """
    pulses = list(pulses)
    if not pulses:
        return np.empty((0,), dtype=np.float64)
    return _derivatives(pulses, omega, control_identifiers, n_oper_identifiers, n_coeffs_deriv, np.asarray(spectrum))


def filter_function_derivatives(pulses, omega, control_identifiers=None, n_oper_identifiers=None,
                                n_coeffs_deriv=None):
    r"""Derivatives of the fidelity filter functions of many pulses by their control amplitudes, shape
    ``(n_pulses, n_nops, n_dt, n_ctrl, n_omega)``: ``np.stack([gradient.filter_function_derivative(p, omega,
    control_identifiers, n_oper_identifiers, n_coeffs_deriv[i]) for i, p in enumerate(pulses)])``.  Routing,
    eigensystems and exceptions as for :func:`infidelity_derivatives`."""
    pulses = list(pulses)
    if not pulses:
        return np.empty((0,), dtype=np.float64)
    return _derivatives(pulses, omega, control_identifiers, n_oper_identifiers, n_coeffs_deriv, None)

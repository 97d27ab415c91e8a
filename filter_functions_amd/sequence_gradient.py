"""Infidelity gradients of many gate sequences given as index arrays into one gate set
(``ffk_sequence_infidelity_derivatives``, include/ffk.h).

``ff.sequence_infidelity_derivatives(gates, sequences, spectrum, omega)`` and
``ff.sequence_filter_function_derivatives(gates, sequences, omega)`` are the loops

``[gradient.infidelity_derivative(ff.concatenate(np.asarray(gates, dtype=object)[s]), spectrum, omega, ...)
for s in sequences]``

and the same with ``gradient.filter_function_derivative``; ``ff.gate_infidelity_derivatives`` adds the slices of those
arrays that belong to one gate, over all its occurrences in all sequences, with a weight per sequence: the derivative
of the cost :math:`\\sum_p w_p \\mathcal I_p` by the gate's amplitudes that an optimiser of a gate set asks for.  Under
correlated noise the derivative by a gate's amplitudes depends on what stands before and behind the gate, which is
what the sequence tells and a per-gate gradient cannot.

On the batched route no ``PulseSequence`` is built for a sequence and nothing is diagonalised again: the kernels work
in the frame of the current position, in which one record per gate segment serves every position of every sequence
(``csrc/sequence_gradient.hip``), and nothing of the size of a sequence -- least of all the running sums of the
interaction-picture noise operators, (sum of G, A, d, d, W) on the single path -- is ever formed.
"""
import numpy as np

from . import _lib, batch, batch_gradient, gradient, util
from ._gate_table import validated
from ._lib import as_c128, as_f64, check, ptr
from .sequences import pack_sequences

__all__ = ['sequence_infidelity_derivatives', 'sequence_filter_function_derivatives', 'gate_infidelity_derivatives']

#: Sequences per pass at most (the sequence is a grid axis).
MAX_SEQUENCES = 65535


def eligibility(gates, n_ctrl=None, n_nops=None):
    """What the batched route needs of the gate set, dict(d, H_all, A_all), or None if the loop's expression is to
    run.  *n_ctrl* and *n_nops*: how many control and noise operators are selected (default: all).

    Eligible: every gate has the same d in {2, 3, 4} and carries identical control and noise operators -- identifiers
    in identical order and equal arrays; sensitivities, amplitudes and the number of segments may differ from gate to
    gate --, both lists unique and in the sorted order ``ff.concatenate`` gives the new pulse (so that a sequence of one
    gate, which the loop copies, reads like every other); at most 4 noise and 8 control operators are selected."""
    if not gates:
        return None
    first = gates[0]
    d = batch_gradient.dimension_of(first)
    c_names = [str(i) for i in first.c_oper_identifiers]
    n_names = [str(i) for i in first.n_oper_identifiers]
    if c_names != sorted(set(c_names)) or n_names != sorted(set(n_names)):
        return None
    n_ctrl = len(c_names) if n_ctrl is None else n_ctrl
    n_nops = len(n_names) if n_nops is None else n_nops
    if not batch_gradient.batchable_shape(d, n_nops, n_ctrl):
        return None
    c_opers, n_opers = np.asarray(first.c_opers), np.asarray(first.n_opers)
    for g in gates[1:]:
        if batch_gradient.dimension_of(g) != d:
            return None
        if [str(i) for i in g.c_oper_identifiers] != c_names or [str(i) for i in g.n_oper_identifiers] != n_names:
            return None
        if not (np.array_equal(np.asarray(g.c_opers), c_opers) and np.array_equal(np.asarray(g.n_opers), n_opers)):
            return None
    return dict(d=d, H_all=len(c_names), A_all=len(n_names))


def padded_gate_set(gates, c_idx, n_idx):
    """The diagonalised gates as the arrays of one pass, every gate padded to the longest with segments of zero
    duration -- identity eigenvectors, the last propagator repeated, zero eigenvalues and sensitivities --, which
    contribute exact zeros and are never walked: dict(segments (T,) int32, D (T, G, d), V (T, G, d, d),
    Q (T, G + 1, d, d), s (T, A, G), dt (T, G), B (A, d, d), C (H, d, d))."""
    T, d = len(gates), batch_gradient.dimension_of(gates[0])
    segments = np.array([len(g.dt) for g in gates], dtype=np.int32)
    G, A = int(segments.max()), len(n_idx)
    D = np.zeros((T, G, d), dtype=np.float64)
    V = np.zeros((T, G, d, d), dtype=np.complex128)
    V[:] = np.eye(d)
    Q = np.empty((T, G + 1, d, d), dtype=np.complex128)
    s = np.zeros((T, A, G), dtype=np.float64)
    dt = np.zeros((T, G), dtype=np.float64)
    for k, g in enumerate(gates):
        n = segments[k]
        D[k, :n], V[k, :n], dt[k, :n] = g.eigvals, g.eigvecs, g.dt
        Q[k, :n + 1] = g.propagators
        Q[k, n + 1:] = Q[k, n]
        s[k, :, :n] = np.asarray(g.n_coeffs)[n_idx]
    return dict(segments=segments, D=D, V=V, Q=Q, s=s, dt=dt, B=as_c128(np.asarray(gates[0].n_opers)[n_idx]),
                C=as_c128(np.asarray(gates[0].c_opers)[c_idx]))


def occurrences(indices, n_gates):
    """Where every gate stands: (offsets (n_gates + 1) int32, sequence, position), the occurrences of gate k at
    ``offsets[k]:offsets[k + 1]``, sequence ascending, then position ascending -- the order of the sums of
    :func:`gate_infidelity_derivatives`.  *indices*: int32 arrays in [0, n_gates) (negative indices already wrapped)."""
    gate = np.concatenate(indices)
    sequence = np.repeat(np.arange(len(indices), dtype=np.int32), [len(i) for i in indices])
    position = np.concatenate([np.arange(len(i), dtype=np.int32) for i in indices])
    order = np.argsort(gate, kind='stable')
    offsets = np.zeros(n_gates + 1, dtype=np.int32)
    np.cumsum(np.bincount(gate, minlength=n_gates), out=offsets[1:])
    return offsets, np.ascontiguousarray(sequence[order]), np.ascontiguousarray(position[order])


def sequence_bytes(n_gates, G, W, A, H, d, want_dF, most_segments, longest):
    """(device bytes a sequence adds to a pass at most, bytes of a pass that do not depend on its sequences)."""
    query = _lib.load().ffk_sequence_infidelity_derivatives_workspace_bytes
    one, two = (query(n_gates, G, 1, 1, n, W, A, H, d, int(want_dF)) for n in (1, 2))
    return (two - one)*most_segments + 32*longest + 64, one


def split_sequences(members, n_gates, G, W, A, H, d, want_dF, most_segments, longest, budget=None):
    """*members* in consecutive passes under ``batch.PASS_BYTES`` (at least two sequences each) and of at most
    :data:`MAX_SEQUENCES` sequences."""
    budget = batch.PASS_BYTES if budget is None else budget
    per_sequence, fixed = sequence_bytes(n_gates, G, W, A, H, d, want_dF, most_segments, longest)
    return batch.split_passes(members, per_sequence, max(2*per_sequence, budget - fixed), MAX_SEQUENCES)


def _run_pass(arrays, indices, omega, d, S, want, weights=None, gate_sums=None):
    """One call of ``ffk_sequence_infidelity_derivatives`` over the sequences *indices*.  *want* 'dF' or 'dI': the
    list of the sequences' arrays (A, G_p, H[, W]); 'gate': adds to *gate_sums* (T, A, G, H) in place."""
    T, G = arrays['dt'].shape
    A, H, W, P = len(arrays['B']), len(arrays['C']), len(omega), len(indices)
    offsets, index, _ = pack_sequences(indices)
    lengths = np.array([arrays['segments'][i].sum() for i in indices], dtype=np.int64)
    dF = np.empty((int(lengths.sum())*A*H, W), dtype=np.float64) if want == 'dF' else None
    dI = np.empty(int(lengths.sum())*A*H, dtype=np.float64) if want == 'dI' else None
    occ = (None, None, None)
    if want == 'gate':
        occ = occurrences(indices, T)
        weights = as_f64(weights)
    check(_lib.load().ffk_sequence_infidelity_derivatives(
        T, G, ptr(arrays['segments']), ptr(arrays['D']), ptr(arrays['V']), ptr(arrays['Q']), ptr(arrays['B']), A,
        ptr(arrays['s']), ptr(arrays['C']), H, ptr(arrays['dt']), d, ptr(offsets), ptr(index), P, ptr(omega), W,
        ptr(S), S.ndim if S is not None else 0, ptr(occ[0]), ptr(occ[1]), ptr(occ[2]),
        ptr(weights) if want == 'gate' else None, ptr(dF), ptr(dI), ptr(gate_sums) if want == 'gate' else None))
    if want == 'gate':
        return None
    flat = dF if want == 'dF' else dI
    bounds = np.concatenate(([0], np.cumsum(lengths)))*A*H
    tail = (W,) if want == 'dF' else ()
    return [flat[bounds[p]:bounds[p + 1]].reshape((A, int(lengths[p]), H) + tail) for p in range(P)]


def _concatenated(gates, sequence):
    """The loop's pulse of one sequence."""
    import filter_functions_amd as ff         # (the public names, as a caller's loop reads them)
    table = np.empty(len(gates), dtype=object)
    table[:] = gates
    return ff.concatenate(table[sequence])


def _single(gates, sequence, spectrum, omega, control_identifiers, n_oper_identifiers):
    """The loop's expression for one sequence."""
    pulse = _concatenated(gates, sequence)
    if spectrum is None:
        return gradient.filter_function_derivative(pulse, omega, control_identifiers, n_oper_identifiers)
    return gradient.infidelity_derivative(pulse, spectrum, omega, control_identifiers, n_oper_identifiers)


def _plan(gates, spectrum, omega, control_identifiers, n_oper_identifiers):
    """Routing, once per call: dict(d, c_idx, n_idx, S) for the batched route, or None -- also where the loop is to
    raise its own exception (identifiers nobody carries, a spectrum that does not fit)."""
    try:
        c_idx = util.get_indices_from_identifiers(gates[0].c_oper_identifiers, control_identifiers)
        n_idx = util.get_indices_from_identifiers(gates[0].n_oper_identifiers, n_oper_identifiers)
    except ValueError:
        return None
    route = eligibility(gates, len(c_idx), len(n_idx))
    if route is None:
        return None
    S = None
    if spectrum is not None:
        # the checks of batch_gradient._validate, without touching a gate
        try:
            S = util.parse_spectrum(spectrum, as_f64(omega), range(route['A_all']))
        except ValueError:
            return None
        if S.ndim == 3 or (S.ndim == 2 and len(n_idx) != route['A_all']):
            return None
        if np.iscomplexobj(S):
            if np.any(np.imag(S) != 0):
                return None
            S = np.real(S)
        S = as_c128(S)
    return dict(d=route['d'], c_idx=c_idx, n_idx=n_idx, S=S)


def _gate_arrays(gates, plan, omega):
    """Diagonalises what is not (as ``ff.infidelity_derivatives`` does) and packs the gate set."""
    batch_gradient._diagonalize(gates, list(range(len(gates))), omega)
    return padded_gate_set(gates, plan['c_idx'], plan['n_idx'])


def _passes(arrays, indices, plan, omega, want_dF):
    T, G = arrays['dt'].shape
    A, H = len(arrays['B']), len(arrays['C'])
    most = max(int(arrays['segments'][i].sum()) for i in indices)
    longest = max(len(i) for i in indices)
    return split_sequences(list(range(len(indices))), T, G, len(omega), A, H, plan['d'], want_dF, most, longest)


def _derivatives(gates, sequences, spectrum, omega, control_identifiers, n_oper_identifiers):
    gates, indices = validated(gates, sequences)
    plan = _plan(gates, spectrum, omega, control_identifiers, n_oper_identifiers)
    if plan is None:
        return [_single(gates, i, spectrum, omega, control_identifiers, n_oper_identifiers) for i in indices]
    want_dF = spectrum is None
    omega_f = as_f64(omega)
    arrays = _gate_arrays(gates, plan, omega)
    out = [None]*len(indices)
    for chunk in _passes(arrays, indices, plan, omega_f, want_dF):
        values = _run_pass(arrays, [indices[i] for i in chunk], omega_f, plan['d'], plan['S'],
                           'dF' if want_dF else 'dI')
        for i, value in zip(chunk, values):
            out[i] = value
    # the members whose result is not finite: what the loop does
    for i, value in enumerate(out):
        if not np.isfinite(value).all():
            out[i] = _single(gates, indices[i], spectrum, omega, control_identifiers, n_oper_identifiers)
    return out


_SHARED = r"""

    *gates* is a sequence of T ``PulseSequence`` objects, *sequences* a list of P one-dimensional integer arrays of
    indices into it, read as :func:`ff.sequence_infidelities <filter_functions_amd.sequence_infidelities.
    sequence_infidelities>` reads them (negative indices wrap, others out of range raise IndexError, an empty sequence
    ValueError, an index that is no integer TypeError).  G_p is the number of segments of the concatenated sequence.
    Values, axis order and exceptions -- a spectrum that does not fit, a spectrum of three dimensions, unknown
    identifiers -- are the loop's.  ``n_coeffs_deriv`` is not offered.

    Routing, once per call.  The batched route takes a gate set in which every gate has the same d in {2, 3, 4} and
    identical control and noise operators (arrays and identifiers, both in sorted order; sensitivities, amplitudes and
    the number of segments may differ from gate to gate), with at most 4 noise and 8 control operators selected, under
    a real spectrum of one or two dimensions.  Gates that are not diagonalised are diagonalised as
    ``ff.infidelity_derivatives`` does it; otherwise no ``PulseSequence`` is built and no gate's cache is touched.  A
    pass is one H2D copy, a fixed number of launches whatever P and one D2H copy; passes are split under
    ``batch.PASS_BYTES``.  A sequence's result is the same bits alone or among others, at any place and in any pass
    split.  Everything else, and every sequence whose result is not finite, evaluates the loop's expression inside the
    call."""


def sequence_infidelity_derivatives(gates, sequences, spectrum, omega, control_identifiers=None,
                                    n_oper_identifiers=None):
    r"""Derivatives of the entanglement infidelities of many gate sequences by the control amplitudes of every segment
    that stands in them: a list of P arrays, array p of shape ``(n_idx, G_p, n_ctrl)``,

    ``[gradient.infidelity_derivative(ff.concatenate(np.asarray(gates, dtype=object)[s]), spectrum, omega,
    control_identifiers, n_oper_identifiers) for s in sequences]``."""
    return _derivatives(gates, sequences, np.asarray(spectrum), omega, control_identifiers, n_oper_identifiers)


def sequence_filter_function_derivatives(gates, sequences, omega, control_identifiers=None, n_oper_identifiers=None):
    r"""Derivatives of the fidelity filter functions of many gate sequences by the control amplitudes of every segment
    that stands in them: a list of P arrays, array p of shape ``(n_idx, G_p, n_ctrl, n_omega)``,

    ``[gradient.filter_function_derivative(ff.concatenate(np.asarray(gates, dtype=object)[s]), omega,
    control_identifiers, n_oper_identifiers) for s in sequences]``."""
    return _derivatives(gates, sequences, None, omega, control_identifiers, n_oper_identifiers)


def scatter_to_gates(gates, indices, derivatives, weights):
    """The sums of :func:`gate_infidelity_derivatives` on the host, from the sequences' arrays: sequence ascending,
    then position ascending, ``acc += w[p]*value``.  The sequences must agree in their noise and control operators
    (on the loop's route a sequence over gates with unequal operators carries the merged tables of its own gates):
    else ValueError."""
    shapes = {np.shape(v)[:1] + np.shape(v)[2:] for v in derivatives}
    if len(shapes) > 1:
        raise ValueError('Every sequence must give derivatives by the same operators for a sum per gate, got '
                         f'(n_nops, n_ctrl) = {sorted(shapes)}.')
    out = [np.zeros(np.shape(derivatives[0])[:1] + (len(g.dt),) + np.shape(derivatives[0])[2:]) for g in gates]
    for p, (sequence, values) in enumerate(zip(indices, derivatives)):
        at = 0
        for k in sequence:
            n = len(gates[k].dt)
            out[k] += weights[p]*values[:, at:at + n]
            at += n
    return out


def gate_infidelity_derivatives(gates, sequences, spectrum, omega, weights=None, control_identifiers=None,
                                n_oper_identifiers=None):
    r"""Derivatives of the cost :math:`\sum_p w_p \mathcal I_p` over many gate sequences by the control amplitudes of
    every GATE: a list of T arrays, array k of shape ``(n_idx, G_k, n_ctrl)``, the sum over the sequences p and the
    positions g at which gate k stands, :math:`\sum_p w_p \sum_{g: s_p[g] = k}`, of the slice of
    :func:`sequence_infidelity_derivatives`'s array p that belongs to position g.  A gate that stands nowhere gets
    zeros.  *weights* has shape (P,); None means ones.

    On the batched route the sums run on the device in a fixed order -- sequence ascending, then position ascending,
    one thread per entry over an occurrence list built on the host, no atomics -- and the sequences' derivatives are
    not copied to the host.  If the result is not finite, and on every other route, the sums are taken on the host
    over the loop's arrays in the same order."""
    gates, indices = validated(gates, sequences)
    weights = np.ones(len(indices)) if weights is None else np.asarray(weights, dtype=np.float64)
    if weights.shape != (len(indices),):
        raise ValueError(f'Expected weights of shape {(len(indices),)}, not {weights.shape}.')
    spectrum = np.asarray(spectrum)
    plan = _plan(gates, spectrum, omega, control_identifiers, n_oper_identifiers)
    if plan is not None:
        omega_f = as_f64(omega)
        arrays = _gate_arrays(gates, plan, omega)
        T, G = arrays['dt'].shape
        sums = np.zeros((T, len(arrays['B']), G, len(arrays['C'])), dtype=np.float64)
        for chunk in _passes(arrays, indices, plan, omega_f, False):
            _run_pass(arrays, [indices[i] for i in chunk], omega_f, plan['d'], plan['S'], 'gate',
                      weights[chunk[0]:chunk[-1] + 1], sums)
        if np.isfinite(sums).all():
            return [sums[k, :, :n].copy() for k, n in enumerate(arrays['segments'])]
    loop = [_single(gates, i, spectrum, omega, control_identifiers, n_oper_identifiers) for i in indices]
    return scatter_to_gates(gates, indices, loop, weights)


for _function in (sequence_infidelity_derivatives, sequence_filter_function_derivatives):
    _function.__doc__ += _SHARED
gate_infidelity_derivatives.__doc__ += _SHARED.replace('Values, axis order and exceptions', 'Axis order and exceptions')
del _function

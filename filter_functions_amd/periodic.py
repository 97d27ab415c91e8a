"""Periodic driving: many pulses at many repeat counts in one pass (``ffk_resident_periodic``, include/ffk.h).

``ff.periodic_filter_functions(pulses, repeats, omega)``, ``ff.periodic_infidelities(pulses, repeats, S, omega)`` and
``ff.periodic_decay_amplitudes(pulses, repeats, S, omega)`` are ``np.stack`` over the pulses and the repeat counts of
``ff.concatenate_periodic(p, n)`` followed by ``get_filter_function`` (its diagonal), ``ff.infidelity`` and
``numeric.calculate_decay_amplitudes``.  No ``PulseSequence`` is built for a result and nothing is tiled: with the
total propagator of one period U = V diag(exp(i phi)) V^dag, the control matrix of n periods is, in U's eigenbasis,
that of one period times ``sum_{g<n} exp(i g theta_jk)``, ``theta_jk = omega T - (phi_j - phi_k)``, so that the repeat
count is the argument of a sine.  The eigensystems -- P problems of d <= 4 -- are solved on
the host through the complex Schur form, which yields a unitary V also where eigenphases coincide.
"""
import ctypes

import numpy as np
from scipy import linalg as sla

from . import _lib, batch, numeric, processes, util
from ._lib import as_c128, as_f64, check

__all__ = ['periodic_filter_functions', 'periodic_infidelities', 'periodic_decay_amplitudes']

#: Largest residue max|U - V diag(exp(i phi)) V^dag| with which a pulse takes the batched route.
MAX_RESIDUE = 1e-12
#: Pulses and repeat counts of one pass at most (both are grid axes).
MAX_MEMBERS = 65535
MAX_REPEATS = 65535

_STAGES = {'filter_function': 1, 'infidelity': 2, 'decay_amplitudes': 3}


def eigensystem(propagator):
    """(V, phi, residue) of a unitary *propagator*: U = V diag(exp(i phi)) V^dag with V unitary whatever phases
    coincide (the complex Schur form of a normal matrix is diagonal), phi = ``np.angle`` of the eigenvalues, and
    residue = max|U - V diag(exp(i phi)) V^dag| for the caller to judge (a U that is not normal leaves one)."""
    U = np.asarray(propagator, dtype=np.complex128)
    T, V = sla.schur(U, output='complex')
    phi = np.angle(np.diag(T))
    residue = np.abs(U - (V*np.exp(1j*phi)) @ V.conj().T).max()
    return V, phi, float(residue)


def phase_differences(propagator, V):
    """phi_j - phi_k (d, d, 2) as hi + lo of two doubles.  A repeat count n multiplies the error of a phase by n, so
    the phases are taken from the Rayleigh quotients v_j^dag U v_j -- for a normal matrix second order in the error
    of v_j -- evaluated in extended precision (``np.longdouble``; where that is the double, lo is 0)."""
    Ul, Vl = np.asarray(propagator, dtype=np.clongdouble), np.asarray(V, dtype=np.clongdouble)
    quotients = np.einsum('ij,ik,kj->j', Vl.conj(), Ul, Vl)
    phi = np.arctan2(quotients.imag, quotients.real)
    delta = phi[:, None] - phi[None, :]
    hi = delta.astype(np.float64)
    return np.stack([hi, (delta - hi).astype(np.float64)], axis=-1)


def _up(nbytes):
    return -(-nbytes//256)*256


def out_elements(stage, K, n_idx, W, N):
    """Doubles of one pulse's result."""
    return K*n_idx*(W if stage == 1 else (1 if stage == 2 else N*N))


def fixed_bytes(stage, K, A, N, W, d, n_idx, s_ndim):
    """Device bytes of a pass that do not grow with its members (``ffk_periodic_workspace_bytes`` without them)."""
    rows = 0 if stage == 1 else (1 if s_ndim == 1 else n_idx)
    return _up(8*W) + _up(16*N*d*d) + _up(4*K) + _up(4*n_idx) + 2*_up(16*rows*W) + 8*256


def member_bytes(stage, K, A, N, W, d, n_idx, host):
    """Device bytes one member adds to a pass at most: pointer, eigensystem, period, result and -- for a control
    matrix held as a host array (*host*) -- its row of the uploaded table."""
    return 8 + 16*d*d + 16*d*d + 8 + 8*out_elements(stage, K, n_idx, W, N) + (16*A*N*W if host else 0)


def split_group(group, is_host, stage, K, A, N, W, d, n_idx, s_ndim, budget=None):
    """*group* in consecutive passes under ``batch.PASS_BYTES``, every member counted as the largest of the group."""
    budget = batch.PASS_BYTES if budget is None else budget
    per_member = member_bytes(stage, K, A, N, W, d, n_idx, any(is_host))
    room = max(per_member, budget - fixed_bytes(stage, K, A, N, W, d, n_idx, s_ndim))
    return batch.split_passes(group, per_member, room, MAX_MEMBERS)


def _eligible(pulse):
    """A shape and basis the kernels take: d = 2, 3, 4, a complete, Hermitian, traceless basis of d^2 elements, one
    to four noise operators."""
    N, A, d = processes.shape_of(pulse)
    basis = pulse.basis
    return (processes.batchable_shape(N, A, d) and N == d*d and bool(basis.istraceless) and bool(basis.isherm))


def _prepare(pulses, omega):
    """Eligible pulses whose control matrix is not known on the grid: ONE ``ff.get_filter_functions`` call."""
    from .pulse_sequence import _same_grid
    fresh = [p for p in pulses
             if _eligible(p) and ('control_matrix' not in p._frequency_data or not _same_grid(p.omega, omega))]
    if fresh:
        batch.get_filter_functions(fresh, omega)


def _run_pass(pulses, members, sources, systems, omega, repeats, spectrum, idx, stage):
    """One call of ``ffk_resident_periodic`` over ``pulses[i] for i in members``: the result (P, K, n_idx, ...)."""
    first = pulses[members[0]]
    N, A, d = processes.shape_of(first)
    P, W, K = len(members), len(omega), len(repeats)
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
    repeats = np.ascontiguousarray(repeats, dtype=np.int32)
    S = None if spectrum is None else as_c128(spectrum)
    n_idx = len(idx)
    shape = (P, K, n_idx) + ((W,) if stage == 1 else (() if stage == 2 else (N, N)))
    out = np.empty(shape, dtype=np.float64)
    check(_lib.load().ffk_resident_periodic(
        handles, slots.ctypes.data, None if table is None else table.ctypes.data, P, A, W, d, omega.ctypes.data,
        B.ctypes.data, V.ctypes.data, phi.ctypes.data, T.ctypes.data, repeats.ctypes.data, K,
        None if S is None else S.ctypes.data, 0 if S is None else S.ndim, idx.ctypes.data, n_idx, int(first.d),
        stage, out.ctypes.data))
    return out


def _single(stage, pulse, n, spectrum, omega, n_oper_identifiers):
    """The loop's expression for one pulse and one repeat count."""
    from .pulse_sequence import concatenate_periodic
    repeated = concatenate_periodic(pulse, n)
    if stage == 1:
        return np.einsum('aaw->aw', repeated.get_filter_function(omega)).real
    if stage == 2:
        return numeric.infidelity(repeated, spectrum, omega, n_oper_identifiers=n_oper_identifiers)
    return numeric.calculate_decay_amplitudes(repeated, spectrum, omega, n_oper_identifiers)


def _checked_repeats(repeats):
    counts = np.asarray(repeats)
    if counts.ndim != 1:
        raise ValueError(f'repeats should be one-dimensional, not of shape {counts.shape}.')
    if counts.size and not np.issubdtype(counts.dtype, np.integer):
        if not np.all(np.equal(np.mod(counts, 1), 0)):
            raise TypeError('repeats should be integers.')
    if counts.size and counts.min() < 1:
        raise ValueError('repeats must be a positive integer')
    if counts.size and counts.max() > np.iinfo(np.int32).max:
        raise ValueError('repeats beyond 2^31 - 1 are not supported.')
    return counts.astype(np.int32)


def _results(what, pulses, repeats, spectrum, omega, n_oper_identifiers):
    from .pulse_sequence import PulseSequence
    stage = _STAGES[what]
    pulses = list(pulses)
    for pulse in pulses:
        if not isinstance(pulse, PulseSequence):
            raise TypeError('Can only concatenate PulseSequences!')
    repeats = _checked_repeats(repeats)
    if not pulses:
        return np.empty((0,), dtype=np.float64)
    if stage == 1:
        idx_of = [np.arange(len(p.n_opers)) for p in pulses]
    else:
        idx_of = [util.get_indices_from_identifiers(p.n_oper_identifiers, n_oper_identifiers) for p in pulses]
        spectrum = np.asanyarray(spectrum)
    # (the basis elements are an axis of the decay amplitudes alone)
    shapes = {(len(idx),) + ((len(p.basis),) if stage == 3 else ()) for idx, p in zip(idx_of, pulses)}
    if len(shapes) > 1:
        raise ValueError('Every pulse must give the same output shape: the pulses have (selected noise operators'
                         f'[, basis elements]) = {sorted(shapes)}.')
    K, W = len(repeats), len(omega)
    out = [None]*len(pulses)
    # cross-spectra and spectra with an imaginary part: the loop (which also raises what a bad spectrum raises)
    batched = K > 0 and (stage == 1 or (spectrum.ndim <= 2 and W >= 2 and not (np.iscomplexobj(spectrum)
                                                                                and np.any(spectrum.imag))))
    if batched:
        _prepare(pulses, omega)
        sources, systems = {}, {}
        for i, pulse in enumerate(pulses):
            source = processes._source(pulse, omega, W) if _eligible(pulse) else None
            if source is None:
                continue
            V, phi, residue = eigensystem(pulse.total_propagator)
            if residue <= MAX_RESIDUE:
                sources[i], systems[i] = source, (V, phase_differences(pulse.total_propagator, V))
        for group in processes.group_members(pulses, sorted(sources), idx_of):
            first = pulses[group[0]]
            N, A, d = processes.shape_of(first)
            idx = idx_of[group[0]]
            parsed = None if stage == 1 else util.parse_spectrum(spectrum, as_f64(omega), np.asarray(idx))
            s_ndim = 0 if parsed is None else parsed.ndim
            is_host = [sources[i][0] == 'host' for i in group]
            for start in range(0, K, MAX_REPEATS):
                counts = repeats[start:start + MAX_REPEATS]
                for members in split_group(group, is_host, stage, len(counts), A, N, W, d, len(idx), s_ndim):
                    values = _run_pass(pulses, members, sources, systems, omega, counts, parsed, idx, stage)
                    for j, i in enumerate(members):
                        if out[i] is None:
                            out[i] = np.empty((K,) + values.shape[2:], dtype=np.float64)
                        out[i][start:start + len(counts)] = values[j]
        for i in sources:
            if not np.isfinite(out[i]).all():
                out[i] = None
    # everything else, and the members whose result is not finite: what the loop does
    for i, pulse in enumerate(pulses):
        if out[i] is None:
            rows = [_single(stage, pulse, int(n), spectrum, omega, n_oper_identifiers) for n in repeats]
            if not rows:
                one = _single(stage, pulse, 1, spectrum, omega, n_oper_identifiers)
                out[i] = np.empty((0,) + np.shape(one), dtype=np.float64)
            else:
                out[i] = np.stack(rows)
    return np.stack(out)


def periodic_filter_functions(pulses, repeats, omega):
    r"""Fidelity filter functions :math:`F_{\alpha\alpha}(\omega)` of *repeats[k]* periods of every pulse, shape
    (n_pulses, n_repeats, n_nops, n_omega), real: the diagonal over the noise operators of
    ``ff.concatenate_periodic(p, n).get_filter_function(omega)``, stacked over pulses and repeat counts.

    *repeats* is a one-dimensional array of integers >= 1 shared by all pulses (else ValueError; a non-pulse raises
    the TypeError of ``ff.concatenate_periodic``).  Routing, per pulse: d = 2, 3, 4 with a complete, Hermitian,
    traceless basis and one to four noise operators takes the batched route -- pulses whose control matrix is not
    known on the grid are completed first by ONE ``ff.get_filter_functions`` call, control matrices resident in HBM
    are read in place (deferred cache entries stay deferred), host arrays are uploaded once per pass, groups of one
    shape and basis are split under ``batch.PASS_BYTES``.  The number of launches does not grow with the number of
    pulses or repeat counts, and a result is the same bits whatever else the call holds.  Every other pulse, and a
    pulse whose propagator's eigensystem leaves a residue above ``MAX_RESIDUE``, runs the loop's expression inside
    the call: correct results, no speed-up.
    """
    return _results('filter_function', pulses, repeats, None, omega, None)


def periodic_infidelities(pulses, repeats, spectrum, omega, n_oper_identifiers=None):
    r"""Infidelities of *repeats[k]* periods of every pulse, shape (n_pulses, n_repeats, n_idx):
    ``ff.infidelity(ff.concatenate_periodic(p, n), spectrum, omega, n_oper_identifiers)`` stacked over pulses and
    repeat counts.  The filter functions never reach memory: the Fejer sums are integrated against the
    trapezoid-weighted spectrum where they are formed.  Routing as :func:`periodic_filter_functions`, for a real
    spectrum of one or two dimensions; cross-spectra (the result then has shape (n_pulses, n_repeats, n_idx, n_idx)),
    complex spectra and non-traceless bases run the loop's expression inside the call.  A bad spectrum or bad
    identifiers raise what ``ff.infidelity`` raises."""
    return _results('infidelity', pulses, repeats, spectrum, omega, n_oper_identifiers)


def periodic_decay_amplitudes(pulses, repeats, spectrum, omega, n_oper_identifiers=None):
    r"""Decay amplitudes :math:`\Gamma_{\alpha\alpha,kl}` of *repeats[k]* periods of every pulse, shape (n_pulses,
    n_repeats, n_idx, N, N): ``numeric.calculate_decay_amplitudes(ff.concatenate_periodic(p, n), spectrum, omega,
    n_oper_identifiers)`` stacked over pulses and repeat counts.  The Gram matrix over the frequencies is taken in
    the propagator's eigenbasis (d = 4: on the matrix cores) and rotated back once per result; the result is
    symmetric bit for bit.  Routing and exceptions as :func:`periodic_infidelities`."""
    return _results('decay_amplitudes', pulses, repeats, spectrum, omega, n_oper_identifiers)

"""Many gate sequences from one gate set in one pass (``ffk_concatenate_sequences_resident``, include/ffk.h).

``ff.concatenate_sequences(sequences)`` is the loop ``[ff.concatenate(s) for s in sequences]`` of randomized
benchmarking: many short sequences drawn from a few distinct gates.  Sequences whose filter function the loop would
compute by the table rule (every gate carries every noise operator, fidelity filter function, d = 2, Hermitian
basis) are grouped by frequency grid, basis and number of noise operators; every group runs in passes: one H2D copy
of the sequences (CSR), the gate table and the small inputs, one launch that forms the gates' phases, Liouville
propagators and every sequence's total propagator, one launch of the rule for all sequences, one D2H copy of the
total propagators and filter functions.  The control matrices stay in HBM behind
:class:`~filter_functions_amd._resident.Deferred` entries.  Every other sequence runs ``ff.concatenate``.
"""
import ctypes
import functools

import numpy as np

from . import _lib, util      # noqa: F401  (_lib: tools/time_sequences.py reads it here)
from ._lib import as_c128, as_f64, check
from ._resident import Deferred, ResidentHandle, ResidentResult, _view, spectrum_arguments
from .batch import MAX_PULSES, PASS_BYTES, _Member, split_passes

__all__ = ['concatenate_sequences']

#: The batched kernels' shapes: single-qubit gates, a basis of four elements, at most this many noise operators.
MAX_NOISE_OPERATORS = 4


class SequencePass(ResidentHandle):
    """Owns the ``ffk_resident`` handle of one sequence pass: the control matrices and filter functions of its
    sequences in HBM, the filter functions also in pinned host memory.  Shared by the resulting pulses, freed when
    the last of them lets go."""

    def evaluate(self, gates, slots, gate_table, propagators, tau, offsets, index, omega, basis, A):
        """One pass; returns (total propagators (P, 2, 2), F (P, A, A, W) viewing the handle's pinned memory)."""
        T, P = len(tau), len(offsets) - 1
        omega, basis = as_f64(omega), as_c128(basis)
        U, tau = as_c128(propagators), as_f64(tau)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        index = np.ascontiguousarray(index, dtype=np.int32)
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        handles = (ctypes.c_void_p*T)(*gates)
        table = None if gate_table is None else as_c128(gate_table)
        W, N, d = len(omega), len(basis), basis.shape[-1]
        total = np.empty((P, d, d), dtype=np.complex128)
        F_ptr = ctypes.c_void_p()
        check(self._lib.ffk_concatenate_sequences_resident(
            self._handle, handles, slots.ctypes.data, None if table is None else table.ctypes.data, U.ctypes.data,
            tau.ctypes.data, T, offsets.ctypes.data, index.ctypes.data, P, omega.ctypes.data, W, basis.ctypes.data,
            1, d, A, N, None, 0, 0, None, 0, 0, total.ctypes.data, ctypes.byref(F_ptr), None))
        self.shape = (P, W, N, A)
        F = _view(F_ptr.value, 2*P*A*A*W, np.complex128, (P, A, A, W), self)
        F.flags.writeable = False        # (as the single resident pass: a view of pinned memory integrated in place)
        return total, F

    def control_matrix(self, member):
        """Sequence *member*'s control matrix (n_nops, n_basis, n_omega), copied to the host now."""
        P, W, N, A = self.shape
        R = np.empty((A, N, W), dtype=np.complex128)
        check(self._lib.ffk_resident_batch_control_matrix(self._handle, int(member), R.ctypes.data))
        return R

    def infidelities(self, members, spectrum, idx, d):
        """Infidelities (len(members), n_idx[, n_idx]) on the members' resident filter functions, one launch;
        *spectrum* already validated (``util.parse_spectrum``)."""
        P, W, N, A = self.shape
        members = np.ascontiguousarray(members, dtype=np.int32)
        S, real, idx, out_shape = spectrum_arguments(spectrum, idx)
        out = np.empty((len(members),) + out_shape, dtype=np.float64)
        if W < 2:
            out[...] = 0.0
            return out
        for a in range(0, len(members), 65535):
            part = np.ascontiguousarray(members[a:a + 65535])
            check(self._lib.ffk_resident_batch_infidelity(self._handle, part.ctypes.data, len(part), S.ctypes.data,
                                                          S.ndim, real, idx.ctypes.data, len(idx), int(d),
                                                          out[a:a + 65535].ctypes.data))
        return out


class _SequenceMember:
    """``pulse._resident`` of a result of :func:`concatenate_sequences`: keeps the pass alive and integrates the
    member's resident filter function (``ff.infidelity`` through ``pulse.resident_infidelity``).  No ``shape``: a
    later ``ff.concatenate`` takes its array route; :func:`concatenate_sequences` reads the member in place."""
    __slots__ = ('batch', 'slot', '_filter_function')
    shape = None

    def __init__(self, batch, slot, filter_function):
        self.batch, self.slot, self._filter_function = batch, slot, filter_function

    @property
    def filter_function(self):
        return self._filter_function

    def infidelity(self, spectrum, idx, d):
        return self.batch.infidelities([self.slot], spectrum, idx, d)[0]

    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (type(None), ())


def resident_source(pulse, d, W, N, A):
    """(handle, slot) of the HBM copy of *pulse*'s control matrix of shape (A, N, W) -- slot -1: a single resident
    result; else the member of a batched or sequence pass --, or None (a host array, or nothing resident)."""
    res = pulse._resident
    if isinstance(res, ResidentResult) and res.shape is not None and res.shape[1:] == (d, W, N, A):
        return res.handle, -1
    if isinstance(res, _Member) and res.slot is not None and res.batch.shape is not None \
            and res.batch.shape[2:] == (d, W, N, A):
        return res.batch.handle, res.slot
    if isinstance(res, _SequenceMember) and d == 2 and res.batch.shape[1:] == (W, N, A):
        return res.batch.handle, res.slot
    return None


def _gate_source(gate, W, A):
    """(handle, slot) of the HBM copy of single-qubit *gate*'s control matrix, or None (a host array)."""
    return resident_source(gate, 2, W, 4, A)


def _plan(pulses, distinct, first, index, calc_filter_function, which, omega):
    """What the batched route needs of one validated sequence, or None if ``ff.concatenate`` is to run it (the
    decision logic of ``concatenate`` up to its table rule, pulse_sequence.py; raises what ``concatenate`` raises
    before that)."""
    from .pulse_sequence import _concatenate_distinct, _same_grid
    if len(pulses) < 2 or calc_filter_function is False or which != 'fidelity':
        return None
    newpulse, _, n_map = _concatenate_distinct(pulses, distinct, first, index)
    basis = newpulse.basis
    new_ids = [str(i) for i in newpulse.n_oper_identifiers]
    A = len(new_ids)
    if (newpulse.d != 2 or newpulse.c_opers.shape[-1] != 2 or len(basis) != 4 or not basis.isherm
            or not 1 <= A <= MAX_NOISE_OPERATORS):
        return None
    # every gate carries every noise operator, in the new pulse's order (the conditions of the single resident route)
    for k, gate in enumerate(distinct):
        mapping = n_map[int(first[k])]
        if len(gate.n_oper_identifiers) != A or [mapping.get(str(i)) for i in gate.n_oper_identifiers] != new_ids:
            return None
    if omega is None:
        cached_R = [g.is_cached('control_matrix') for g in distinct]
        cached_w = [g.is_cached('omega') for g in distinct]
        candidates = [g.omega for g, c in zip(distinct, cached_R if any(cached_R) else cached_w) if c]
        if not candidates or not all(_same_grid(candidates[0], w) for w in candidates[1:]):
            return None
        if calc_filter_function is None and not any(cached_R):
            return None
        omega = candidates[0]
    # every gate knows its control matrix on this grid and its total propagator: nothing is computed on a gate
    for gate in distinct:
        if (not gate.is_cached('control_matrix') or not _same_grid(gate.omega, omega)
                or 'total_propagator' not in gate._data):
            return None
    newpulse.omega = omega
    newpulse._defer_by_products()
    return dict(pulse=newpulse, distinct=distinct, index=index, omega=newpulse.omega, basis=basis, A=A)


def pack_sequences(indices):
    """CSR form of a list of index arrays: (offsets (P + 1), index (sum of lengths), order) with ``order`` the
    sequences sorted by length, longest first (stable), as the device deals them out."""
    lengths = np.array([len(i) for i in indices], dtype=np.int64)
    offsets = np.zeros(len(indices) + 1, dtype=np.int32)
    np.cumsum(lengths, out=offsets[1:])
    index = np.concatenate(indices).astype(np.int32) if indices else np.empty(0, dtype=np.int32)
    order = np.argsort(-lengths, kind='stable')
    return offsets, index, order


def group_plans(plans):
    """Indices into *plans* grouped by (frequency grid, basis, number of noise operators), each in input order."""
    from .pulse_sequence import _same_grid
    groups = []
    for i, plan in enumerate(plans):
        b = np.asarray(plan['basis'])
        for g in groups:
            ref = plans[g[0]]
            if (ref['A'] == plan['A'] and _same_grid(ref['omega'], plan['omega'])
                    and (ref['basis'] is plan['basis'] or np.array_equal(np.asarray(ref['basis']), b))):
                g.append(i)
                break
        else:
            groups.append([i])
    return groups


def pass_bytes(max_length, A, W, n_gates):
    """Device bytes one sequence adds to a pass at most: its control matrix and filter function, its positions, a
    share of the gate table (the table of a pass holds at most this sequence's own distinct gates more)."""
    return 16*A*(4 + A)*W + 8*max_length + 16*A*4*W*min(n_gates, max_length) + 64


def _run_pass(plans, members):
    """One pass over ``plans[i] for i in members``: fills the new pulses."""
    group = [plans[i] for i in members]
    first = group[0]
    omega, A = first['omega'], first['A']
    W = len(omega)
    slot_of, gates = {}, []
    for plan in group:
        for gate in plan['distinct']:
            if id(gate) not in slot_of:
                slot_of[id(gate)] = len(gates)
                gates.append(gate)
    from ._gate_table import staged_gates            # (which imports this module)
    handles, slots, gate_table, propagators, tau = staged_gates(gates, omega, 2, 4, A)
    indices = [np.array([slot_of[id(g)] for g in plan['distinct']], dtype=np.int32)[plan['index']] for plan in group]
    offsets, index, _ = pack_sequences(indices)
    batch = SequencePass()
    total, F = batch.evaluate(handles, slots, gate_table, propagators, tau, offsets, index, omega,
                              np.asarray(first['basis']), A)
    nbytes = 16*A*4*W
    for j, plan in enumerate(group):
        pulse, F_j = plan['pulse'], F[j]
        pulse.total_propagator = total[j]
        pulse._frequency_data['control_matrix'] = Deferred(functools.partial(batch.control_matrix, j), nbytes)
        pulse.cache_filter_function(omega, filter_function=F_j)
        pulse._resident = _SequenceMember(batch, j, F_j)


@util.parse_optional_parameters(which=('fidelity', 'generalized'))
def concatenate_sequences(sequences, calc_filter_function=None, which='fidelity', omega=None):
    r"""Concatenate many sequences of pulses: ``[ff.concatenate(s, calc_filter_function=calc_filter_function,
    which=which, omega=omega) for s in sequences]``, with the same results, caches and exceptions.

    A sequence whose filter function the loop computes by the table rule -- ``which='fidelity'``, every gate
    carrying every noise operator of the new pulse in its order, single-qubit gates (d = 2) in a Hermitian basis,
    at most four noise operators, every gate's control matrix and total propagator known on the grid -- takes the
    batched route: such sequences are grouped by frequency grid, basis and number of noise operators, and each
    group is evaluated in passes of one launch per stage for all its sequences.  Distinct gates are identified by
    object identity; a gate whose control matrix is resident in HBM (a single resident result, a member of an
    ``ff.get_filter_functions`` batch, a result of this function) is read in place.  Every other sequence runs
    ``ff.concatenate``.  Output in input order.
    """
    from .pulse_sequence import _validated_sequence, concatenate
    out, plans = [], []
    for sequence in sequences:
        pulses, distinct, first, index = _validated_sequence(sequence)
        plan = _plan(pulses, distinct, first, index, calc_filter_function, which, omega)
        if plan is None:
            out.append(concatenate(pulses, calc_filter_function=calc_filter_function, which=which, omega=omega))
        else:
            out.append(plan['pulse'])
            plans.append(plan)
    for members in group_plans(plans):
        first = plans[members[0]]
        longest = max(len(plans[i]['index']) for i in members)
        per_sequence = pass_bytes(longest, first['A'], len(first['omega']), len(first['distinct']))
        for chunk in split_passes(members, per_sequence, PASS_BYTES, MAX_PULSES):
            _run_pass(plans, chunk)
    return out

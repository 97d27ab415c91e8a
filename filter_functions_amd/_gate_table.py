"""The gate table behind the passes over many gate sequences (the leading arguments that
``ffk_concatenate_sequences_resident``, ``ffk_sequence_correlation_infidelities[4]``, ``ffk_sequence_infidelities``,
``ffk_sequence_processes`` and ``ffk_sequence_frequency_shifts`` share, include/ffk.h) and the front end of the
functions that take index arrays into one gate set: what they ask of gates and sequences, and how a gate set is routed.

Nothing here knows which pass it serves: spectra, further inputs, outputs and pass splitting stay with the callers.
"""
import ctypes

import numpy as np

from ._lib import as_c128
from .sequences import MAX_NOISE_OPERATORS, pack_sequences, resident_source


def index_arrays(sequences, n_gates):
    """The sequences as int32 arrays in [0, n_gates), with the rules of ``np.asarray(gates, dtype=object)[s]``:
    negative indices wrap, others out of range raise IndexError; an empty sequence raises ValueError, an index that
    is no integer TypeError."""
    out = []
    for p, s in enumerate(sequences):
        a = np.asarray(s)
        if a.ndim != 1:
            raise ValueError(f'Sequence {p}: expected a one-dimensional array of gate indices, not shape {a.shape}.')
        if a.size == 0:
            raise ValueError(f'Sequence {p} is empty.')
        if a.dtype.kind not in 'iu':
            raise TypeError(f'Sequence {p}: gate indices must be integers, not {a.dtype}.')
        bad = (a < -n_gates) | (a >= n_gates)
        if bad.any():
            raise IndexError(f'Sequence {p}: index {a[bad][0]} is out of bounds for {n_gates} gates.')
        out.append(np.where(a < 0, a + n_gates, a).astype(np.int32))
    return out


def eligibility(gates):
    """What the batched route needs of the gate set, dict(d, N, A, basis), or None if the loop's expression is to run.

    Eligible: all gates have d = 2 or all have d = 4; they share one basis (the same object, else equal arrays) that
    is Hermitian, traceless and has d^2 elements; they carry identical noise-operator identifiers in identical order
    with equal operator arrays, 1 to 4 of them, unique and in the sorted order ``ff.concatenate`` gives the new pulse
    (so that row a of the result means the same operator as in the loop).  Whether every gate knows its total
    propagator is checked by :func:`batched_plan`, after the control matrices are complete."""
    if not gates:
        return None
    first = gates[0]
    d, basis = first.d, first.basis
    if d not in (2, 4) or any(g.d != d or g.c_opers.shape[-1] != d for g in gates):
        return None
    if len(basis) != d*d or not basis.isherm or not basis.istraceless:
        return None
    reference = np.asarray(basis)
    for g in gates[1:]:
        if g.basis is not basis and not (np.shape(g.basis) == reference.shape
                                         and np.array_equal(np.asarray(g.basis), reference)):
            return None
    names = [str(i) for i in first.n_oper_identifiers]
    A = len(names)
    if not 1 <= A <= MAX_NOISE_OPERATORS or names != sorted(set(names)):
        return None
    n_opers = np.asarray(first.n_opers)
    for g in gates[1:]:
        if [str(i) for i in g.n_oper_identifiers] != names or not np.array_equal(np.asarray(g.n_opers), n_opers):
            return None
    return dict(d=d, N=len(basis), A=A, basis=basis)


def _on_grid(gate, omega):
    from .pulse_sequence import _same_grid
    return gate.is_cached('control_matrix') and _same_grid(gate.omega, omega)


def validated(gates, sequences):
    """(the gates as a list, the sequences as :func:`index_arrays`), with the exceptions of the loop: TypeError for a
    gate that is no ``PulseSequence``, ValueError if there is no sequence."""
    from .pulse_sequence import PulseSequence
    gates = list(gates)
    for gate in gates:
        if not isinstance(gate, PulseSequence):
            raise TypeError('Can only concatenate PulseSequences!')
    indices = index_arrays(sequences, len(gates))
    if not indices:
        raise ValueError('Need at least one sequence.')
    return gates, indices


def batched_plan(gates, omega):
    """Routing of a gate set, once per call: its :func:`eligibility`, or None.  Gates of an eligible set whose control
    matrix is not cached on *omega* are completed by ONE ``ff.get_filter_functions(missing, omega)`` call; a set in
    which a gate then does not know its total propagator is not eligible."""
    plan = eligibility(gates)
    if plan is None:
        return None
    missing = [g for g in gates if not _on_grid(g, omega)]
    if missing:
        from .batch import get_filter_functions
        get_filter_functions(missing, omega)
    if not all('total_propagator' in g._data for g in gates):
        return None
    return plan


def staged_gates(table_gates, omega, d, N, A):
    """What a pass needs of the gates of its table: (handles, slots, host table or None, total propagators, durations).
    A gate whose control matrix (A, N, W) is resident in HBM is named by its handle and slot (:func:`~sequences.
    resident_source`); the others' control matrices on *omega* are the rows of the host table, in table order."""
    sources = [resident_source(g, d, len(omega), N, A) for g in table_gates]
    host = [g for g, src in zip(table_gates, sources) if src is None]
    table = as_c128(np.array([g.get_control_matrix(omega) for g in host])) if host else None
    handles = (ctypes.c_void_p*len(table_gates))(*[None if src is None else src[0].value for src in sources])
    slots = np.array([-1 if src is None else src[1] for src in sources], dtype=np.int32)
    U = as_c128(np.array([g.total_propagator for g in table_gates]))
    tau = np.array([g.tau for g in table_gates], dtype=np.float64)
    return handles, slots, table, U, tau


class PassTable:
    """The table of one pass over the sequences *indices* (int32 arrays into *gates*) of a gate set routed by *plan*:
    only the gates the pass uses are in it, and the sequences are renumbered to index it (CSR ``offsets``, ``index``).
    ``used`` are the positions in *gates* of the table's ``gates``.  *extra* (optional): further int32 arrays into
    *gates*, one per sequence, whose gates the table holds as well; ``extra`` is then their concatenation, renumbered
    like ``index`` (else None)."""

    def __init__(self, gates, indices, plan, omega, extra=None):
        self.d, self.N, self.A = plan['d'], plan['N'], plan['A']
        self.used = np.unique(np.concatenate(list(indices) + list(extra or [])))
        slot_of = np.full(len(gates), -1, dtype=np.int32)
        slot_of[self.used] = np.arange(len(self.used), dtype=np.int32)
        self.gates = [gates[k] for k in self.used]
        self.handles, self.slots, self.table, self.U, self.tau = staged_gates(self.gates, omega, self.d, self.N, self.A)
        self.offsets, self.index, _ = pack_sequences([slot_of[i] for i in indices])
        self.extra = None if extra is None else np.ascontiguousarray(np.concatenate([slot_of[e] for e in extra]),
                                                                     dtype=np.int32)
        self.omega = omega
        self.basis = as_c128(np.asarray(plan['basis']))

    def c_arguments(self):
        """The sixteen leading arguments of the C entries, in order; the arrays live as long as this object."""
        return (self.handles, self.slots.ctypes.data, None if self.table is None else self.table.ctypes.data,
                self.U.ctypes.data, self.tau.ctypes.data, len(self.gates), self.offsets.ctypes.data,
                self.index.ctypes.data, len(self.offsets) - 1, self.omega.ctypes.data, len(self.omega),
                self.basis.ctypes.data, 1, self.d, self.A, self.N)

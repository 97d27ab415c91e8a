"""CPU-only: the workspace query and the argument checks of the sequence gradient pass
(ffk_sequence_infidelity_derivatives), the routing predicate, the padding of short gates, the occurrence lists of
ff.gate_infidelity_derivatives, the pass split of sequence_gradient.py, and the kernels' resources."""
import numpy as np
import pytest

import filter_functions_amd as ff
from filter_functions_amd import _lib, batch, sequence_gradient
from filter_functions_amd._lib import ptr
from test_kernel_resources import kernels  # noqa: F401  (the module's fixture)


def query(T=4, G=5, P=3, n_index=10, n_segments=30, W=70, A=2, H=2, d=3, want_dF=0):
    return _lib.load().ffk_sequence_infidelity_derivatives_workspace_bytes(T, G, P, n_index, n_segments, W, A, H, d,
                                                                           want_dF)


def test_the_names_are_exported():
    for name in ('sequence_infidelity_derivatives', 'sequence_filter_function_derivatives',
                 'gate_infidelity_derivatives', 'sequence_gradient'):
        assert name in ff.__all__ and hasattr(ff, name)
    for name in ('ffk_sequence_infidelity_derivatives', 'ffk_sequence_infidelity_derivatives_workspace_bytes'):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)


@pytest.mark.parametrize('want_dF', [0, 1])
def test_the_workspace_query_is_linear_in_the_walked_segments(want_dF):
    sizes = [query(n_segments=n, want_dF=want_dF) for n in (30, 60, 90, 3000)]
    assert sizes[0] > 0
    step = sizes[1] - sizes[0]
    assert step > 0 and sizes[2] - sizes[1] == step and sizes[3] - sizes[0] == 99*step
    A, H, W = 2, 2, 70
    # per segment: the rows of dF, or one partial per frequency tile and the result
    assert step == 30*8*A*H*(W if want_dF else -(-W//64) + 1)
    # ... and it covers the gate set: records, totals, eigensystems
    assert query(T=8) > query(T=4) and query(G=10) > query(G=5) and query(W=140) > query(W=70)


def test_the_workspace_query_is_zero_for_shapes_the_pass_does_not_take():
    assert query(d=5) == 0 and query(A=5) == 0 and query(H=9) == 0
    assert query(d=1) == 0 and query(W=0) == 0 and query(P=0) == 0 and query(P=65536) == 0
    assert query(d=2) > 0 and query(d=4, A=4, H=8) > 0


def call(T=2, G=2, segments=(2, 1), offsets=(0, 2, 3), index=(0, 1, 1), W=5, A=1, H=1, d=2, s_ndim=1, want='dI'):
    """The entry point on a tiny, well-formed gate set, with one thing wrong: nothing may reach the device."""
    segments = np.array(segments, dtype=np.int32)
    offsets, index = np.array(offsets, dtype=np.int32), np.array(index, dtype=np.int32)
    D = np.zeros((T, G, d))
    V = np.zeros((T, G, d, d), dtype=complex)
    V[:] = np.eye(d)
    Q = np.zeros((T, G + 1, d, d), dtype=complex)
    Q[:] = np.eye(d)
    B, C = np.zeros((A, d, d), dtype=complex), np.zeros((H, d, d), dtype=complex)
    s, dt = np.ones((T, A, G)), np.ones((T, G))
    omega = np.linspace(0.0, 1.0, max(W, 1))
    S = np.ones(max(W, 1), dtype=complex)
    out = np.zeros(64*max(W, 1))
    status = _lib.load().ffk_sequence_infidelity_derivatives(
        T, G, ptr(segments), ptr(D), ptr(V), ptr(Q), ptr(B), A, ptr(s), ptr(C), H, ptr(dt), d, ptr(offsets),
        ptr(index), len(offsets) - 1, ptr(omega), W, ptr(S), s_ndim, None, None, None, None,
        ptr(out) if want == 'dF' else None, ptr(out) if want == 'dI' else None, None)
    return status, _lib.load().ffk_last_error().decode()


@pytest.mark.parametrize('kw, fragment', [
    (dict(index=(0, 2, 1)), 'index[1] = 2 outside [0, 2)'),
    (dict(index=(0, 1, -1)), 'index[2] = -1 outside [0, 2)'),
    (dict(offsets=(0, 2, 2), index=(0, 1)), 'sequence 1 is empty'),
    (dict(W=0), 'empty axis: W=0'),
    (dict(s_ndim=3), 'needs a spectrum of shape (W,) or (A, W), not s_ndim=3'),
    (dict(d=5), 'support 2 <= d <= 4, not d=5'),
    (dict(A=5), 'A <= 4 noise and H <= 8 control operators, not A=5 H=1'),
    (dict(segments=(3, 1)), 'gate 0 has 3 segments, expected 1 to 2'),
    (dict(want=None), 'no output requested'),
])
def test_bad_arguments_are_refused_before_anything_touches_the_device(kw, fragment):
    status, message = call(**kw)
    assert status == _lib.FFK_EINVAL
    assert fragment in message, message


def operators(rng, d, n):
    M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
    return M + M.conj().transpose(0, 2, 1)


def gate(rng, c_opers, n_opers, G, d):
    return ff.PulseSequence(list(zip(c_opers, rng.standard_normal((len(c_opers), G)))),
                            list(zip(n_opers, rng.random((len(n_opers), G)) + 0.1)), rng.random(G) + 0.2,
                            ff.Basis.ggm(d))


def test_the_routing_predicate():
    rng = np.random.default_rng(1)
    d = 3
    C, B = operators(rng, d, 2), operators(rng, d, 2)
    gates = [gate(rng, C, B, G, d) for G in (1, 2, 5, 3)]
    assert sequence_gradient.eligibility(gates) == dict(d=3, H_all=2, A_all=2)      # equal operators, different G_k
    other = C.copy()
    other[1] = other[1] + np.diag([1.0, 0.0, -1.0])
    assert sequence_gradient.eligibility(gates + [gate(rng, other, B, 2, d)]) is None      # another control operator
    assert sequence_gradient.eligibility(gates + [gate(rng, C, B[::-1].copy(), 2, d)]) is None
    assert sequence_gradient.eligibility(gates + [gate(rng, C[:1], B, 2, d)]) is None
    assert sequence_gradient.eligibility(gates + [gate(rng, operators(rng, 2, 2), operators(rng, 2, 2), 2, 2)]) is None
    C5, B5 = operators(rng, 5, 2), operators(rng, 5, 2)
    assert sequence_gradient.eligibility([gate(rng, C5, B5, 2, 5) for _ in range(2)]) is None          # d = 5
    many = [gate(rng, operators(rng, 2, 9), operators(rng, 2, 5), 2, 2)]
    assert sequence_gradient.eligibility(many) is None
    assert sequence_gradient.eligibility(many, n_ctrl=8, n_nops=5) is None          # more than 4 noise operators
    assert sequence_gradient.eligibility(many, n_ctrl=9, n_nops=4) is None          # more than 8 control operators
    assert sequence_gradient.eligibility(many, n_ctrl=8, n_nops=4) == dict(d=2, H_all=9, A_all=5)
    assert sequence_gradient.eligibility([]) is None
    # identifiers that are not in the order ff.concatenate gives: a sequence of one gate would read otherwise
    named = ff.PulseSequence([[C[0], [1.0], 'b'], [C[1], [1.0], 'a']], [[B[0], [1.0]]], [1.0], ff.Basis.ggm(d))
    assert list(named.c_oper_identifiers) == ['a', 'b'] and sequence_gradient.eligibility([named]) is not None


def test_the_plan_sends_what_the_kernels_do_not_take_to_the_loop():
    rng = np.random.default_rng(2)
    d, W = 2, 9
    gates = [gate(rng, operators(rng, d, 2), operators(rng, d, 2), 2, d)]
    omega = np.linspace(0.1, 1.0, W)
    plan = sequence_gradient._plan(gates, np.ones(W), omega, None, None)
    assert plan['d'] == 2 and plan['S'].dtype == np.complex128 and plan['S'].shape == (W,)
    assert sequence_gradient._plan(gates, None, omega, None, None)['S'] is None
    assert sequence_gradient._plan(gates, np.ones((2, W)), omega, None, None)['S'].shape == (2, W)
    assert sequence_gradient._plan(gates, np.ones(W)*(1 + 0j), omega, None, None) is not None     # no imaginary part
    for spectrum in (np.ones(W)*(1 + 1j), np.ones((2, 2, W)), np.ones(W + 1)):
        assert sequence_gradient._plan(gates, spectrum, omega, None, None) is None
    ids = gates[0].n_oper_identifiers
    assert sequence_gradient._plan(gates, np.ones((2, W)), omega, None, ids[:1]) is None
    assert sequence_gradient._plan(gates, np.ones(W), omega, ['nobody'], None) is None
    assert sequence_gradient._plan(gates, np.ones(W), omega, None, ids[::-1])['n_idx'].tolist() == [1, 0]
    assert not any(g.is_cached('eigvals') for g in gates) and gates[0].omega is None


def test_short_gates_are_padded_with_segments_of_zero_duration():
    rng = np.random.default_rng(3)
    d = 2
    C, B = operators(rng, d, 3), operators(rng, d, 2)
    gates = [gate(rng, C, B, G, d) for G in (1, 3, 2)]
    for k, g in enumerate(gates):        # (stand-ins for the eigensystems: the padding only copies them)
        G = len(g.dt)
        g.eigvals, g.eigvecs = rng.random((G, d)), operators(rng, d, G)
        g.propagators = operators(rng, d, G + 1)
    arrays = sequence_gradient.padded_gate_set(gates, np.array([2, 0]), np.array([1]))
    assert arrays['segments'].tolist() == [1, 3, 2] and arrays['segments'].dtype == np.int32
    assert arrays['D'].shape == (3, 3, d) and arrays['V'].shape == (3, 3, d, d) and arrays['Q'].shape == (3, 4, d, d)
    assert arrays['s'].shape == (3, 1, 3) and arrays['dt'].shape == (3, 3)
    assert np.array_equal(arrays['B'], B[[1]]) and np.array_equal(arrays['C'], C[[2, 0]])
    for k, g in enumerate(gates):
        G = len(g.dt)
        assert np.array_equal(arrays['D'][k, :G], g.eigvals) and not arrays['D'][k, G:].any()
        assert np.array_equal(arrays['V'][k, :G], g.eigvecs)
        assert np.array_equal(arrays['V'][k, G:], np.broadcast_to(np.eye(d), (3 - G, d, d)))
        assert np.array_equal(arrays['Q'][k, :G + 1], g.propagators)
        assert np.array_equal(arrays['Q'][k, G + 1:], np.broadcast_to(g.propagators[G], (3 - G, d, d)))
        assert np.array_equal(arrays['s'][k, 0, :G], g.n_coeffs[1]) and not arrays['s'][k, :, G:].any()
        assert np.array_equal(arrays['dt'][k, :G], g.dt) and not arrays['dt'][k, G:].any()
    for key in ('D', 'V', 'Q', 's', 'dt', 'B', 'C', 'segments'):
        assert arrays[key].flags.c_contiguous, key


def test_the_occurrence_lists():
    from filter_functions_amd._gate_table import index_arrays
    indices = index_arrays([[0, 2, 0], [-1, 1], [2], [-4, -2, 0, 2]], 4)       # negative indices wrap
    assert [i.tolist() for i in indices] == [[0, 2, 0], [3, 1], [2], [0, 2, 0, 2]]
    offsets, sequence, position = sequence_gradient.occurrences(indices, 5)
    assert offsets.dtype == sequence.dtype == position.dtype == np.int32
    assert offsets.tolist() == [0, 4, 5, 9, 10, 10]                          # (gate 4 stands nowhere)
    listed = list(zip(sequence.tolist(), position.tolist()))
    assert listed[0:4] == [(0, 0), (0, 2), (3, 0), (3, 2)]                   # sequence ascending, then position
    assert listed[4:5] == [(1, 1)]
    assert listed[5:9] == [(0, 1), (2, 0), (3, 1), (3, 3)]
    assert listed[9:10] == [(1, 0)]
    for k in range(5):
        for p, g in listed[offsets[k]:offsets[k + 1]]:
            assert indices[p][g] == k


def test_the_host_scatter_adds_in_the_documented_order():
    class Gate:
        def __init__(self, G):
            self.dt = np.ones(G)
    gates = [Gate(1), Gate(2)]
    indices = [np.array([1, 0, 1]), np.array([0])]
    values = [np.arange(2*5*3, dtype=float).reshape(2, 5, 3), 100 + np.arange(2*1*3, dtype=float).reshape(2, 1, 3)]
    out = sequence_gradient.scatter_to_gates(gates, indices, values, [2.0, -1.0])
    assert out[0].shape == (2, 1, 3) and out[1].shape == (2, 2, 3)
    assert np.array_equal(out[0], 2.0*values[0][:, 2:3] - values[1])
    assert np.array_equal(out[1], 2.0*values[0][:, 0:2] + 2.0*values[0][:, 3:5])


def test_the_pass_split(monkeypatch):
    T, G, W, A, H, d = 4, 5, 70, 2, 2, 3
    for want_dF in (False, True):
        per, fixed = sequence_gradient.sequence_bytes(T, G, W, A, H, d, want_dF, 40, 12)
        assert per >= 40*8*A*H*(W if want_dF else 3) and fixed > 0
        members = list(range(21))
        assert sequence_gradient.split_sequences(members, T, G, W, A, H, d, want_dF, 40, 12) == [members]
        monkeypatch.setattr(batch, 'PASS_BYTES', fixed + 5*per)
        parts = sequence_gradient.split_sequences(members, T, G, W, A, H, d, want_dF, 40, 12)
        assert len(parts) >= 4 and sum(parts, []) == members
        assert all(2 <= len(part) <= 5 for part in parts)
        # every pass fits the budget it was cut for
        for part in parts:
            assert query(T, G, len(part), 12*len(part), 40*len(part), W, A, H, d, int(want_dF)) <= fixed + 5*per
        monkeypatch.setattr(batch, 'PASS_BYTES', 1)             # (never fewer than two sequences a pass)
        assert all(len(part) <= 2 for part in
                   sequence_gradient.split_sequences(members, T, G, W, A, H, d, want_dF, 40, 12))
        monkeypatch.undo()


def test_the_walk_kernel_has_three_instantiations_without_private_memory(kernels):  # noqa: F811
    """sequence_gradient_walk_kernel<D> for D = 2, 3, 4 holds what grad_batch_kernel<D> holds -- the conjugate total
    and the running sum of one noise operator in registers, the integrals in per-lane LDS columns."""
    found = {name: k for name, k in kernels.items() if 'sequence_gradient_walk_kernel' in name}
    assert len(found) == 3, sorted(found)
    for D in (2, 3, 4):
        assert sum(f'ILi{D}E' in name for name in found) == 1, (D, sorted(found))
    found.update({name: k for name, k in kernels.items() if 'sequence_gradient_gather_kernel' in name})
    assert len(found) == 4
    for name, k in found.items():
        assert k['.private_segment_fixed_size'] == 0, name
        assert k['.vgpr_spill_count'] == 0, name
        assert k['.max_flat_workgroup_size'] == 64, name
        assert k['.vgpr_count'] + k['.agpr_count'] <= 512, (name, k['.vgpr_count'], k['.agpr_count'])

"""CPU side of ff.correlation_infidelities: which sequences take the batched route, the ragged output's offsets and
the order of the results after pass splitting, the byte account of a pass, and the workspace query without a GPU."""
import numpy as np
import pytest

import filter_functions_amd as ff
from filter_functions_amd import _lib, batch, correlations
from filter_functions_amd.pulse_sequence import _validated_sequence
from test_sequences_host import cached, gate, plan_of


def batched(seq, spectrum, omega=None, n_oper_identifiers=None):
    return correlations._batched_plan(*_validated_sequence(seq), spectrum, omega, n_oper_identifiers)


def test_eligibility():
    omega = np.linspace(0.1, 1.0, 5)
    S = 1/omega
    a, b = cached(gate(), omega), cached(gate(), omega)
    plan = batched([a, b, a], S)
    assert plan is not None and list(plan['index']) == [0, 1, 0] and plan['idx'].tolist() == [0]
    assert plan['spectrum'].dtype == np.float64 and plan['spectrum'].shape == (5,)
    # what _plan rejects is rejected
    other = cached(gate(), np.linspace(0.1, 2.0, 5))
    missing = cached(gate(noise=('Z',)), omega)
    plain = gate()
    for seq, kw in (([a, other], {}), ([a, missing], {}), ([plain, plain], {}),
                    ([a, b], dict(omega=np.linspace(0.1, 3.0, 5)))):
        assert plan_of(seq, calc_filter_function=True, **kw) is None
        assert batched(seq, S, **kw) is None
    assert batched([a], S) is None                                      # length 1 follows the loop
    d4 = cached(gate(d=4), omega)
    assert batched([d4, d4], S) is None                                 # d = 4: the loop
    assert correlations.MAX_LENGTH == 256
    assert batched([a, b]*128, S) is not None                           # 256 positions are in
    assert batched([a, b]*128 + [a], S) is None                         # 257 are out
    two = cached(gate(noise=('X', 'Z')), omega)
    assert batched([two, two], np.ones((2, 2, 5))) is None              # cross-spectra: the loop
    assert batched([two, two], np.ones((2, 5)))['spectrum'].shape == (2, 5)
    assert batched([two, two], S, n_oper_identifiers=['Z', 'X'])['idx'].tolist() == [1, 0]
    assert batched([two, two], S, n_oper_identifiers=['Q']) is None     # the loop raises
    assert batched([two, two], np.ones(4)) is None                      # a spectrum of the wrong length: the loop raises
    assert batched([a, b], S*(1 + 0j))['spectrum'].dtype == np.float64
    assert batched([a, b], S*(1 + 1j)) is None                          # an imaginary part: the loop
    with pytest.raises(TypeError):
        ff.correlation_infidelities([[a, 3]], S)
    assert ff.correlation_infidelities([], S) == []


def test_grouping_also_by_selected_operators():
    omega = np.linspace(0.1, 1.0, 5)
    two = cached(gate(noise=('X', 'Z')), omega)
    one = cached(gate(), omega)
    S = 1/omega
    plans = [batched([two, two], S), batched([two, two], S, n_oper_identifiers=['Z']), batched([one, one], S),
             batched([two, two, two], S), batched([two, two], S, n_oper_identifiers=['Z'])]
    # (plan 2 has one noise operator: a group of its own although its idx equals nothing else's)
    assert correlations._group_by_idx(plans) == [[0, 3], [1, 4], [2]]


def test_output_offsets_and_order_after_splitting(monkeypatch):
    assert correlations.output_offsets([2, 1, 3]).tolist() == [0, 4, 5, 14]
    assert correlations.output_offsets([256]*40000).dtype == np.int64
    assert correlations.output_offsets([256]*40000)[-1] == 40000*65536            # past 2^31
    # ragged results come back in input order whatever the passes: a fake pass that returns each sequence's gates
    omega = np.linspace(0.1, 1.0, 5)
    gates = [cached(gate(), omega) for _ in range(3)]
    lengths = [2, 5, 3, 2, 4, 7, 2, 3, 6]
    seqs = [[gates[(k + j) % 3] for j in range(m)] for k, m in enumerate(lengths)]
    passes = []

    def fake_pass(plans, members):
        passes.append(list(members))
        return [np.full((len(plans[i]['index']),)*2 + (1,), float(i)) for i in members]
    monkeypatch.setattr(correlations, '_run_pass', fake_pass)
    monkeypatch.setattr(correlations, 'PASS_BYTES', 3*correlations.pass_bytes(7, 1, 5, 3, 1))
    got = ff.correlation_infidelities(seqs, 1/omega)
    assert passes == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    assert [g.shape for g in got] == [(m, m, 1) for m in lengths]
    assert [g[0, 0, 0] for g in got] == list(range(9))


def test_pass_bytes_cover_the_output_and_the_partials():
    for G, W, n_idx in ((2, 301, 1), (151, 301, 1), (256, 8192, 4), (100, 8192, 2)):
        per = correlations.pass_bytes(G, 4, W, 24, n_idx)
        assert per >= 8*G*G*n_idx*(1 + correlations.slabs(W))
    assert correlations.slabs(2) == 1 and correlations.slabs(301) == 19 and correlations.slabs(512) == 32
    assert correlations.slabs(513) == 17 and correlations.slabs(8192) == 32
    members = list(range(1050))
    # the study (1050 sequences of up to 152 gates at 301 frequencies), every sequence counted as the longest
    chunks = batch.split_passes(members, correlations.pass_bytes(152, 1, 301, 24, 1))
    assert sum(chunks, []) == members and 2 <= len(chunks) <= 8


def test_workspace_query_needs_no_gpu():
    query = _lib.load().ffk_sequence_correlation_infidelities_workspace_bytes
    base = query(24, 2, 20, 0, 2, 1, 4, 301, 1, 1)
    assert base > 8*20*20*(1 + correlations.slabs(301))
    assert query(24, 200, 218, 0, 2, 1, 4, 301, 1, 1) > query(24, 2, 218, 0, 2, 1, 4, 301, 1, 1)      # grows with P
    assert query(24, 2, 40, 0, 2, 1, 4, 301, 1, 1) > base                                            # ... and n_index
    assert query(24, 2, 20, 3, 2, 1, 4, 301, 1, 1) >= base + 3*16*4*301                              # host rows
    assert query(24, 2, 20, 0, 4, 1, 16, 301, 1, 1) == 0      # d = 4
    assert query(24, 2, 20, 0, 2, 5, 4, 301, 1, 1) == 0       # A = 5
    assert query(24, 2, 20, 0, 2, 1, 4, 301, 1, 3) == 0       # cross-spectra
    assert query(24, 2, 20, 0, 2, 1, 4, 301, 2, 1) == 0       # more selected operators than there are
    # the bound holds for the worst split of n_index positions into P sequences: one block of the arena per pass
    n_index, P = 300, 3
    worst = 256**2 + 43**2 + 1
    assert query(24, P, n_index, 0, 2, 1, 4, 301, 1, 1) >= 8*worst*(1 + correlations.slabs(301))


def test_binding_header_and_exports_agree():
    """test_abi's agreement, with the new entries in all three places."""
    import test_abi
    names = test_abi.header_symbols()
    for name in ('ffk_sequence_correlation_infidelities', 'ffk_sequence_correlation_infidelities_workspace_bytes'):
        assert name in names and name in _lib.SIGNATURES
    test_abi.test_library_exports_every_declared_symbol()
    test_abi.test_binding_table_matches_header()


def test_bad_arguments_are_refused_before_the_device():
    """NULL and all-zero arguments: FFK_EINVAL (the sweep of the sanitizer build's child, on the new entries)."""
    lib = _lib.load()
    res, args = _lib.SIGNATURES['ffk_sequence_correlation_infidelities']
    import ctypes
    assert lib.ffk_sequence_correlation_infidelities(*[None if a is ctypes.c_void_p else 0 for a in args]) \
        == _lib.FFK_EINVAL
    assert 'NULL' in lib.ffk_last_error().decode()

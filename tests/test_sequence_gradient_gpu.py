"""ff.sequence_infidelity_derivatives / ff.sequence_filter_function_derivatives / ff.gate_infidelity_derivatives
(sequence_gradient.py, csrc/sequence_gradient.hip) against the loop over ``gradient.infidelity_derivative`` on the
concatenated pulses, against finite differences of ``ff.sequence_infidelities``, and bit for bit against themselves.

test_against_the_loop prints the worst rel_err of every case (DESIGN.md 7.17 records them); the bar is 1e-10."""
import numpy as np
import pytest

import filter_functions_amd as ff
from conftest import rel_err
from filter_functions_amd import batch, gradient, sequence_gradient

pytestmark = pytest.mark.gpu

TOL = 1e-10          # TOL of tests/test_batch_gradient_gpu.py: the project's bar
SEGMENTS = (1, 2, 5, 3)


def operators(rng, d, A, H):
    def herm(n):
        M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
        return M + M.conj().transpose(0, 2, 1)
    return herm(H), herm(A)


def make_gate(rng, c_opers, n_opers, G, d, c_coeffs=None):
    """A gate over the shared operators: its own amplitudes, sensitivities (per segment) and durations."""
    H, A = len(c_opers), len(n_opers)
    c_coeffs = rng.standard_normal((H, G)) if c_coeffs is None else c_coeffs
    n_coeffs = rng.random((A, G)) + 0.1
    dt = rng.random(G) + 0.2
    return ff.PulseSequence(list(zip(c_opers, c_coeffs)), list(zip(n_opers, n_coeffs)), dt, ff.Basis.ggm(d))


def gate_set(seed, d, A, H, segments=SEGMENTS):
    rng = np.random.default_rng(seed)
    c_opers, n_opers = operators(rng, d, A, H)
    return [make_gate(rng, c_opers, n_opers, G, d) for G in segments]


def crossing_grid(rng, W):
    omega = np.sort(rng.random(W))*10 - 2.0                    # negative frequencies ...
    omega[W//2] = 0.0                                          # ... and w = 0
    return np.sort(omega)


def some_sequences(rng, T):
    """Lengths 1, 2, 3, 17 and 65 (the last crosses the chunk of 64 positions); the fourth with negative indices."""
    seqs = [rng.integers(0, T, n) for n in (1, 2, 3, 17, 65)]
    seqs[3] = seqs[3] - T
    seqs[1] = np.array([2, 2])                                 # the longest gate twice
    return seqs


def the_loop(gates, sequences, S, omega, **kw):
    table = np.asarray(gates, dtype=object)
    pulses = [ff.concatenate(table[s]) for s in sequences]
    if S is None:
        return [gradient.filter_function_derivative(p, omega, **kw) for p in pulses]
    return [gradient.infidelity_derivative(p, S, omega, **kw) for p in pulses]


def assert_batched(gates, **selected):
    """The case runs the kernels, not the loop."""
    n_ctrl = len(selected.get('control_identifiers', gates[0].c_oper_identifiers))
    n_nops = len(selected.get('n_oper_identifiers', gates[0].n_oper_identifiers))
    assert sequence_gradient.eligibility(gates, n_ctrl, n_nops) is not None


def host_scatter(segments, sequences, values, weights):
    """The per-gate sums from the sequences' arrays, written out here: p ascending, then position ascending."""
    A, H = values[0].shape[0], values[0].shape[2]
    out = [np.zeros((A, G, H)) for G in segments]
    for p, s in enumerate(sequences):
        at = 0
        for k in s:
            out[k] += weights[p]*values[p][:, at:at + segments[k]]
            at += segments[k]
    return out


def compare_lists(got, ref, what, worst):
    assert len(got) == len(ref)
    for p, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and a.dtype == np.float64, (what, p, a.shape, b.shape)
        worst[what] = max(worst.get(what, 0.0), rel_err(a, b))


@pytest.mark.parametrize('d', [2, 3, 4])
@pytest.mark.parametrize('A,H,W', [(1, 1, 7), (2, 2, 64), (3, 2, 65), (4, 8, 70)])
def test_against_the_loop(d, A, H, W):
    """A partial tile, a full tile, one frequency past it and a partial second tile; gates of 1, 2, 5 and 3 segments;
    sequences of 1 to 65 positions; spectra of one and of two dimensions.  The route differs from the loop only in
    rounding: gate-local times plus one phase per position against the cumulated times of the joined pulse."""
    rng = np.random.default_rng(9100 + 10*d + A)
    gates = gate_set(9200 + 10*d + A, d, A, H)
    sequences = some_sequences(rng, len(gates))
    omega = crossing_grid(rng, W)
    weights = rng.standard_normal(len(sequences))
    assert_batched(gates)
    wrapped = [np.where(s < 0, s + len(gates), s) for s in sequences]
    worst = {}
    ref = the_loop(gates, sequences, None, omega)
    got = ff.sequence_filter_function_derivatives(gates, sequences, omega)
    for p, s in enumerate(wrapped):
        assert got[p].shape == (A, sum(SEGMENTS[k] for k in s), H, W)
    compare_lists(got, ref, 'dF', worst)
    for S in (1.0/(1.0 + omega**2), rng.random((A, W)) + 0.1):
        ref = the_loop(gates, sequences, S, omega)
        compare_lists(ff.sequence_infidelity_derivatives(gates, sequences, S, omega), ref, f'dI S{S.ndim}', worst)
        compare_lists(ff.gate_infidelity_derivatives(gates, sequences, S, omega, weights),
                      host_scatter(SEGMENTS, wrapped, ref, weights), f'gate S{S.ndim}', worst)
    for key, value in worst.items():
        print(f'd={d} A={A} H={H} W={W} {key}: rel_err {value:.3e}')
    for key, value in worst.items():
        assert value < TOL, key


def test_identifiers_as_a_subset_in_another_order():
    d, W = 3, 70
    rng = np.random.default_rng(9300)
    gates = gate_set(9301, d, 3, 4)
    sequences = some_sequences(rng, len(gates))[:4]
    omega = crossing_grid(rng, W)
    S = 1.0/(1.0 + omega**2)
    c_ids, n_ids = gates[0].c_oper_identifiers, gates[0].n_oper_identifiers
    kw = dict(control_identifiers=[c_ids[3], c_ids[0], c_ids[2]], n_oper_identifiers=[n_ids[2], n_ids[0]])
    assert_batched(gates, **kw)
    worst = {}
    compare_lists(ff.sequence_infidelity_derivatives(gates, sequences, S, omega, **kw),
                  the_loop(gates, sequences, S, omega, **kw), 'dI', worst)
    compare_lists(ff.sequence_filter_function_derivatives(gates, sequences, omega, **kw),
                  the_loop(gates, sequences, None, omega, **kw), 'dF', worst)
    print(worst)
    assert max(worst.values()) < TOL
    got = ff.sequence_infidelity_derivatives(gates, sequences, S, omega, **kw)
    assert got[0].shape == (2, SEGMENTS[int(sequences[0][0])], 3)


def test_finite_differences_of_the_sequence_infidelities():
    """The inputs and bounds of test_finite_differences_of_the_batched_infidelities (tests/test_batch_gradient_gpu.py);
    a sequence of six positions in which the perturbed gate stands three times.  Nothing here goes through
    ``gradient.infidelity_derivative``."""
    rng = np.random.default_rng(4200)
    d = 3

    def herm(n):
        M = rng.standard_normal((n, d, d)) + 1j*rng.standard_normal((n, d, d))
        return M + M.conj().transpose(0, 2, 1)
    c_opers, n_opers = herm(2), herm(2)
    c_opers = (c_opers + c_opers.conj().transpose(0, 2, 1))/2
    n_opers = (n_opers + n_opers.conj().transpose(0, 2, 1))/2
    segments = (4, 2, 3)
    c_coeffs = [rng.standard_normal((2, G)) for G in segments]
    n_coeffs = [rng.random((2, G)) + 0.5 for G in segments]
    dts = [rng.random(G) + 0.3 for G in segments]
    omega = np.geomspace(1e-2, 30, 200)
    S = 1e-2/omega
    eps = 1e-6
    sequence = [np.array([1, 0, 2, 1, 1, 0])]
    k = 1                                                       # stands three times

    def gates_with(cc_k):
        cc = list(c_coeffs)
        cc[k] = cc_k
        return [ff.PulseSequence(list(zip(c_opers, cc[j])), list(zip(n_opers, n_coeffs[j])), dts[j], ff.Basis.ggm(d))
                for j in range(len(segments))]
    G = segments[k]
    infids = np.empty((G, 2, 2, 2))
    for s in range(G):
        for h in range(2):
            for j, sign in enumerate((1.0, -1.0)):
                cc = c_coeffs[k].copy()
                cc[h, s] += sign*eps
                infids[s, h, j] = ff.sequence_infidelities(gates_with(cc), sequence, S, omega)[0]
    fd = (infids[:, :, 0] - infids[:, :, 1])/(2*eps)                 # (G, H, A)
    gates = gates_with(c_coeffs[k])
    assert_batched(gates)
    grad = ff.gate_infidelity_derivatives(gates, sequence, S, omega)
    assert [g.shape for g in grad] == [(2, G_j, 2) for G_j in segments]
    order = np.argsort(np.argsort(gates[k].c_oper_identifiers))
    for s in range(G):
        for h in range(2):
            print(s, h, grad[k][:, s, order[h]], fd[s, h])
            assert np.allclose(grad[k][:, s, order[h]], fd[s, h], rtol=1e-5, atol=1e-9), (s, h)


@pytest.mark.parametrize('d', [2, 4])
def test_one_gate_at_one_position(d):
    rng = np.random.default_rng(9400 + d)
    gates = gate_set(9401 + d, d, 2, 2)
    omega = crossing_grid(rng, 70)
    S = 1.0/(1.0 + omega**2)
    for k in (0, 2):
        twin = [ff.PulseSequence(list(zip(gates[k].c_opers, gates[k].c_coeffs)),
                                 list(zip(gates[k].n_opers, gates[k].n_coeffs)), gates[k].dt, ff.Basis.ggm(d))
                for _ in range(2)]
        ref = ff.infidelity_derivatives(twin, S, omega)[0]
        got = ff.sequence_infidelity_derivatives(gates, [[k]], S, omega)[0]
        assert got.shape == ref.shape
        assert rel_err(got, ref) < TOL
        ref = ff.filter_function_derivatives(twin, omega)[0]
        assert rel_err(ff.sequence_filter_function_derivatives(gates, [[k]], omega)[0], ref) < TOL


@pytest.fixture(scope='module')
def bits_case():
    d, A, H, W = 3, 2, 2, 70
    rng = np.random.default_rng(9500)
    gates = gate_set(9501, d, A, H)
    for g in gates:
        g.diagonalize()
    omega = crossing_grid(rng, W)
    S = rng.random((A, W)) + 0.1
    mine = np.array([3, 0, 2, 2, 1, 3, 0])
    others = [rng.integers(0, len(gates), n) for n in rng.integers(1, 30, 20)]
    alone = (ff.sequence_infidelity_derivatives(gates, [mine], S, omega)[0],
             ff.sequence_filter_function_derivatives(gates, [mine], omega)[0],
             ff.gate_infidelity_derivatives(gates, [mine], S, omega, [0.7]))
    return gates, omega, S, mine, others, alone


def one_hot(n, at, value):
    w = np.zeros(n)
    w[at] = value
    return w


@pytest.mark.parametrize('place', ['first', 'last'])
def test_a_sequence_does_not_depend_on_its_pass(bits_case, place):
    gates, omega, S, mine, others, alone = bits_case
    sequences = [mine] + others if place == 'first' else others + [mine]
    at = 0 if place == 'first' else len(others)
    assert np.array_equal(ff.sequence_infidelity_derivatives(gates, sequences, S, omega)[at], alone[0])
    assert np.array_equal(ff.sequence_filter_function_derivatives(gates, sequences, omega)[at], alone[1])
    # (the per-gate sums of the pass with every other sequence weighted zero)
    sums = ff.gate_infidelity_derivatives(gates, sequences, S, omega, one_hot(len(sequences), at, 0.7))
    assert all(np.array_equal(a, b) for a, b in zip(sums, alone[2]))


def test_a_sequence_does_not_depend_on_the_pass_split(bits_case, monkeypatch):
    gates, omega, S, mine, others, alone = bits_case
    sequences = others[:10] + [mine] + others[10:]
    weights = np.random.default_rng(9502).standard_normal(len(sequences))
    whole = (ff.sequence_infidelity_derivatives(gates, sequences, S, omega),
             ff.sequence_filter_function_derivatives(gates, sequences, omega),
             ff.gate_infidelity_derivatives(gates, sequences, S, omega, weights))
    T, G, W, A, H, d = len(gates), max(SEGMENTS), len(omega), 2, 2, 3
    most, longest = max(sum(SEGMENTS[k] for k in s) for s in sequences), max(len(s) for s in sequences)
    for want_dF in (False, True):
        per, fixed = sequence_gradient.sequence_bytes(T, G, W, A, H, d, want_dF, most, longest)
        monkeypatch.setattr(batch, 'PASS_BYTES', fixed + 5*per)
        assert len(sequence_gradient.split_sequences(list(range(len(sequences))), T, G, W, A, H, d, want_dF, most,
                                                     longest)) >= 4
        if want_dF:
            split = ff.sequence_filter_function_derivatives(gates, sequences, omega)
            assert all(np.array_equal(a, b) for a, b in zip(split, whole[1]))
            assert np.array_equal(split[10], alone[1])
        else:
            split = ff.sequence_infidelity_derivatives(gates, sequences, S, omega)
            assert all(np.array_equal(a, b) for a, b in zip(split, whole[0]))
            assert np.array_equal(split[10], alone[0])
            # consecutive passes continue one sequential sum: the same bits as one pass
            sums = ff.gate_infidelity_derivatives(gates, sequences, S, omega, weights)
            assert all(np.array_equal(a, b) for a, b in zip(sums, whole[2]))
            sums = ff.gate_infidelity_derivatives(gates, sequences, S, omega, one_hot(len(sequences), 10, 0.7))
            assert all(np.array_equal(a, b) for a, b in zip(sums, alone[2]))


def test_the_per_gate_sums_are_sequential_sums_in_the_documented_order(bits_case):
    gates, omega, S, mine, others, alone = bits_case
    sequences = [mine] + others
    weights = np.random.default_rng(9503).standard_normal(len(sequences))
    values = ff.sequence_infidelity_derivatives(gates, sequences, S, omega)
    got = ff.gate_infidelity_derivatives(gates, sequences, S, omega, weights)
    ref = [np.zeros((2, G, 2)) for G in SEGMENTS]
    magnitude = [np.zeros((2, G, 2)) for G in SEGMENTS]
    count = np.zeros(len(gates), dtype=int)
    for p, s in enumerate(sequences):                           # p ascending, then position ascending
        at = 0
        for k in s:
            ref[k] += weights[p]*values[p][:, at:at + SEGMENTS[k]]
            magnitude[k] += np.abs(weights[p]*values[p][:, at:at + SEGMENTS[k]])
            count[k] += 1
            at += SEGMENTS[k]
    assert count.min() > 3
    for k in range(len(gates)):
        # both are sequential sums of the same n summands: each within n 2^-53 sum|.| of the exact sum
        assert np.all(np.abs(got[k] - ref[k]) <= count[k]*2.0**-52*magnitude[k]), k


def test_gate_sets_the_batched_route_does_not_take_return_what_the_loop_returns():
    W = 33
    rng = np.random.default_rng(9600)
    omega = crossing_grid(rng, W)
    S = 1.0/(1.0 + omega**2)
    sequences = [np.array([0, 1, 1]), np.array([-1, 0])]
    five = lambda: gate_set(9601, 5, 2, 2, (2, 3))                # noqa: E731

    def unequal():
        gates = gate_set(9602, 2, 2, 2, (2, 3))
        c_opers = np.array(gates[1].c_opers)
        c_opers[0] = c_opers[0] + np.diag([1.0, -1.0])
        gates[1] = ff.PulseSequence(list(zip(c_opers, gates[1].c_coeffs)),
                                    list(zip(gates[1].n_opers, gates[1].n_coeffs)), gates[1].dt, ff.Basis.ggm(2))
        return gates
    for build, spectrum in ((five, S), (unequal, S), (lambda: gate_set(9603, 2, 2, 2, (2, 3)), S*(1 + 0.5j))):
        assert sequence_gradient._plan(build(), np.asarray(spectrum), omega, None, None) is None
        ref = the_loop(build(), sequences, spectrum, omega)
        got = ff.sequence_infidelity_derivatives(build(), sequences, spectrum, omega)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref))
        wrapped = [np.where(s < 0, s + 2, s) for s in sequences]
        sums = ff.gate_infidelity_derivatives(build(), sequences, spectrum, omega, [0.5, 2.0])
        host = host_scatter((2, 3), wrapped, ref, [0.5, 2.0])
        assert all(np.array_equal(a, b) for a, b in zip(sums, host))
        if build is unequal:
            # a sequence of one gate carries that gate's two control operators, the others the merged three
            with pytest.raises(ValueError):
                ff.gate_infidelity_derivatives(build(), sequences + [np.array([1])], spectrum, omega)
        if spectrum is S:
            ref = the_loop(build(), sequences, None, omega)
            got = ff.sequence_filter_function_derivatives(build(), sequences, omega)
            assert all(np.array_equal(a, b) for a, b in zip(got, ref))


def test_exceptions_are_those_of_the_loop_and_caches_stay():
    d, A, W = 2, 2, 33
    rng = np.random.default_rng(9700)
    omega = crossing_grid(rng, W)
    S = 1.0/(1.0 + omega**2)
    fresh = lambda: gate_set(9701, d, A, 2)                     # noqa: E731
    sequences = [[0, 1], [2, 3, 3]]
    ids = fresh()[0].n_oper_identifiers
    for args, kw in (((np.ones(W + 1),), {}),                                      # does not fit
                     ((np.ones((A, A, W)),), {}),                                  # three dimensions
                     ((np.ones((A, W)),), dict(n_oper_identifiers=ids[:1])),       # rows for operators not selected
                     ((S,), dict(control_identifiers=['no such control'])),
                     ((S,), dict(n_oper_identifiers=['no such noise']))):
        with pytest.raises(Exception) as loop:
            the_loop(fresh(), sequences, args[0], omega, **kw)
        with pytest.raises(loop.type) as mine:
            ff.sequence_infidelity_derivatives(fresh(), sequences, *args, omega, **kw)
        assert str(mine.value) == str(loop.value)
        with pytest.raises(loop.type) as mine:
            ff.gate_infidelity_derivatives(fresh(), sequences, *args, omega, **kw)
        assert str(mine.value) == str(loop.value)
    with pytest.raises(ValueError) as loop:
        the_loop(fresh(), sequences, None, omega, control_identifiers=['no such control'])
    with pytest.raises(ValueError) as mine:
        ff.sequence_filter_function_derivatives(fresh(), sequences, omega, control_identifiers=['no such control'])
    assert str(mine.value) == str(loop.value)
    with pytest.raises(IndexError):
        ff.sequence_infidelity_derivatives(fresh(), [[0, 4]], S, omega)
    with pytest.raises(ValueError):
        ff.sequence_infidelity_derivatives(fresh(), [[0], []], S, omega)
    with pytest.raises(TypeError):
        ff.sequence_infidelity_derivatives(fresh(), [[0.5]], S, omega)
    with pytest.raises(ValueError):
        ff.gate_infidelity_derivatives(fresh(), sequences, S, omega, weights=[1.0])
    # a batched call leaves the gates' frequency data as it found it, and reads the eigensystems it finds
    gates = fresh()
    ff.infidelities(gates, S, omega)
    keys = ('eigvals', 'eigvecs', 'propagators')
    before = [{k: g._frequency_data.peek(k) for k in g._frequency_data} for g in gates]
    eigensystems = [[g._data[k] for k in keys] for g in gates]
    ff.sequence_infidelity_derivatives(gates, sequences, S, omega)
    ff.gate_infidelity_derivatives(gates, sequences, S, omega)
    ff.sequence_filter_function_derivatives(gates, sequences, omega)
    for g, frequency_data, row in zip(gates, before, eigensystems):
        assert set(g._frequency_data) == set(frequency_data)
        assert all(g._frequency_data.peek(k) is v for k, v in frequency_data.items())
        assert all(g._data[k] is v for k, v in zip(keys, row))

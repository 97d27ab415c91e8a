"""CPU side of ffk_expm_real_batch and ff.exponentiate_cumulant_functions: the ABI in header, exports and binding, the
workspace query without a GPU, the refusals of the entries before the device, the routes of the Python function that need
no device (complex input, N > 16, bad shapes and types), the chunking under the budget (the entry replaced by a stand-in),
and the 50-digit yardstick of the GPU tests against closed forms."""
import ctypes

import numpy as np
import pytest
from scipy import linalg as sla

import filter_functions_amd as ff
from expm_yardstick import closed_forms, expm50
from filter_functions_amd import _lib, expm_batch
from filter_functions_amd import sequence_prefix_second_order as sp2

ENTRIES = ('ffk_expm_real_batch_workspace_bytes', 'ffk_expm_real_batch_dev', 'ffk_expm_real_batch')


def test_public_names():
    assert 'exponentiate_cumulant_functions' in ff.__all__ and 'expm_batch' in ff.__all__
    assert ff.exponentiate_cumulant_functions is expm_batch.exponentiate_cumulant_functions
    assert 'sequence_prefix_error_transfer_matrices' in ff.__all__
    assert ff.sequence_prefix_error_transfer_matrices is sp2.sequence_prefix_error_transfer_matrices
    doc = ff.sequence_prefix_error_transfer_matrices.__doc__
    assert 'SHARED' not in doc and 'closing' in doc and 'sequence_prefix_cumulant_functions' in doc
    assert 'along a sequence are not offered' not in ff.sequence_prefix_cumulant_functions.__doc__
    assert 'sequence_prefix_error_transfer_matrices' in ff.sequence_prefix_cumulant_functions.__doc__


def test_binding_header_and_exports_agree():
    import test_abi
    names = test_abi.header_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in names and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES[ENTRIES[0]] == (ctypes.c_size_t, [ctypes.c_long, ctypes.c_int, ctypes.c_int])
    assert len(_lib.SIGNATURES[ENTRIES[1]][1]) == 7 and len(_lib.SIGNATURES[ENTRIES[2]][1]) == 6


def test_workspace_query_needs_no_gpu():
    query = _lib.load().ffk_expm_real_batch_workspace_bytes
    for count, rows, N in ((1, 1, 1), (1000, 3, 4), (16000, 2, 16), (7, 4, 9)):
        need = 8*count*rows*N*N + 8*count*N*N + 4*count
        assert need <= query(count, rows, N) <= need + 3*256
    assert query(1 << 33, 1, 4) > (1 << 33)*256                   # a long count
    assert query(10, 1, 17) == 0 and query(10, 1, 0) == 0 and query(10, 0, 4) == 0 and query(-1, 1, 4) == 0
    # what the Python function counts per matrix is what the entry stages
    assert expm_batch.chunk_length(3, 4, budget=1 << 20) == (1 << 20)//(8*3*16 + 8*16 + 4)
    assert expm_batch.chunk_length(4, 16, budget=10) == 1


def test_bad_arguments_are_refused_before_the_device():
    lib = _lib.load()
    tiles, out, flags = np.zeros((2, 3, 4, 4)), np.zeros((2, 4, 4)), np.zeros(2, dtype=np.int32)
    good = dict(tiles=tiles.ctypes.data, count=2, rows=3, N=4, result=out.ctypes.data, not_finite=flags.ctypes.data)
    cases = [(dict(tiles=None), 'NULL'), (dict(result=None), 'NULL'), (dict(not_finite=None), 'NULL'),
             (dict(count=-1), 'count'), (dict(rows=0), 'rows'), (dict(rows=-2), 'rows'), (dict(N=0), 'outside [1, 16]'),
             (dict(N=17), 'outside [1, 16]'), (dict(N=-4), 'outside [1, 16]')]
    for change, message in cases:
        a = {**good, **change}
        host = (a['tiles'], a['count'], a['rows'], a['N'], a['result'], a['not_finite'])
        for entry, args in ((lib.ffk_expm_real_batch, host), (lib.ffk_expm_real_batch_dev, host + (None,))):
            assert entry(*args) == _lib.FFK_EINVAL, change
            assert message in lib.ffk_last_error().decode(), (change, lib.ffk_last_error().decode())
    # no matrix: success, nothing touched (no device here)
    host = (good['tiles'], 0, 3, 4, good['result'], good['not_finite'])
    assert lib.ffk_expm_real_batch(*host) == _lib.FFK_OK
    assert lib.ffk_expm_real_batch_dev(*host, None) == _lib.FFK_OK
    assert not out.any() and not flags.any()


def test_the_yardstick_against_closed_forms():
    """mpmath's exponential at 50 digits, the reference of the GPU tests: a diagonal matrix, a plane rotation and a
    nilpotent block at N = 4 and 16, to the last bit of the double."""
    for N in (4, 16):
        for name, K, exact in closed_forms(N):
            got = expm50(K)
            scale = np.abs(exact).max()
            assert np.abs(got - exact).max() <= 2*np.finfo(float).eps*scale, (N, name)


def test_complex_input_is_the_single_function_per_matrix():
    """Needs no device: complex input is what the reference's call does with it, per matrix."""
    rng = np.random.default_rng(0)
    K = rng.standard_normal((5, 2, 4, 4)) + 1j*rng.standard_normal((5, 2, 4, 4))
    got = ff.exponentiate_cumulant_functions(K)
    assert got.shape == (5, 4, 4) and np.iscomplexobj(got)
    for g, k in zip(got, K):
        assert np.array_equal(g, sla.expm(k.sum(axis=0)))
        assert np.array_equal(g, ff.error_transfer_matrix(cumulant_function=k))
    # a list of members does the same
    assert np.array_equal(ff.exponentiate_cumulant_functions(list(K)), got)


def test_empty_input():
    for empty, shape in ((np.empty((0, 3, 4, 4)), (0, 4, 4)), (np.empty((0, 16, 16)), (0, 16, 16)), ([], (0, 0, 0))):
        got = ff.exponentiate_cumulant_functions(empty)
        assert got.shape == shape and got.dtype == np.float64


def same_exception(call, reference):
    with pytest.raises(Exception) as ref:
        reference()
    with pytest.raises(type(ref.value)) as got:
        call()
    assert str(got.value) == str(ref.value)


def test_bad_shapes_and_types_raise_what_the_single_function_raises():
    bad = [[[1.0, 2.0], [3.0, 4.0]]]                                   # a member that is a list: no sum
    same_exception(lambda: ff.exponentiate_cumulant_functions(bad),
                   lambda: ff.error_transfer_matrix(cumulant_function=bad[0]))
    for stack in (np.ones((3, 4)),                                     # members of one dimension
                  np.ones((3, 2, 4, 5)), np.ones((2, 3, 4)),           # members that are not square
                  np.ones(3)):                                         # scalars
        same_exception(lambda: ff.exponentiate_cumulant_functions(stack),
                       lambda: ff.error_transfer_matrix(cumulant_function=stack[0]))
    with pytest.raises(TypeError):
        ff.exponentiate_cumulant_functions(None)


class Entry:
    """Stands in for the library: records the chunks and answers exp of a diagonal sum, flagging what is not finite."""

    def __init__(self):
        self.calls = []

    def ffk_expm_real_batch(self, tiles, count, rows, N, result, not_finite):
        def array(address, shape, dtype=np.float64):
            n = int(np.prod(shape))*np.dtype(dtype).itemsize
            return np.frombuffer((ctypes.c_char*n).from_address(address), dtype=dtype).reshape(shape)
        self.calls.append((count, rows, N))
        with np.errstate(invalid='ignore'):
            K = array(tiles, (count, rows, N, N)).sum(axis=1)
        bad = ~np.isfinite(K).all(axis=(1, 2))
        array(not_finite, (count,), np.int32)[:] = bad
        array(result, (count, N, N))[:] = np.where(bad[:, None, None], -1.0, np.exp(K)*np.eye(N))
        return 0


def test_chunks_flags_and_routes_with_a_stand_in(monkeypatch):
    library = Entry()
    monkeypatch.setattr(expm_batch._lib, 'load', lambda: library)
    rng = np.random.default_rng(1)
    K = rng.standard_normal((23, 3, 2, 4, 4))*np.eye(4)
    want = np.exp(K.sum(axis=(1, 2)))*np.eye(4)
    got = ff.exponentiate_cumulant_functions(K)
    assert library.calls == [(23, 6, 4)] and np.array_equal(got, want)
    # a budget of five matrices: five chunks, every result in its place; integers and lists of arrays take the entry too
    monkeypatch.setattr(expm_batch, 'PASS_BYTES', 5*(8*6*16 + 8*16 + 4) + 3)
    library.calls.clear()
    assert np.array_equal(ff.exponentiate_cumulant_functions(list(K)), want)
    assert library.calls == [(5, 6, 4)]*4 + [(3, 6, 4)]
    library.calls.clear()
    ints = np.arange(2*9).reshape(2, 3, 3)*np.eye(3, dtype=int)
    assert np.array_equal(ff.exponentiate_cumulant_functions(ints), np.exp(ints)*np.eye(3))
    assert library.calls == [(2, 1, 3)]
    # a flagged matrix is the single function's (patched here: it would need the device or raise)
    monkeypatch.setattr(expm_batch, '_single', lambda k: np.full(k.shape[-2:], 7.0))
    K[4, 1, 1, 2, 2] = np.inf
    K[9, 0, 0, 1, 1], K[9, 2, 1, 1, 1] = np.inf, -np.inf            # not finite in the sum alone: NaN
    got = ff.exponentiate_cumulant_functions(K)
    assert (got[[4, 9]] == 7.0).all()
    keep = np.ones(23, dtype=bool)
    keep[[4, 9]] = False
    assert np.array_equal(got[keep], want[keep])
    # N > 16, float32, members of several shapes: the loop's expression, no call of the entry
    library.calls.clear()
    assert ff.exponentiate_cumulant_functions(np.zeros((2, 17, 17))).shape == (2, 17, 17)
    assert ff.exponentiate_cumulant_functions(np.zeros((2, 4, 4), dtype=np.float32)).shape == (2, 4, 4)
    assert ff.exponentiate_cumulant_functions([np.zeros((4, 4)), np.zeros((2, 4, 4))]).shape == (2, 4, 4)
    assert not library.calls


def test_prefix_error_transfer_matrices_compose_the_cumulant_functions_and_one_exponential(monkeypatch):
    """The composition on the host, both calls replaced by stand-ins: the arguments reach
    sequence_prefix_cumulant_functions unchanged, every position's tiles go through the exponential ONCE, and every
    matrix comes back to its place -- stacked and not, spectra of one operator axis and cross-spectra."""
    seqs = [[0, 1], [2], [1, 1, 0]]
    asked, exponentials = [], []

    def cumulants(n_axes):
        def call(gates, sequences, spectrum, omega, n_oper_identifiers=None, closing=None, second_order=False,
                 stacked=False, return_propagators=False):
            asked.append((gates, sequences, n_oper_identifiers, closing, second_order, stacked, return_propagators))
            lead = (len(spectrum),) if stacked else ()
            rng = np.random.default_rng(3)
            values = [rng.standard_normal(lead + (len(s),) + (2,)*n_axes + (4, 4)) for s in sequences]
            return (values, [np.ones((len(s), 2, 2)) for s in sequences]) if return_propagators else values
        return call

    def exponential(tiles):
        exponentials.append(np.shape(tiles))
        return np.asarray(tiles).sum(axis=1) + 100.0
    monkeypatch.setattr(expm_batch, 'exponentiate_cumulant_functions', exponential)
    for n_axes in (1, 2):
        monkeypatch.setattr(sp2, 'sequence_prefix_cumulant_functions', cumulants(n_axes))
        rows = 2**n_axes
        for stacked, spectrum in ((False, np.ones(5)), (True, np.ones((3, 5)))):
            K = cumulants(n_axes)('g', seqs, spectrum, 'w', stacked=stacked)
            asked.clear()
            exponentials.clear()
            got, U = ff.sequence_prefix_error_transfer_matrices('g', seqs, spectrum, 'w', ['Z'], closing='c',
                                                                second_order=True, stacked=stacked,
                                                                return_propagators=True)
            assert asked == [('g', seqs, ['Z'], 'c', True, stacked, True)]
            n = (3 if stacked else 1)*6
            assert exponentials == [(n, rows, 4, 4)]
            assert [u.shape for u in U] == [(len(s), 2, 2) for s in seqs]
            for g, k, s in zip(got, K, seqs):
                assert g.shape == ((3,) if stacked else ()) + (len(s), 4, 4)
                assert np.array_equal(g, k.sum(axis=tuple(range(g.ndim - 2, k.ndim - 2))) + 100.0)
            plain = ff.sequence_prefix_error_transfer_matrices('g', seqs, spectrum, 'w', stacked=stacked)
            assert asked[-1] == ('g', seqs, None, None, False, stacked, False) and isinstance(plain, list)

"""ffk_expm_real_batch and ff.exponentiate_cumulant_functions on the GPU: cases in which every step is exact, the
orientation of the products, the accuracy against a 50-digit exponential next to the parent route's and SciPy's, the
bits of a matrix whatever surrounds it, and the matrices that are not finite."""
import numpy as np
import pytest
from scipy import linalg as sla

import filter_functions_amd as ff
from expm_yardstick import NORMS, expm50, grid_matrix, grid_tiles, nilpotent_block, one_norm, plane_rotation
from filter_functions_amd import _lib, expm_batch, numeric

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def entry(tiles):
    """The C entry on tiles (n, rows, N, N): (result, flags)."""
    tiles = np.ascontiguousarray(tiles, dtype=np.float64)
    n, rows, N = tiles.shape[:3]
    out = np.full((n, N, N), np.nan)
    flags = np.full(n, -1, dtype=np.int32)
    _lib.check(_lib.load().ffk_expm_real_batch(tiles.ctypes.data, n, rows, N, out.ctypes.data, flags.ctypes.data))
    return out, flags


def both(tiles):
    """The result of the C entry, checked to be the bits of the Python function's and flag-free."""
    out, flags = entry(tiles)
    assert not flags.any()
    assert np.array_equal(out, ff.exponentiate_cumulant_functions(np.asarray(tiles)))
    return out


# ---- exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [4, 16])
def test_nilpotent_blocks_and_zero_are_exact(N):
    """K K = 0: scaling, every product of the Taylor scheme and every squaring are exact, so exp K = I + K to the bit --
    with entries up to 40 several squarings run.  K is not symmetric: a mixed-up (X, X^T) pair or a wrong row map
    fails here."""
    cases = [nilpotent_block(N, seed, largest) for seed, largest in ((0, 40), (1, 40), (2, 3), (3, 1))]
    K = np.stack([k for k, _ in cases] + [np.zeros((N, N))])
    assert one_norm(K[0]) > 32 and one_norm(K[3]) <= N
    want = np.stack([u for _, u in cases] + [np.eye(N)])
    assert np.array_equal(both(K[:, None]), want)
    # the same matrices as sums of three tiles
    tiles = np.stack([K, 2*K, -2*K], axis=1)
    assert np.array_equal(both(tiles), want)


# ---- orientation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [4, 16])
@pytest.mark.parametrize('theta', [0.3, 20.0])
def test_a_plane_rotation_turns_the_right_way(N, theta):
    """K = theta J on one plane: the rotation by +theta (a transposed operand returns -theta)."""
    planes = [(0, N - 1), (1, 2), (N - 2, 0)]
    K = np.stack([plane_rotation(N, theta, i, j)[0] for i, j in planes])
    want = np.stack([plane_rotation(N, theta, i, j)[1] for i, j in planes])
    got = both(K[:, None])
    print('rotation', N, theta, np.abs(got - want).max())
    assert np.abs(got - want).max() < 1e-13*max(1.0, theta)
    assert np.abs(got - want.swapaxes(1, 2)).max() > 0.2


# ---- accuracy ---------------------------------------------------------------------------------------------------------
_YARD = {}


def accuracy_inputs(N):
    """The matrices of one N (on the fixed-point grid of expm_yardstick: every split into tiles adds up to them without
    rounding) and their 50-digit exponentials, computed once and shared by the cases of every `rows`."""
    if N not in _YARD:
        rng = np.random.default_rng(100 + N)
        per_norm = 4                                         # (40 matrices: the yardstick stays within seconds)
        inputs = [grid_matrix(rng, N, norm) for norm in NORMS for _ in range(per_norm)]
        K = np.stack([k for k, _, _ in inputs])
        _YARD[N] = (K, [q for _, _, q in inputs], np.repeat(np.arange(len(NORMS)), per_norm),
                    np.stack([expm50(k) for k in K]))
    return _YARD[N]


def measure(U, U_ref):
    """The project's measure (assert_etm_close of test_processes_gpu.py): max|U - U_ref| against max|U_ref - I|."""
    return np.abs(U - U_ref).max()/np.abs(U_ref - np.eye(len(U_ref))).max()


@pytest.mark.parametrize('rows', [1, 2, 4])
@pytest.mark.parametrize('N', [1, 3, 4, 5, 9, 15, 16])
def test_accuracy_next_to_the_parent_route_and_scipy(N, rows):
    """Against the 50-digit exponential, per class of 1-norm (1e-12, at and on both sides of the squaring boundaries
    1/2 and 1, 3, 20, 50): the new route's worst error is at most twice the larger of the worst errors of the parent
    route (numeric.error_transfer_matrix per matrix) and of scipy.linalg.expm (what the reference calls) on the same
    tiles, plus four units in the last place of max|U_ref| for the classes both get exactly."""
    K, quanta, classes, U_ref = accuracy_inputs(N)
    assert len(K) <= 40
    rng = np.random.default_rng(7*N + rows)
    tiles = np.stack([grid_tiles(rng, k, rows, q) for k, q in zip(K, quanta)])
    new = both(tiles)
    parent = np.stack([numeric.error_transfer_matrix(cumulant_function=t) for t in tiles])
    scipy = np.stack([sla.expm(t.sum(axis=0)) for t in tiles])
    for c, norm in enumerate(NORMS):
        members = np.flatnonzero(classes == c)
        errors = {name: max(measure(U[m], U_ref[m]) for m in members)
                  for name, U in (('new', new), ('parent', parent), ('scipy', scipy))}
        floor = max(4*EPS*np.abs(U_ref[m]).max()/np.abs(U_ref[m] - np.eye(N)).max() for m in members)
        print(f'N={N} rows={rows} norm={norm:.3g}: new {errors["new"]:.2e} parent {errors["parent"]:.2e} '
              f'scipy {errors["scipy"]:.2e} floor {floor:.2e}')
        assert errors['new'] <= 2*max(errors['parent'], errors['scipy']) + floor, (N, rows, norm, errors)


# ---- same bits ----------------------------------------------------------------------------------------------------------
def random_tiles(rng, n, rows, N, norms):
    tiles = rng.standard_normal((n, rows, N, N))
    scale = np.resize(np.asarray(norms, dtype=float), n)/np.abs(tiles.sum(axis=1)).sum(axis=1).max(axis=1)
    return tiles*scale[:, None, None, None]


@pytest.mark.parametrize('N, rows', [(4, 1), (4, 3), (16, 1), (16, 2), (9, 2), (1, 1)])
def test_a_matrix_has_the_same_bits_wherever_it_stands(N, rows, monkeypatch):
    rng = np.random.default_rng(N + rows)
    pool = random_tiles(rng, 1000, rows, N, [1e-3, 0.4, 0.7, 3.0, 20.0, 60.0, 1e-9])
    probe = random_tiles(rng, 1, rows, N, [7.0])
    alone = both(probe)
    assert np.isfinite(alone).all()
    first = both(np.concatenate([probe, pool[:64]]))
    last = both(np.concatenate([pool[:999], probe]))
    assert np.array_equal(first[0], alone[0]) and np.array_equal(last[-1], alone[0])
    # every count gives the bits of the matrices' own calls
    whole = both(pool[:257])
    for count in (1, 63, 64, 65, 257):
        assert np.array_equal(both(pool[:count]), whole[:count]), count
    for i in (0, 63, 64, 256):
        assert np.array_equal(both(pool[i:i + 1])[0], whole[i]), i
    # one pass against a budget that forces at least seven chunks
    calls = []
    real = _lib.load().ffk_expm_real_batch

    class Counting:
        def ffk_expm_real_batch(self, *args):
            calls.append(args[1])
            return real(*args)
    with monkeypatch.context() as patch:
        patch.setattr(expm_batch, 'PASS_BYTES', 40*(8*rows*N*N + 8*N*N + 4))
        patch.setattr(expm_batch._lib, 'load', lambda: Counting())
        split = ff.exponentiate_cumulant_functions(pool[:257])
    assert calls == [40]*6 + [17] and np.array_equal(split, whole)


def test_lanes_of_one_wavefront_with_different_squarings():
    """N = 4, one matrix per lane: neighbours that need 0, 1 and 7 squarings (a divergent trip count) do not touch
    each other's arithmetic."""
    rng = np.random.default_rng(5)
    norms = np.resize([0.3, 0.8, 40.0], 64)
    assert [numeric_squarings(x) for x in (0.3, 0.8, 40.0)] == [0, 1, 7]
    tiles = random_tiles(rng, 64, 1, 4, norms)
    got = both(tiles)
    for i in range(64):
        assert np.array_equal(both(tiles[i:i + 1])[0], got[i]), i
    uniform = both(np.repeat(tiles[2:3], 64, axis=0))
    assert all(np.array_equal(u, got[2]) for u in uniform)


def numeric_squarings(norm):
    s = 0
    while norm > 0.5:
        norm *= 0.5
        s += 1
    return s


# ---- not finite ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [4, 16, 5])
def test_matrices_that_are_not_finite_are_flagged_alone(N):
    rng = np.random.default_rng(N)
    clean = random_tiles(rng, 10, 2, N, [0.3, 2.0, 11.0])
    want = both(clean)
    for kind in ('nan', 'inf in the sum alone'):
        tiles = clean.copy()
        if kind == 'nan':
            tiles[3, 1, N - 1, 0] = np.nan
        else:
            tiles[3, 0, 0, N - 1], tiles[3, 1, 0, N - 1] = 1.7e308, 1.7e308           # finite tiles, Inf in their sum
            assert np.isfinite(tiles).all()
        out, flags = entry(tiles)
        assert flags.tolist() == [0, 0, 0, 1] + [0]*6, kind
        keep = np.arange(10) != 3
        assert np.array_equal(out[keep], want[keep]), kind
        # the Python function: the single function's answer for the flagged one, whatever it does with it
        try:
            with np.errstate(over='ignore'):
                single = numeric.error_transfer_matrix(cumulant_function=tiles[3])
        except Exception as error:      # noqa: BLE001  (SciPy may refuse a matrix that is not finite: then so does the call)
            with pytest.raises(type(error)):
                ff.exponentiate_cumulant_functions(tiles)
            continue
        got = ff.exponentiate_cumulant_functions(tiles)
        assert np.array_equal(got[keep], want[keep]) and np.array_equal(got[3], single, equal_nan=True)

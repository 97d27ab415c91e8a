"""The yardstick of the batched exponential's tests: mpmath's matrix exponential at 50 digits, closed forms to check it
against, and test matrices on a fixed-point grid -- their tiles add up without rounding in any order, so the matrix a
kernel exponentiates is known exactly, its 1-norm can be put exactly at and next to a squaring boundary, and the
yardstick of one matrix serves every split of it into tiles."""
import math

import mpmath
import numpy as np

DIGITS = 50


def expm50(K):
    """exp(K) of a real matrix at 50 digits, rounded to double."""
    K = np.asarray(K, dtype=np.float64)
    with mpmath.workprec(int(DIGITS*math.log2(10)) + 8):
        U = mpmath.expm(mpmath.matrix(K.tolist()))
        return np.array([[float(U[i, j]) for j in range(K.shape[1])] for i in range(K.shape[0])])


def plane_rotation(N, theta, i=0, j=None):
    """(theta J, exp(theta J)) with J[i, j] = -1, J[j, i] = +1: the rotation by +theta in the plane (i, j), N >= 2.  Not
    symmetric: a transposed operand anywhere in the products gives the rotation by -theta."""
    j = N - 1 if j is None else j
    K = np.zeros((N, N))
    K[i, j], K[j, i] = -theta, theta
    U = np.eye(N)
    U[i, i] = U[j, j] = math.cos(theta)
    U[i, j], U[j, i] = -math.sin(theta), math.sin(theta)
    return K, U


def nilpotent_block(N, seed=0, largest=40):
    """(K, I + K) with non-zero small integers only in the block i < N/2, j >= N/2: K K = 0, so every step of scaling,
    Taylor polynomial and squaring is exact in double."""
    rng = np.random.default_rng(seed)
    K = np.zeros((N, N))
    h = N//2
    K[:h, h:] = rng.integers(1, largest + 1, (h, N - h))*rng.choice([-1.0, 1.0], (h, N - h))
    K[0, N - 1] = largest
    return K, np.eye(N) + K


def closed_forms(N):
    """(name, K, exp K) whose exponential is known in closed form."""
    diagonal = np.linspace(-3.0, 2.5, N)
    return [('diagonal', np.diag(diagonal), np.diag(np.exp(diagonal))),
            ('rotation 0.3',) + plane_rotation(N, 0.3), ('rotation 20',) + plane_rotation(N, 20.0, 1, N - 2),
            ('nilpotent',) + nilpotent_block(N)]


def one_norm(K):
    return np.abs(K).sum(axis=0).max()


def grid_matrix(rng, N, norm):
    """A random non-symmetric N x N matrix of multiples of q = 2^(floor(log2 norm) - 40) whose 1-norm is exactly the
    multiple of q next to *norm* (one column holds it, the others stay below 0.9 of it): (K, its norm, q)."""
    q = 2.0**(math.floor(math.log2(norm)) - 40)
    norm = round(norm/q)*q
    K = rng.standard_normal((N, N))
    K = np.round(K*(0.9*norm/one_norm(K))/q)*q
    j = int(np.abs(K).sum(axis=0).argmax())
    K[:, j] = np.round(K[:, j]*0.95/q)*q                   # (room for the entry that takes the rest)
    rest = norm - np.abs(K[:, j]).sum()
    assert rest > 0
    K[0, j] += rest if K[0, j] >= 0 else -rest
    assert one_norm(K) == norm and (np.round(K/q) == K/q).all()
    return K, norm, q


def grid_tiles(rng, K, rows, q):
    """*rows* tiles of multiples of q that add up to K without rounding, in any order."""
    scale = max(one_norm(K)/len(K), q)
    parts = [np.round(rng.standard_normal(K.shape)*scale/q)*q for _ in range(rows - 1)]
    tiles = np.stack(parts + [K - sum(parts, np.zeros_like(K))])
    total = np.zeros_like(K)
    for t in tiles:
        total = total + t
    assert np.array_equal(total, K) and np.array_equal(tiles.sum(axis=0), K)
    return tiles


#: the 1-norms of the accuracy cases: tiny, at and on both sides of the squaring boundaries 1/2 and 1, and large
NORMS = (1e-12, 0.5 - 2.0**-42, 0.5, 0.5 + 2.0**-41, 1.0 - 2.0**-41, 1.0, 1.0 + 2.0**-40, 3.0, 20.0, 50.0)

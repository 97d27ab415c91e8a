"""The batched pass (ff.get_filter_functions / ff.infidelities -> ffk_pipeline_batch_dev) at ragged shapes and with
incomplete bases: every member's control matrix against the oracle, its filter function and infidelities against
long-double sums of the oracle's control matrix, and everything against the single-pulse path on a twin pulse.

What the back half of the batched pass has of its own -- a chunk length that divides G so that no chunk straddles two
pulses, the accumulate kernels over the P G segments laid end to end, W_a folded for all of them, the expansion that
reduces each pulse's own slab of partial sums, the integral with the pulse as a grid axis, P single passes inside
the call where the shape leaves the fused route -- is what the shapes below are chosen for.  Every test prints its
worst error per quantity before it asserts."""
import numpy as np
import pytest

import ff_oracle as orc
import filter_functions_amd as ff
import workloads as wl
from conftest import rel_err
from filter_functions_amd import _lib, batch, util

pytestmark = pytest.mark.gpu

LD, CLD = np.longdouble, np.clongdouble
TIGHT = 2e-13                       # batched against single path (tests/test_batch_gpu.py)
BLOCK = {2: 512, 4: 768, 8: 1024}   # threads of the dimension's own accumulate kernel


class Figures:
    """The figures of one test: the worst value per quantity, printed before anything is asserted."""

    def __init__(self):
        self.worst, self.missed = {}, []

    def bar(self, name, value, bound, where=None, inclusive=False):
        value = float(value)
        if not value <= self.worst.get(name, -1.0):          # (a NaN replaces everything and stays)
            self.worst[name] = value
        if not (value <= bound if inclusive else value < bound):
            self.missed.append((name, value, bound, where))

    def close(self, label):
        print(f'{label}: ' + ' '.join(f'{k}={v:.2e}' for k, v in sorted(self.worst.items())))
        assert not self.missed, self.missed[:8]


def basis_for(d, kind):
    """'pauli' / 'ggm': complete; an int n: the first n elements of the dimension's Pauli (d = 8, 16) or GGM basis."""
    qubits = {2: 1, 4: 2, 8: 3, 16: 4}
    if kind == 'pauli':
        return ff.Basis.pauli(qubits[d])
    if kind == 'ggm':
        return ff.Basis.ggm(d)
    full = ff.Basis.pauli(qubits[d]) if d in (8, 16) else ff.Basis.ggm(d)
    return ff.Basis(full[:kind])


class Family:
    """P pulses of one shape: amplitudes, durations, control and noise operators and noise coefficients of their own
    (workloads.random_pulse_inputs, one seed per member), one basis and one frequency grid.  Member `idle` (never
    the first) has a segment with H = 0: fully degenerate."""

    def __init__(self, d, G, A, W, P, basis, seed=0):
        self.d, self.G, self.A, self.W, self.P = d, G, A, W, P
        self.basis = basis_for(d, basis)
        self.inputs = [wl.random_pulse_inputs(seed=1000*seed + 7919*d + 31*G + p, d=d, G=G, A=A, n_cops=3)
                       for p in range(P)]
        self.idle = 1 if P <= 16 else P//2
        self.inputs[self.idle][1][:, G//2] = 0.0
        self.n_ids = np.array([f'B_{a:02d}' for a in range(A)])
        self.c_ids = np.array([f'A_{i}' for i in range(3)])
        if W == 1:
            self.omega = np.array([0.3])
        else:
            self.omega = np.concatenate(([0.0], np.geomspace(1e-3, 50, W - 1)))
            if W > 4:
                # x = omega + dE = 0 (to rounding) for one entry of member 0's first segment
                c_opers, c_coeffs = self.inputs[0][:2]
                D0 = np.linalg.eigvalsh(np.einsum('ijk,i->jk', c_opers, c_coeffs[:, 0]))
                self.omega[3] = D0[1] - D0[0]
        # all members, or the first, the last and three in between (the idle one among them)
        self.checked = list(range(P)) if P <= 16 else [0, P//4, P//2, 3*P//4, P - 1]
        self._reference = {}

    def pulse(self, p, scale=1.0):
        c_opers, c_coeffs, n_opers, n_coeffs, dt = self.inputs[p]
        return ff.PulseSequence.from_arrays(c_opers, self.c_ids, c_coeffs, n_opers, self.n_ids, n_coeffs*scale, dt,
                                            self.basis)

    def pulses(self):
        """A fresh list: the batched route takes only pulses with nothing cached."""
        return [self.pulse(p) for p in range(self.P)]

    def reference(self, p, pulse):
        """(R_ref, F_ref) of member p: the oracle's control matrix from the member's own eigensystem and
        propagators, and F_ref[a,b,w] = sum_k conj(R_ref[a,k,w]) R_ref[b,k,w] summed in long double.  Computed once."""
        if p not in self._reference:
            c_opers, c_coeffs, n_opers, n_coeffs, dt = self.inputs[p]
            R_ref = orc.control_matrix_from_scratch(pulse.eigvals, pulse.eigvecs, pulse.propagators, self.omega,
                                                    np.asarray(self.basis), n_opers, n_coeffs, dt)
            R_ld = R_ref.astype(CLD)
            F_ref = np.einsum('akw,bkw->abw', R_ld.conj(), R_ld)
            for x in (R_ref, F_ref):
                x.flags.writeable = False
            self._reference[p] = (R_ref, F_ref)
        return self._reference[p]

    def spectra(self, n_idx):
        """Spectra of one, two and three dimensions, finite at omega = 0; the last complex, Hermitian in its
        operator indices and positive on the diagonal."""
        w = self.omega
        S1 = 1e-3/(1 + w)
        a = np.arange(n_idx)
        S2 = (1 + a)[:, None]*S1*(1 + 0.5*np.cos(np.outer(a, w)))
        rng = np.random.default_rng(n_idx)
        X = rng.standard_normal((n_idx, n_idx)) + 1j*rng.standard_normal((n_idx, n_idx))
        M = X @ X.conj().T + n_idx*np.eye(n_idx)
        S3 = M[:, :, None]*S1*np.exp(0.2j*(a[:, None] - a[None, :])[:, :, None]*w)
        return [S1, S2, S3]


def trapezoid_weights(omega):
    """c_w / 2 pi of the trapezoid rule in long double (the weights gamma_weights of
    tests/test_sequence_prefixes_gpu.py builds, without the spectrum)."""
    x = omega.astype(LD)
    c = np.zeros(len(x), dtype=LD)
    c[1:] += np.diff(x)/2
    c[:-1] += np.diff(x)/2
    return c/(8*np.arctan(LD(1)))


def infidelity_reference(F_ref, S, omega, idx, d):
    """(1 / 2 pi d) int S F dw on F_ref, in long double: (n_idx,) or, for a spectrum of three dimensions,
    (n_idx, n_idx)."""
    idx = np.asarray(idx)
    c = trapezoid_weights(omega)
    S = np.asarray(S)
    if S.ndim == 3:
        integrand = (F_ref[idx[:, None], idx, :]*S.astype(CLD)).real
    else:
        integrand = F_ref[idx, idx, :].real*np.broadcast_to(S, (len(idx), len(omega))).astype(LD)
    return (integrand*c).sum(axis=-1)/LD(d)


def column_error(R, R_ref):
    """max over frequencies of max|R - R_ref| / max|R_ref| of the column (inf for an error in a zero column)."""
    num = np.abs(R - R_ref).max(axis=(0, 1))
    den = np.abs(R_ref).max(axis=(0, 1))
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(den > 0, num/den, np.where(num > 0, np.inf, 0.0))
    return ratio.max()


def run_batch(family, pulses, spectrum=None, ids=None):
    """The batched call; at W = 1, which ff.get_filter_functions leaves to the single route (a grid of one point
    has no integral), the pass itself."""
    if family.W == 1:
        for pulse in pulses:
            pulse.omega = family.omega
        return batch._run_pass(pulses, list(range(len(pulses))), pulses[0].omega, np.asarray(family.basis))[0]
    if spectrum is None:
        return ff.get_filter_functions(pulses, family.omega)
    return ff.infidelities(pulses, spectrum, family.omega, n_oper_identifiers=ids)


def check_route(family, pulses, fused, per_pulse_chunks=None):
    """Every pulse is a member of one batch, in input order; the launch recorded is that of the route the case
    names: the fused route records its one accumulate launch over P G segments (no flop model: 0), the P single
    passes leave the last pass's own."""
    P, G, d = family.P, family.G, family.d
    members = [pulse._resident for pulse in pulses]
    assert all(isinstance(m, batch._Member) for m in members)
    assert all(m.batch is members[0].batch for m in members) and [m.slot for m in members] == list(range(P))
    st = _lib.stats()
    assert (st['accumulate_flops'] == 0) == fused, st
    if fused:
        assert st['chunks'] >= P and st['chunks'] % P == 0 and st['grid_z'] == st['chunks'], st
        assert G % (st['chunks']//P) == 0, st                # no chunk straddles two pulses
        if d in BLOCK:
            assert st['block'] == BLOCK[d], st
        if per_pulse_chunks == 'one':
            assert st['chunks'] == P, st
        elif per_pulse_chunks == 'several':
            assert st['chunks']//P > 1, st
    return st


def check_family(family, fused, per_pulse_chunks=None, label=''):
    fig = Figures()
    d, A, W, omega = family.d, family.A, family.W, family.omega
    N = len(family.basis)
    pulses = family.pulses()
    F = run_batch(family, pulses)
    st = check_route(family, pulses, fused, per_pulse_chunks)
    assert F.shape == (family.P, A, A, W) and F.dtype == np.complex128
    R = {}
    for p in family.checked:
        pulse = pulses[p]
        R[p] = pulse.get_control_matrix(omega)
        assert R[p].shape == (A, N, W)
        R_ref, F_ref = family.reference(p, pulse)
        # control matrix against the oracle: the norm, and frequency by frequency, so that one wrong column of a
        # ragged last tile cannot hide behind the norm of the rest
        fig.bar('R', rel_err(R[p], R_ref), 1e-12, p)
        fig.bar('R_column', column_error(R[p], R_ref), 1e-11, p, inclusive=True)
        # filter function against the long-double sum
        scale = float(np.abs(F_ref).max())
        fig.bar('F', rel_err(F[p], F_ref), 1e-12, p)
        fig.bar('F_hermitian', np.abs(F[p] - F[p].conj().transpose(1, 0, 2)).max()/scale, 1e-15, p, inclusive=True)
        diag = F[p][np.arange(A), np.arange(A)]
        assert (diag.imag == 0).all() and (diag.real >= 0).all(), p
        # the single path on the twin
        twin = family.pulse(p)
        fig.bar('F_single', rel_err(F[p], twin.get_filter_function(omega)), TIGHT, p)
        fig.bar('R_single', rel_err(R[p], twin.get_control_matrix(omega)), TIGHT, p)
    if W >= 2:
        calls = [(S, None) for S in family.spectra(A)]
        if A >= 2:
            # a subset of the identifiers, not in sorted order
            sub = [A - 1, 0] if A == 2 else [A - 1, 0, A//2]
            calls += [(S, [family.n_ids[a] for a in sub]) for S in family.spectra(len(sub))[1:]]
        for S, ids in calls:
            idx = np.arange(A) if ids is None else util.get_indices_from_identifiers(family.n_ids, ids)
            assert ids is None or list(idx) == sub
            members = family.pulses()
            got = run_batch(family, members, S, ids)
            assert got.shape == (family.P,) + (len(idx),)*(2 if S.ndim == 3 else 1) and got.dtype == np.float64
            assert all(isinstance(m._resident, batch._Member) for m in members)
            name = f'infid_{S.ndim}d' + ('' if ids is None else '_subset')
            for p in family.checked:
                # (the batch's own F of this call is the one of the first call: same inputs, same launches)
                _, F_ref = family.reference(p, pulses[p])
                fig.bar(name, rel_err(got[p], infidelity_reference(F_ref, S, omega, idx, d)), 1e-12, p)
                want = ff.infidelity(family.pulse(p), S, omega, n_oper_identifiers=ids)
                fig.bar(name + '_single', rel_err(got[p], want), TIGHT, p)
    fig.close(f'{label} d={d} G={family.G} A={A} W={W} P={family.P} N={N} chunks={st["chunks"]} block={st["block"]}')


# (G, A, W, P, fused route?, chunks per pulse the case claims)
D4 = [
    (1, 1, 1, 2, True, 'one'),            # one segment, one operator (a group of one), one frequency
    (3, 2, 17, 300, True, 'one'),         # many pulses on the grid axis; oracle on five members
    (16, 3, 64, 2, True, None),           # the front chunk exactly, a full frequency tile
    (17, 7, 33, 5, True, None),           # one segment past the front chunk; groups 3 + 2 + 2
    (97, 3, 70, 2, True, 'one'),          # G prime: the divisor search falls to one chunk per pulse; ragged second tile
    (100, 4, 64, 2, True, 'several'),     # the search steps down to a divisor above one; groups 2 + 2
    (96, 5, 130, 3, True, 'several'),     # several chunks per pulse, three pulses, groups 3 + 2, ragged third tile
    (64, 10, 31, 2, True, None),          # groups 3 + 3 + 2 + 2; chunks longer than the ring of eight tiles
]


@pytest.mark.parametrize('G,A,W,P,fused,per_pulse', D4)
def test_d4_batch_ragged_shapes(G, A, W, P, fused, per_pulse):
    """ctrl_pq.hip in the batch: groups of 3 / 2 / 1 operators, a ring of eight tiles, four producers."""
    check_family(Family(4, G, A, W, P, 'pauli'), fused, per_pulse, 'd4')


D2 = [
    (1, 1, 2, 3, True, 'one'),            # one segment, the shortest grid with an integral
    (7, 4, 65, 4, True, None),            # fewer segments than wavefronts; groups 2 + 2; one frequency past a tile
    (130, 3, 200, 2, True, None),         # several chunks per pulse, ragged sub-chunks of the wavefronts
    (1024, 2, 40, 2, True, None),         # the last G of the fused front
    (1025, 2, 40, 2, False, None),        # the first G that runs P single passes inside the call
]


@pytest.mark.parametrize('G,A,W,P,fused,per_pulse', D2)
def test_d2_batch_ragged_shapes(G, A, W, P, fused, per_pulse):
    """ctrl_d2.hip in the batch: eight wavefronts split a chunk and add up through LDS."""
    check_family(Family(2, G, A, W, P, 'pauli'), fused, per_pulse, 'd2')


D8 = [
    (5, 4, 65, 2, 'pauli', True),         # complete basis, A (N + d^2) = 512: the last shape expand_ff_pulses takes
    (9, 5, 33, 2, 'pauli', False),        # A (N + d^2) = 640: P single passes
    (33, 3, 7, 3, 'pauli', True),         # fold_w8 over P G = 99 segments, less than half a frequency tile
    (6, 13, 70, 2, 16, False),            # incomplete basis: 13 (16 + 64) 256 B = 260 KiB of tiles, single passes
    (6, 9, 40, 2, 16, False),             # incomplete basis: 180 KiB of tiles, where A 2 N alone promised 72 KiB
    (6, 6, 40, 2, 16, True),              # incomplete basis: 120 KiB, the last A of N = 16 the fused expansion takes
]


@pytest.mark.parametrize('G,A,W,P,basis,fused', D8)
def test_d8_batch_ragged_shapes(G, A, W, P, basis, fused):
    """ctrl_pcr.hip in the batch, W_a folded over P G segments; bases of 64 and of 16 elements.  (While the
    predicate of the fused expansion looked at A and N alone, the launch refused the N = 16 shapes with A = 9 and
    13, and the d = 16 shape with A = 3 below, with an error: batched and, for the fused F, on the single path.)"""
    check_family(Family(8, G, A, W, P, basis), fused, None, 'd8')


MFMA = [
    (12, 6, 1, 20, 2, 'ggm', True),       # d = 12, its own matrix-core kernel, no epilogue in the batch
    (16, 4, 1, 16, 2, 'pauli', True),     # A (N + d^2) = 512
    (16, 3, 3, 16, 2, 16, False),         # incomplete basis: 204 KiB of tiles, where A 2 N alone promised 24 KiB
    (16, 3, 2, 9, 2, 16, False),          # incomplete basis: 136 KiB of tiles, above the predicate's 128 KiB
    (16, 3, 1, 9, 2, 16, True),           # incomplete basis in the fused expansion: partials 16 x the R tile
]


@pytest.mark.parametrize('d,G,A,W,P,basis,fused', MFMA)
def test_d12_d16_batch_ragged_shapes(d, G, A, W, P, basis, fused):
    """ctrl_mfma.hip in the batch."""
    check_family(Family(d, G, A, W, P, basis), fused, None, 'mfma')


OTHER = [
    (3, 9, 2, 31, 3, 'ggm', True),        # N = 9: ragged against the basis tile of 8
    (3, 9, 2, 31, 3, 5, True),            # N = 5 < d^2: ragged against the basis tile of 4
    (5, 6, 4, 22, 2, 'ggm', True),
    (6, 4, 2, 17, 2, 'ggm', True),
    (7, 12, 3, 40, 2, 'ggm', True),       # no padded route in the batch: d = 7's own kernel
    (11, 5, 2, 19, 2, 'ggm', True),       # likewise d = 11
    (13, 4, 2, 17, 2, 'ggm', False),      # A (N + d^2) = 676: single passes
    (13, 4, 1, 17, 2, 'ggm', True),       # d = 13's own kernel in the batch
]


@pytest.mark.parametrize('d,G,A,W,P,basis,fused', OTHER)
def test_other_dimensions_batch_ragged_shapes(d, G, A, W, P, basis, fused):
    """The templated kernel of every other dimension, each its own instantiation."""
    check_family(Family(d, G, A, W, P, basis), fused, None, 'other')


def test_several_passes_on_the_device(monkeypatch):
    """A list split over several passes: every pass its own batch, the results in input order."""
    family = Family(4, 20, 3, 70, 7, 'pauli', seed=1)
    omega, A, d = family.omega, family.A, family.d
    S = family.spectra(A)[1]
    single = [(t.get_filter_function(omega), t.get_control_matrix(omega))
              for t in (family.pulse(p) for p in range(7))]
    single_infid = [ff.infidelity(family.pulse(p), S, omega) for p in range(7)]
    # (split_passes: sizes that differ by one at most; a budget of one byte still gives passes of two pulses at most)
    for name, value, sizes in (('MAX_PULSES', 3, [2, 2, 3]), ('PASS_BYTES', 1, [1, 2, 2, 2])):
        fig = Figures()
        with monkeypatch.context() as patch:
            patch.setattr(batch, name, value)
            pulses = family.pulses()
            F = ff.get_filter_functions(pulses, omega)
            members = family.pulses()
            infid = ff.infidelities(members, S, omega)
        for group in (pulses, members):
            assert all(isinstance(pulse._resident, batch._Member) for pulse in group)
            # consecutive members share a pass, members of different passes hold different batches
            batches = []
            for pulse in group:
                if not batches or batches[-1][0] is not pulse._resident.batch:
                    batches.append((pulse._resident.batch, []))
                batches[-1][1].append(pulse._resident.slot)
            assert len({id(b) for b, _ in batches}) == len(batches)
            assert [len(slots) for _, slots in batches] == sizes
            assert all(slots == list(range(len(slots))) for _, slots in batches)
        for p in range(7):
            R = pulses[p].get_control_matrix(omega)
            R_ref, F_ref = family.reference(p, pulses[p])
            fig.bar('R', rel_err(R, R_ref), 1e-12, p)
            fig.bar('R_column', column_error(R, R_ref), 1e-11, p, inclusive=True)
            fig.bar('F', rel_err(F[p], F_ref), 1e-12, p)
            fig.bar('infid', rel_err(infid[p], infidelity_reference(F_ref, S, omega, np.arange(A), d)), 1e-12, p)
            fig.bar('F_single', rel_err(F[p], single[p][0]), TIGHT, p)
            fig.bar('R_single', rel_err(R, single[p][1]), TIGHT, p)
            fig.bar('infid_single', rel_err(infid[p], single_infid[p]), TIGHT, p)
        fig.close(f'passes {name}={value}')


def test_no_member_touches_a_neighbour():
    """Members 1 and 2 of four replaced by pulses 1e150 times as loud: members 0 and 3 come out bit for bit (the
    chunk count per pulse depends on P alone), the loud ones finite and 1e150 times their originals."""
    family = Family(4, 17, 5, 33, 4, 'pauli', seed=2)
    omega = family.omega
    S = family.spectra(family.A)[0]

    def evaluate(scales):
        pulses = [family.pulse(p, scale) for p, scale in enumerate(scales)]
        F = np.array(ff.get_filter_functions(pulses, omega))
        R = np.array([pulse.get_control_matrix(omega) for pulse in pulses])
        infid = ff.infidelities([family.pulse(p, scale) for p, scale in enumerate(scales)], S, omega)
        return R, F, infid
    quiet = evaluate([1.0, 1.0, 1.0, 1.0])
    loud = evaluate([1.0, 1e150, 1e150, 1.0])
    fig = Figures()
    for p in (0, 3):
        for a, b in zip(quiet, loud):
            assert np.array_equal(a[p], b[p]), p
    for p in (1, 2):
        assert all(np.isfinite(x[p]).all() for x in loud), p
        fig.bar('R_scaled', rel_err(loud[0][p]/1e150, quiet[0][p]), TIGHT, p)
        fig.bar('F_scaled', rel_err(loud[1][p]/1e300, quiet[1][p]), TIGHT, p)
        fig.bar('infid_scaled', rel_err(loud[2][p]/1e300, quiet[2][p]), TIGHT, p)
    fig.close('neighbours')

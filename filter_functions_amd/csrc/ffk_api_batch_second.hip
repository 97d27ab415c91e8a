// ffk_api_batch_second.hip -- the frequency shifts of P pulses of one shape in ONE pass (ffk_batch_frequency_shifts;
// kernels: second.hip, so_shift_kernel).  A host-pointer entry on StagedCall: every input array crosses in one copy
// of its own (pulse-major, so their number does not depend on P), the launches follow on the same stream without a
// synchronisation, the result comes back in one copy.  The second-order filter function is never in memory.
// ffk_frequency_shifts_from_scratch (ffk_api_frozen.hip) and its kernels are untouched.
#include "ffk_api_common.h"

namespace {

// the scratch of one pass in the order it is sliced; per-pulse arrays hold P times `one` elements
struct ShiftScratch {
    size_t segtab, Tc, ops, nt, bt, NB, M, partial;      // elements per pulse (doubles; cplx for Tc .. M)
};
ShiftScratch shift_scratch(int W, int N, int A, int G, int d, size_t n_out) {
    const size_t dd = size_t(d)*d;
    const int chunk = ffk::so_shift_chunk(W, N, A, G, d);
    const size_t FB = chunk ? (size_t(W) + chunk - 1)/chunk : 0;
    return {size_t(G)*ffk::seg_stride(d), size_t(G)*dd, size_t(G)*(1 + A)*dd, size_t(A)*G*dd, size_t(G)*N*dd,
            size_t(G)*A*N*dd, size_t(G)*A*N*dd, FB*n_out*N*N};
}
bool shift_shape_ok(int W, int N, int A, int G, int d) {
    return W >= 1 && N >= 1 && A >= 1 && G >= 1 && d_templated_ok(d) && size_t(A)*N <= 65535 &&
           ffk::so_shift_chunk(W, N, A, G, d) > 0 && ffk::so_shift_tile(A*N, d) > 0;
}
size_t tile_slots(int A, int N) {
    const size_t t16 = (size_t(A)*N + 15)/16;
    return t16*t16;
}

}  // namespace

extern "C" {

int ffk_batch_frequency_shifts_chunk(int W, int N, int A, int G, int d) {
    if (!shift_shape_ok(W, N, A, G, d)) return 0;
    return ffk::so_shift_chunk(W, N, A, G, d);
}

size_t ffk_batch_frequency_shifts_workspace_bytes(int P, int W, int N, int A, int G, int d, int n_idx, int s_ndim) {
    if (P < 1 || P > 65535 || n_idx < 1 || n_idx > A || s_ndim < 1 || s_ndim > 3 || !shift_shape_ok(W, N, A, G, d))
        return 0;
    // linear in P: the shared part plus P times one pulse's slices, each rounded up on its own -- an upper bound of
    // what the call declares for every P
    const SpectrumShape sh = spectrum_shape(s_ndim, n_idx);
    const size_t dd = size_t(d)*d;
    const ShiftScratch s = shift_scratch(W, N, A, G, d, sh.n_out);
    size_t shared = align_up(8*size_t(W)) + align_up(16*size_t(N)*dd) + 2*align_up(16*size_t(W)*sh.rows) +
                    align_up(4*size_t(n_idx)) + align_up(4*size_t(A)*A) + align_up(8*tile_slots(A, N));
    size_t one = align_up(8*size_t(G)*d) + align_up(16*size_t(G)*dd) + align_up(16*size_t(G + 1)*dd) +
                 align_up(16*size_t(A)*dd) + align_up(8*size_t(A)*G) + align_up(8*size_t(G)) +
                 align_up(8*(size_t(G) + 1));                                                        // inputs
    one += align_up(8*s.segtab) + align_up(16*s.Tc) + align_up(16*s.ops) + align_up(16*s.nt) + align_up(16*s.bt) +
           align_up(16*s.NB) + align_up(16*s.M) + align_up(8*s.partial) + align_up(8*sh.n_out*N*N);
    return shared + size_t(P)*one;
}

int ffk_batch_frequency_shifts(int P, const double* eigvals, const double* eigvecs, const double* propagators,
                               const double* omega, int W, const double* basis, int N, const double* n_opers, int A,
                               const double* n_coeffs, const double* dt, const double* t, int G, int d,
                               const double* spectrum, int s_ndim, const int32_t* idx, int n_idx,
                               double* frequency_shifts) {
    FFK_REQUIRE(P >= 1 && P <= 65535, "need 1 <= P <= 65535 pulses, got P=%d", P);
    FFK_REQUIRE(d_templated_ok(d), "unsupported dimension d=%d (need 2 <= d <= %d)", d, FFK_MAX_D_TEMPLATED);
    FFK_REQUIRE(W >= 1 && N >= 1 && A >= 1 && G >= 1, "empty axis: W=%d N=%d A=%d G=%d", W, N, A, G);
    FFK_REQUIRE(eigvals && eigvecs && propagators && omega && basis && n_opers && n_coeffs && dt && t && spectrum &&
                    idx && frequency_shifts, "NULL argument");
    FFK_REQUIRE(s_ndim >= 1 && s_ndim <= 3, "Expected spectrum to have < 4 dimensions, not %d", s_ndim);
    FFK_REQUIRE(n_idx >= 1 && n_idx <= A, "need 1 <= n_idx <= A distinct noise operators, got n_idx=%d", n_idx);
    for (int i = 0; i < n_idx; ++i) {
        FFK_REQUIRE(idx[i] >= 0 && idx[i] < A, "noise operator index %d out of range [0, %d)", idx[i], A);
        for (int j = 0; j < i; ++j) FFK_REQUIRE(idx[j] != idx[i], "noise operator %d selected twice", idx[i]);
    }
    FFK_REQUIRE(shift_shape_ok(W, N, A, G, d),
                "the batched frequency shifts take the shapes of the matrix-core kernel only: d=%d A*N=%d", d, A*N);
    const int mt = ffk::so_shift_tile(A*N, d);
    std::vector<int32_t> pair_slot(size_t(A)*A), tiles(2*tile_slots(A, N));
    const int ntiles = ffk::so_shift_plan(A, N, mt, s_ndim, idx, n_idx, pair_slot.data(), tiles.data());
    FFK_REQUIRE(ntiles >= 1 && ntiles <= 65535, "%d tiles: too many for one pass", ntiles);

    const SpectrumShape sh = spectrum_shape(s_ndim, n_idx);
    const size_t dd = size_t(d)*d, p = size_t(P);
    const ShiftScratch s = shift_scratch(W, N, A, G, d, sh.n_out);
    StagedCall c;
    const auto D = c.in<double>(eigvals, p*G*d);
    const auto V = c.in<cplx>(eigvecs, p*G*dd);
    const auto Q = c.in<cplx>(propagators, p*(G + 1)*dd);
    const auto B = c.in<cplx>(n_opers, p*A*dd);
    const auto nc = c.in<double>(n_coeffs, p*A*G);
    const auto ddt = c.in<double>(dt, p*G);
    const auto tt = c.in<double>(t, p*(size_t(G) + 1));
    const auto om = c.in<double>(omega, W);
    const auto C = c.in<cplx>(basis, size_t(N)*dd);
    const auto S = c.in<cplx>(spectrum, size_t(W)*sh.rows);
    const auto slot = c.in<int32_t>(pair_slot.data(), pair_slot.size());
    const auto til = c.in<int32_t>(tiles.data(), tiles.size(), 2*size_t(ntiles));
    const auto scale = c.out<cplx>(size_t(W)*sh.rows);
    const auto segtab = c.out<double>(p*s.segtab);
    const auto Tc = c.out<cplx>(p*s.Tc);
    const auto ops = c.out<cplx>(p*s.ops);
    const auto nt = c.out<cplx>(p*s.nt);
    const auto bt = c.out<cplx>(p*s.bt);
    const auto NB = c.out<cplx>(p*s.NB);
    const auto M = c.out<cplx>(p*s.M);
    const auto partial = c.out<double>(p*s.partial);
    const auto out = c.out<double>(p*sh.n_out*N*N);
    if (int rc = c.stage()) return rc;
    FFK_REQUIRE(c[out] && c[partial] && c[M], "internal: arena too small");
    hipStream_t st = nullptr;
    FFK_HIP(ffk::launch_spectral_weights(c[S], static_cast<int>(sh.rows), W, c[om], W, 0, c[scale], st));
    FFK_HIP(ffk::launch_prologue_pulses(c[D], c[V], c[Q], c[B], c[nc], c[ddt], c[tt], G, P, d, A, c[segtab], c[Tc],
                                        c[ops], c[nt], st));
    FFK_REQUIRE(p*G <= 0x7fffffffull, "P*G too large");
    FFK_HIP(ffk::launch_basis_transformed(c[Tc], c[C], P*G, N, d, c[bt], st));
    FFK_HIP(ffk::launch_second_order_prepare_pulses(c[D], c[ddt], c[nt], c[bt], P, G, d, A, N, c[NB], c[M], st));
    FFK_HIP(ffk::launch_frequency_shifts_pulses(P, c[om], W, c[D], c[ddt], c[tt], c[NB], c[M], G, d, A, N, c[scale],
                                                s_ndim, c[slot], c[til], ntiles, static_cast<int>(sh.n_out),
                                                c[partial], c[out], st));
    if (int rc = c.copy_back(frequency_shifts, out)) return rc;
    return c.finish();
}

}  // extern "C"

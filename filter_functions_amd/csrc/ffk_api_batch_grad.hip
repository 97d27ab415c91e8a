// ffk_api_batch_grad.hip -- the gradient of the filter function / infidelity of P pulses of one shape in ONE pass
// (ffk_batch_filter_function_derivative; kernels: grad_batch.hip).  The inputs of all pulses are packed into one
// pinned staging block and cross in one H2D copy; the launches follow on the same stream without a synchronisation;
// one D2H copy per requested output.  The number of launches and copies does not depend on P.
// ffk_filter_function_derivative (ffk_api_frozen.hip) and its kernels are untouched.
#include "ffk_api_common.h"

namespace {

// the one layout of the pass: [inputs, in the order they are staged][scratch][outputs].  With base NULL it only
// measures.  The input block is the same in the pinned staging block and at the front of the device block.
struct GradBatchWs {
    double *D, *V, *Q, *om, *B, *nc, *C, *ratio, *dt, *t, *S;       // inputs
    size_t input_bytes;
    cplx *scale, *rec, *totals, *ytot;
    double *partial, *dI, *dF;
};

size_t slice_grad_batch(void* base, size_t bytes, int P, int W, int A, int H, int G, int d, int srows, bool with_ratio,
                        bool want_dI, bool want_dF, GradBatchWs* w) {
    Bump ws(base, base ? bytes : ~size_t(0)/2);
    const size_t dd = size_t(d)*d, p = size_t(P);
    const int L = ffk::grad_batch_chunk(G, d, W), C = (G + L - 1)/L, tiles = (W + 63)/64;
    *w = GradBatchWs{};
    w->D = ws.take<double>(p*G*d);
    w->V = ws.take<double>(2*p*G*dd);
    w->Q = ws.take<double>(2*p*(G + 1)*dd);
    w->B = ws.take<double>(2*p*A*dd);
    w->nc = ws.take<double>(p*A*G);
    w->C = ws.take<double>(2*p*H*dd);
    if (with_ratio) w->ratio = ws.take<double>(p*A*H*G);
    w->dt = ws.take<double>(p*G);
    w->t = ws.take<double>(p*(G + 1));
    w->om = ws.take<double>(W);
    if (srows > 0) w->S = ws.take<double>(2*size_t(srows)*W);
    w->input_bytes = ws.used;
    if (srows > 0) w->scale = ws.take<cplx>(size_t(srows)*W);
    w->rec = ws.take<cplx>(p*G*ffk::grad_batch_record_elems(d, A, H));
    w->totals = ws.take<cplx>(p*C*A*dd*W);
    w->ytot = ws.take<cplx>(p*A*dd*W);
    if (want_dI) {
        w->partial = ws.take<double>(size_t(tiles)*p*A*G*H);
        w->dI = ws.take<double>(p*A*G*H);
    }
    if (want_dF) w->dF = ws.take<double>(p*A*G*H*W);
    return ws.used;
}

// pinned staging block, grown on demand; guarded by g_arena.mu like the arena it feeds
void* g_stage = nullptr;
size_t g_stage_bytes = 0;

int stage_reserve(size_t bytes, void** out) {
    if (bytes > g_stage_bytes) {
        if (g_stage) (void)hipHostFree(g_stage);
        g_stage = nullptr;
        g_stage_bytes = 0;
        const size_t want = align_up(bytes, size_t(1) << 20);
        FFK_HIP(hipHostMalloc(&g_stage, want, 0));
        g_stage_bytes = want;
    }
    *out = g_stage;
    return FFK_OK;
}

}  // namespace

extern "C" {

int ffk_batch_filter_function_derivative_chunk(int G, int d, int W) {
    if (G < 1 || d < 2 || d > 4 || W < 1) return 0;
    return ffk::grad_batch_chunk(G, d, W);
}

size_t ffk_batch_filter_function_derivative_workspace_bytes(int P, int W, int A, int H, int G, int d, int want_dF) {
    if (!ffk::grad_batch_supported(P, W, A, H, G, d)) return 0;
    // linear in P: the shared part (frequencies, spectrum, weights: counted for a spectrum per operator) plus P times
    // one pulse's slices, each rounded up on its own -- an upper bound of the packed layout for every P
    GradBatchWs w;
    const size_t none = slice_grad_batch(nullptr, 0, 1, W, A, H, G, d, 0, false, false, false, &w);
    const size_t shared = slice_grad_batch(nullptr, 0, 1, W, A, H, G, d, A, false, false, false, &w) - none +
                          align_up(8*size_t(W));
    const size_t one = slice_grad_batch(nullptr, 0, 1, W, A, H, G, d, 0, true, true, want_dF != 0, &w) -
                       align_up(8*size_t(W));
    return shared + size_t(P)*one;
}

int ffk_batch_filter_function_derivative(int P, const double* eigvals, const double* eigvecs,
                                         const double* propagators, const double* omega, int W,
                                         const double* n_opers, int A, const double* n_coeffs,
                                         const double* c_opers, int H, const double* n_coeffs_ratio,
                                         const double* dt, const double* t, int G, int d, const double* spectrum,
                                         int s_ndim, double* filter_function_derivative,
                                         double* infidelity_derivative) {
    FFK_REQUIRE(P >= 1 && P <= 65535, "need 1 <= P <= 65535 pulses, got P=%d", P);
    FFK_REQUIRE(d >= 2 && d <= 4, "the batched gradient kernels support 2 <= d <= 4, not d=%d", d);
    FFK_REQUIRE(W >= 1 && A >= 1 && H >= 1 && G >= 1, "empty axis: W=%d A=%d H=%d G=%d", W, A, H, G);
    FFK_REQUIRE(A <= 4 && H <= 8, "the batched gradient takes A <= 4 noise and H <= 8 control operators, not A=%d H=%d",
                A, H);
    FFK_REQUIRE(eigvals && eigvecs && propagators && omega && n_opers && n_coeffs && c_opers && dt && t,
                "NULL argument");
    FFK_REQUIRE(filter_function_derivative || infidelity_derivative, "no output requested");
    FFK_REQUIRE(!infidelity_derivative || (spectrum && (s_ndim == 1 || s_ndim == 2)),
                "infidelity derivative needs a spectrum of shape (W,) or (A, W)");
    FFK_REQUIRE(ffk::grad_batch_supported(P, W, A, H, G, d), "shape too large for one pass: W=%d G=%d", W, G);
    const bool want_dI = infidelity_derivative != nullptr, want_dF = filter_function_derivative != nullptr;
    const int srows = want_dI ? (s_ndim == 2 ? A : 1) : 0;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    GradBatchWs m;
    const size_t total = slice_grad_batch(nullptr, 0, P, W, A, H, G, d, srows, n_coeffs_ratio != nullptr, want_dI,
                                          want_dF, &m);
    void *base, *stage;
    if (int rc = arena_reserve(total, &base)) return rc;
    if (int rc = stage_reserve(m.input_bytes, &stage)) return rc;
    GradBatchWs h, w;
    slice_grad_batch(stage, m.input_bytes, P, W, A, H, G, d, srows, n_coeffs_ratio != nullptr, false, false, &h);
    slice_grad_batch(base, g_arena.size, P, W, A, H, G, d, srows, n_coeffs_ratio != nullptr, want_dI, want_dF, &w);
    FFK_REQUIRE(w.ytot && (!want_dI || w.dI) && (!want_dF || w.dF), "internal: arena too small");
    const size_t dd = size_t(d)*d, p = size_t(P);
    std::memcpy(h.D, eigvals, 8*p*G*d);
    std::memcpy(h.V, eigvecs, 16*p*G*dd);
    std::memcpy(h.Q, propagators, 16*p*(G + 1)*dd);
    std::memcpy(h.B, n_opers, 16*p*A*dd);
    std::memcpy(h.nc, n_coeffs, 8*p*A*G);
    std::memcpy(h.C, c_opers, 16*p*H*dd);
    if (n_coeffs_ratio) std::memcpy(h.ratio, n_coeffs_ratio, 8*p*A*H*G);
    std::memcpy(h.dt, dt, 8*p*G);
    std::memcpy(h.t, t, 8*p*(G + 1));
    std::memcpy(h.om, omega, 8*size_t(W));
    if (srows > 0) std::memcpy(h.S, spectrum, 16*size_t(srows)*W);
    hipStream_t st = nullptr;
    StreamDrain drain{st};
    FFK_HIP(hipMemcpyAsync(base, stage, m.input_bytes, hipMemcpyHostToDevice, st));
    if (want_dI)
        FFK_HIP(ffk::launch_spectral_weights(reinterpret_cast<const cplx*>(w.S), srows, W, w.om, W, 0, w.scale, st));
    FFK_HIP(ffk::launch_grad_batch(P, w.D, reinterpret_cast<const cplx*>(w.V), reinterpret_cast<const cplx*>(w.Q),
                                   w.om, W, reinterpret_cast<const cplx*>(w.B), A, w.nc,
                                   reinterpret_cast<const cplx*>(w.C), H, w.ratio, w.dt, w.t, G, d, w.scale, s_ndim,
                                   w.rec, w.totals, w.ytot, w.partial, w.dF, w.dI, st));
    if (want_dI)
        FFK_HIP(hipMemcpyAsync(infidelity_derivative, w.dI, 8*p*A*G*H, hipMemcpyDeviceToHost, st));
    if (want_dF)
        FFK_HIP(hipMemcpyAsync(filter_function_derivative, w.dF, 8*p*A*G*H*W, hipMemcpyDeviceToHost, st));
    FFK_HIP(hipStreamSynchronize(st));
    return FFK_OK;
}

}  // extern "C"

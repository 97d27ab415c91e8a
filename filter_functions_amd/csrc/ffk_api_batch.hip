// ffk_api_batch.hip -- P pulses of one shape in ONE pass (ffk_pipeline_batch_dev): one launch per stage, the pulse a
// grid axis, every per-pulse array pulse-major.  Shared by all pulses: the frequency grid, the basis, the spectrum and
// idx.  The single-pulse entry points and their kernels are untouched.
//
// Stages (fused front: use_fused_front(G, d) and expand_ff_supported(A, N, d)):
//   eigh_expm_controls_pulses  (G, P)     H summed from the pulse's own controls, eigensystem, segment propagators
//   scan_local_pulses          (chunks, P) chunk-local prefix products; a chunk never straddles two pulses
//   apply_prologue_pulses      (G + N, P) scan fix-up from the pulse's own chunk totals + prologue; basis compacted once
//   fold_w8 (d = 8)            (P G, A)   per segment: the P G segments laid end to end
//   accumulate (the single-pulse kernels, unchanged) over the P G segments with a chunk length that divides G: every
//              grid.z slab lies inside one pulse, Ypart comes out (P, chunks/P, A, d, d, W)
//   expand_ff_pulses           (W/16, P)  R (P, A, N, W), F (P, A, A, W)
//   infid_pulses               (nout, P)  on the shared spectrum
// Other shapes run P single passes of the pipeline on the stream inside the call (header comment of include/ffk.h).
#include "ffk_api_common.h"

namespace ffk_api {
namespace {

bool batch_fused(int W, int N, int A, int G, int d) {
    return ffk::use_fused_front(G, d) && ffk::expand_ff_supported(A, N, d);
}

struct BatchWs {
    int* status;                 // (P, G) eigensolver flags: FIRST, ffk_eigensolver_status_batch_dev reads them
    cplx* seg_prop;              // fused: (P, G, d, d)
    cplx* qloc;                  //        (P, G+1, d, d)
    cplx* totals;                //        (P, nchunks, d, d)
    double* segtab;              //        (P, G, seg_stride)
    cplx* Tc;                    //        (P, G, d, d)
    cplx* ops;                   //        (P, G, 1+A, d, d)
    cplx* Ypart;                 //        (P, chunks/P, A, d, d, W)
    void* ews;                   //        compacted basis
    cplx* wfold;                 //        d = 4, 8: folded operands of the accumulate kernel
    cplx* H;                     // single passes: (P, G, d, d)
    void* single;                //                one pass's pipeline workspace, reused pulse after pulse
    size_t single_bytes;
    double *D, *V, *Q, *R, *F;   // outputs the caller did not ask for
};

// The one slicing of the workspace: with base NULL it only measures (every optional output counted); returns the
// bytes used.  NULL members: not part of this shape's layout.
size_t slice_batch_ws(void* base, size_t bytes, int P, int W, int N, int A, int G, int d, const bool want[5],
                      BatchWs* w) {
    Bump ws(base, base ? bytes : ~size_t(0)/2);
    const size_t dd = size_t(d)*d, PG = size_t(P)*G;
    *w = BatchWs{};
    w->status = ws.take<int>(PG);
    if (batch_fused(W, N, A, G, d)) {
        const int L = ffk::front_chunk(d);
        const size_t nch = size_t(G + L - 1)/L;
        const ffk::AccumGeometry geo = ffk::accumulate_geometry_pulses(W, A, G, d, P);
        w->seg_prop = ws.take<cplx>(PG*dd);
        w->qloc = ws.take<cplx>(size_t(P)*(G + 1)*dd);
        w->totals = ws.take<cplx>(size_t(P)*nch*dd);
        w->segtab = ws.take<double>(PG*ffk::seg_stride(d));
        w->Tc = ws.take<cplx>(PG*dd);
        w->ops = ws.take<cplx>(PG*(1 + A)*dd);
        w->Ypart = ws.take<cplx>(size_t(geo.chunks)*A*dd*W);
        w->ews = ws.take<unsigned char>(ffk::expand_workspace_bytes(N, d));
        if (d == 4 || d == 8) w->wfold = ws.take<cplx>(ffk::wfold_elems(d, G, A, W, 1)*P);
    } else {
        w->H = ws.take<cplx>(PG*dd);
        w->single_bytes = ffk_pipeline_workspace_bytes(W, N, A, G, d, 0, 0);
        w->single = ws.take<unsigned char>(w->single_bytes);
    }
    if (want[0]) w->D = ws.take<double>(PG*d);
    if (want[1]) w->V = ws.take<double>(2*PG*dd);
    if (want[2]) w->Q = ws.take<double>(2*size_t(P)*(G + 1)*dd);
    if (want[3]) w->R = ws.take<double>(2*size_t(P)*A*N*W);
    if (want[4]) w->F = ws.take<double>(2*size_t(P)*A*A*W);
    return ws.used;
}

size_t batch_ws_bytes(int P, int W, int N, int A, int G, int d) {
    const bool all[5] = {true, true, true, true, true};
    BatchWs w;
    return slice_batch_ws(nullptr, 0, P, W, N, A, G, d, all, &w);
}

}  // namespace

int pipeline_batch_dev_impl(int P, const double* c_opers, int n_cops, const double* c_coeffs, const double* dt,
                            const double* t, int G, int d, const double* omega, int W, const double* basis, int N,
                            const double* n_opers, int A, const double* n_coeffs, const double* spectrum, int s_ndim,
                            const int32_t* idx, int n_idx, int d_infidelity, double* eigvals, double* eigvecs,
                            double* propagators, double* control_matrix, double* filter_function, double* infid,
                            void* workspace, size_t workspace_bytes, void* stream) {
    FFK_REQUIRE(P >= 1 && P <= 65535, "need 1 <= P <= 65535 pulses, got P=%d", P);
    FFK_REQUIRE(d_templated_ok(d), "unsupported dimension d=%d (need 2 <= d <= %d)", d, FFK_MAX_D_TEMPLATED);
    FFK_REQUIRE(W >= 1 && N >= 1 && A >= 1 && G >= 1 && n_cops >= 1, "empty axis: W=%d N=%d A=%d G=%d n_cops=%d", W,
                N, A, G, n_cops);
    FFK_REQUIRE(c_opers && c_coeffs && dt && t && omega && basis && n_opers && n_coeffs && workspace,
                "NULL argument");
    const bool want_infid = spectrum != nullptr && infid != nullptr;
    FFK_REQUIRE(!want_infid || (idx && n_idx >= 1 && s_ndim >= 1 && s_ndim <= 3 && d_infidelity >= 1),
                "bad spectrum arguments");
    FFK_REQUIRE(workspace_bytes >= ffk_pipeline_batch_workspace_bytes(P, W, N, A, G, d, n_idx, s_ndim),
                "workspace too small");
    const bool want[5] = {!eigvals, !eigvecs, !propagators, !control_matrix, !filter_function};
    BatchWs w;
    slice_batch_ws(workspace, workspace_bytes, P, W, N, A, G, d, want, &w);
    double* D = eigvals ? eigvals : w.D;
    double* V = eigvecs ? eigvecs : w.V;
    double* Q = propagators ? propagators : w.Q;
    double* R = control_matrix ? control_matrix : w.R;
    double* F = filter_function ? filter_function : w.F;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t dd = size_t(d)*d;
    const cplx* Cop = reinterpret_cast<const cplx*>(c_opers);
    if (batch_fused(W, N, A, G, d)) {
        FFK_HIP(ffk::launch_eigh_expm_controls_pulses(Cop, c_coeffs, n_cops, dt, G, P, d, D,
                                                      reinterpret_cast<cplx*>(V), w.seg_prop, w.status, s));
        FFK_HIP(ffk::launch_scan_local_pulses(w.seg_prop, G, P, d, ffk::front_chunk(d), w.qloc, w.totals, s));
        FFK_HIP(ffk::launch_apply_prologue_compact_pulses(
            w.qloc, w.totals, G, P, d, reinterpret_cast<cplx*>(Q), D, reinterpret_cast<const cplx*>(V),
            reinterpret_cast<const cplx*>(n_opers), n_coeffs, dt, t, A, w.segtab, w.Tc, w.ops,
            reinterpret_cast<const cplx*>(basis), N, w.ews, s, w.wfold));
        const ffk::AccumGeometry geo = ffk::accumulate_geometry_pulses(W, A, G, d, P);
        // (no expansion epilogue: it needs one chunk in the whole launch; no padded route: wfold only where the
        // dimension's own kernel reads it)
        FFK_HIP(ffk::launch_accumulate(omega, W, w.segtab, w.ops, P*G, d, A, geo, w.Ypart, s, nullptr, nullptr,
                                       w.wfold));
        g_stats.accumulate_flops = 0.0;         // (no model of the batched launch; include/ffk.h)
        record_accumulate_launch(W, A, P*G, d, geo);
        FFK_HIP(ffk::launch_expand_ff_pulses(w.Ypart, geo.chunks/P, size_t(A)*dd*W, A, N, d, W, P,
                                             reinterpret_cast<cplx*>(R), reinterpret_cast<cplx*>(F), w.ews, s));
    } else {
        FFK_HIP(ffk::launch_assemble_hamiltonians_pulses(Cop, c_coeffs, n_cops, G, P, d, w.H, s));
        const DiagWs sw = slice_diag_ws(w.single, w.single_bytes, G, d);
        for (int p = 0; p < P; ++p) {
            PassOptions opt;
            if (int rc = pipeline_dev_impl(reinterpret_cast<const double*>(w.H + size_t(p)*G*dd), dt + size_t(p)*G,
                                           t + size_t(p)*(G + 1), G, d, omega, W, basis, N,
                                           n_opers + 2*size_t(p)*A*dd, A, n_coeffs + size_t(p)*A*G, nullptr, 0,
                                           nullptr, 0, D + size_t(p)*G*d, V + 2*size_t(p)*G*dd,
                                           Q + 2*size_t(p)*(G + 1)*dd, R + 2*size_t(p)*A*N*W,
                                           F + 2*size_t(p)*A*A*W, nullptr, w.single, w.single_bytes, stream, opt))
                return rc;
            FFK_HIP(hipMemcpyAsync(w.status + size_t(p)*G, sw.status, sizeof(int)*size_t(G),
                                   hipMemcpyDeviceToDevice, s));
        }
    }
    if (want_infid)
        FFK_HIP(ffk::launch_infidelity_pulses(reinterpret_cast<const cplx*>(F), A, W, P,
                                              reinterpret_cast<const cplx*>(spectrum), s_ndim, omega, idx, n_idx,
                                              d_infidelity, infid, s));
    return FFK_OK;
}

}  // namespace ffk_api

extern "C" {

size_t ffk_pipeline_batch_workspace_bytes(int P, int W, int N, int A, int G, int d, int n_idx, int s_ndim) {
    (void)n_idx;
    (void)s_ndim;     // (the integral needs no scratch)
    if (P < 1 || W < 1 || N < 1 || A < 1 || G < 1 || !d_templated_ok(d)) return 0;
    return batch_ws_bytes(P, W, N, A, G, d);
}

int ffk_pipeline_batch_dev(int P, const double* c_opers, int n_cops, const double* c_coeffs, const double* dt,
                           const double* t, int G, int d, const double* omega, int W, const double* basis, int N,
                           const double* n_opers, int A, const double* n_coeffs, const double* spectrum, int s_ndim,
                           const int32_t* idx, int n_idx, double* eigvals, double* eigvecs, double* propagators,
                           double* control_matrix, double* filter_function, double* infid, void* workspace,
                           size_t workspace_bytes, void* stream) {
    return pipeline_batch_dev_impl(P, c_opers, n_cops, c_coeffs, dt, t, G, d, omega, W, basis, N, n_opers, A,
                                   n_coeffs, spectrum, s_ndim, idx, n_idx, d, eigvals, eigvecs, propagators,
                                   control_matrix, filter_function, infid, workspace, workspace_bytes, stream);
}

int ffk_eigensolver_status_batch_dev(const void* workspace, size_t workspace_bytes, int P, int G, int d,
                                     int32_t* n_failed, void* stream) {
    FFK_REQUIRE(workspace && n_failed && P >= 1 && P <= 65535 && G >= 1 && d_templated_ok(d), "bad argument");
    FFK_REQUIRE(workspace_bytes >= align_up(sizeof(int)*size_t(P)*G), "workspace too small");
    // the flags are the first slice of the batch workspace
    FFK_HIP(ffk::launch_count_failures_pulses(static_cast<const int*>(workspace), G, P, n_failed,
                                              static_cast<hipStream_t>(stream)));
    return FFK_OK;
}

}  // extern "C"

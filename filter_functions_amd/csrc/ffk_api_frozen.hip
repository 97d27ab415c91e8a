// ffk_api_frozen.hip -- extern "C" entry points OUTSIDE SURVEY section 8's scope table, frozen since
// round 2 and exercised by the `slow` tests only: second-order filter function, frequency shifts and
// their cumulant-function contribution; the gradient of the filter function / infidelity.
#include "ffk_api_common.h"

extern "C" {

// ---------------------------------------------------------------------------------------------
// second order: filter function, frequency shifts, cumulant-function contribution
// ---------------------------------------------------------------------------------------------
static int second_order_impl(const double* eigvals, const double* eigvecs,
                             const double* propagators, const double* omega, int W,
                             const double* basis, int N, const double* n_opers, int A,
                             const double* n_coeffs, const double* dt, const double* t, int G, int d,
                             double* filter_function_2, const double* spectrum, int s_ndim,
                             const int32_t* idx, int n_idx, double* frequency_shifts) {
    FFK_REQUIRE(d_templated_ok(d), "unsupported dimension d=%d (need 2 <= d <= %d)", d, FFK_MAX_D_TEMPLATED);
    FFK_REQUIRE(W >= 1 && N >= 1 && A >= 1 && G >= 1, "empty axis: W=%d N=%d A=%d G=%d", W, N, A, G);
    FFK_REQUIRE(eigvals && eigvecs && propagators && omega && basis && n_opers && n_coeffs && dt && t,
                "NULL argument");
    FFK_REQUIRE(filter_function_2 || frequency_shifts, "no output requested");
    FFK_REQUIRE(size_t(A)*N <= 65535, "A*N = %zu too large", size_t(A)*N);
    if (frequency_shifts) {
        FFK_REQUIRE(spectrum && idx, "NULL argument");
        FFK_REQUIRE(s_ndim >= 1 && s_ndim <= 3, "Expected spectrum to have < 4 dimensions, not %d", s_ndim);
        FFK_REQUIRE(n_idx >= 1, "empty axis");
        for (int i = 0; i < n_idx; ++i)
            FFK_REQUIRE(idx[i] >= 0 && idx[i] < A, "noise operator index %d out of range [0, %d)", idx[i], A);
    }
    StagedCall c;
    const SpectrumShape sh = frequency_shifts ? spectrum_shape(s_ndim, n_idx) : SpectrumShape{};
    const size_t wsb = ffk_second_order_workspace_bytes(W, N, A, G, d);
    const size_t swsb = frequency_shifts ? ffk_frequency_shifts_workspace_bytes(W, n_idx, s_ndim) : 0;
    const PulseSlices p = stage_pulse(c, eigvals, eigvecs, propagators, omega, W, basis, N, n_opers, A, n_coeffs, dt,
                                      t, G, d);
    const auto F = c.out<double>(2*size_t(A)*A*N*N*W);
    const auto ws = c.workspace(wsb);
    const auto S = c.in<double>(spectrum, 2*size_t(W)*sh.rows);
    const auto didx = c.in<int32_t>(idx, frequency_shifts ? n_idx : 0);
    const auto shifts = c.out<double>(sh.n_out*N*N);
    const auto sws = c.out<unsigned char>(swsb);
    if (int rc = c.stage()) return rc;
    if (int rc = ffk_second_order_filter_function_dev(c[p.eigvals], c[p.eigvecs], c[p.propagators], c[p.omega], W,
                                                      c[p.basis], N, c[p.n_opers], A, c[p.n_coeffs], c[p.dt], c[p.t],
                                                      G, d, c[F], c[ws], wsb, nullptr))
        return rc;
    if (frequency_shifts) {
        if (int rc = ffk_frequency_shifts_shard_dev(c[F], A, N, W, c[S], s_ndim, c[p.omega], W, 0, c[didx], n_idx,
                                                    c[shifts], c[sws], swsb, nullptr))
            return rc;
        if (int rc = c.copy_back(frequency_shifts, shifts)) return rc;
    }
    if (filter_function_2)
        if (int rc = c.copy_back(filter_function_2, F)) return rc;
    return c.finish();
}

int ffk_second_order_filter_function(const double* eigvals, const double* eigvecs,
                                     const double* propagators, const double* omega, int W,
                                     const double* basis, int N, const double* n_opers, int A,
                                     const double* n_coeffs, const double* dt, const double* t, int G,
                                     int d, double* filter_function_2) {
    FFK_REQUIRE(filter_function_2, "NULL argument");
    return second_order_impl(eigvals, eigvecs, propagators, omega, W, basis, N, n_opers, A, n_coeffs, dt,
                             t, G, d, filter_function_2, nullptr, 0, nullptr, 0, nullptr);
}

int ffk_frequency_shifts_from_scratch(const double* eigvals, const double* eigvecs,
                                      const double* propagators, const double* omega, int W,
                                      const double* basis, int N, const double* n_opers, int A,
                                      const double* n_coeffs, const double* dt, const double* t, int G,
                                      int d, const double* spectrum, int s_ndim, const int32_t* idx,
                                      int n_idx, double* filter_function_2, double* frequency_shifts) {
    FFK_REQUIRE(frequency_shifts, "NULL argument");
    return second_order_impl(eigvals, eigvecs, propagators, omega, W, basis, N, n_opers, A, n_coeffs, dt,
                             t, G, d, filter_function_2, spectrum, s_ndim, idx, n_idx, frequency_shifts);
}

int ffk_second_order_filter_function_from_atomic(const double* filter_function_atomic,
                                                 const double* control_matrix_step,
                                                 const double* propagators_liouville, int G, int A,
                                                 int N, int W, double* filter_function_2) {
    FFK_REQUIRE(filter_function_atomic && control_matrix_step && filter_function_2, "NULL argument");
    FFK_REQUIRE(G >= 1 && A >= 1 && N >= 1 && W >= 1, "empty axis: G=%d A=%d N=%d W=%d", G, A, N, W);
    FFK_REQUIRE(G == 1 || propagators_liouville, "NULL argument");
    StagedCall c;
    const size_t nl = G > 1 ? G - 1 : 1;
    const auto Fa = c.in<cplx>(filter_function_atomic, size_t(G)*A*A*N*N*W);
    const auto R = c.in<cplx>(control_matrix_step, size_t(G)*A*N*W);
    const auto L = c.in<double>(propagators_liouville, nl*N*N, size_t(G - 1)*N*N);
    const auto ws = c.workspace(ffk::second_order_from_atomic_workspace_bytes(G, A, N, W));
    const auto out = c.out<cplx>(size_t(A)*A*N*N*W);
    if (int rc = c.stage()) return rc;
    FFK_HIP(ffk::launch_second_order_from_atomic(c[Fa], c[R], c[L], G, A, N, W, c[out], c[ws], nullptr));
    if (int rc = c.copy_back(filter_function_2, out)) return rc;
    return c.finish();
}

int ffk_frequency_shifts(const double* filter_function_2, int A, int N, int W, const double* spectrum,
                         int s_ndim, const double* omega, const int32_t* idx, int n_idx,
                         double* frequency_shifts) {
    FFK_REQUIRE(filter_function_2 && spectrum && omega && idx && frequency_shifts, "NULL argument");
    FFK_REQUIRE(s_ndim >= 1 && s_ndim <= 3, "Expected spectrum to have < 4 dimensions, not %d", s_ndim);
    FFK_REQUIRE(A >= 1 && N >= 1 && W >= 1 && n_idx >= 1, "empty axis");
    for (int i = 0; i < n_idx; ++i)
        FFK_REQUIRE(idx[i] >= 0 && idx[i] < A, "noise operator index %d out of range [0, %d)", idx[i], A);
    StagedCall c;
    const SpectrumShape sh = spectrum_shape(s_ndim, n_idx);
    const size_t wsb = ffk_frequency_shifts_workspace_bytes(W, n_idx, s_ndim);
    const auto F = c.in<double>(filter_function_2, 2*size_t(A)*A*N*N*W);
    const auto S = c.in<double>(spectrum, 2*size_t(W)*sh.rows);
    const auto om = c.in<double>(omega, W);
    const auto didx = c.in<int32_t>(idx, n_idx);
    const auto out = c.out<double>(sh.n_out*N*N);
    const auto ws = c.workspace(wsb);
    if (int rc = c.stage()) return rc;
    if (int rc = ffk_frequency_shifts_shard_dev(c[F], A, N, W, c[S], s_ndim, c[om], W, 0, c[didx], n_idx, c[out],
                                                c[ws], wsb, nullptr))
        return rc;
    if (int rc = c.copy_back(frequency_shifts, out)) return rc;
    return c.finish();
}

int ffk_cumulant_function_second_order(const double* frequency_shifts, int batch, int N, int d,
                                       const double* basis, double* cumulant_function) {
    FFK_REQUIRE(frequency_shifts && basis && cumulant_function, "NULL argument");
    FFK_REQUIRE(batch >= 1 && N >= 1, "empty axis");
    FFK_REQUIRE(d_templated_ok(d), "dimension %d outside [2, %d]", d, FFK_MAX_D_TEMPLATED);
    StagedCall c;
    const size_t wsb = ffk_cumulant_function_second_order_workspace_bytes(batch, N, d);
    const auto D = c.in<double>(frequency_shifts, size_t(batch)*N*N);
    const auto K = c.in<double>(cumulant_function, size_t(batch)*N*N);      // added to in place
    const auto B = c.in<double>(basis, 2*size_t(N)*d*d);
    const auto ws = c.workspace(wsb);
    if (int rc = c.stage()) return rc;
    if (int rc = ffk_cumulant_function_second_order_dev(c[D], batch, N, d, c[B], c[K], c[ws], wsb, nullptr))
        return rc;
    if (int rc = c.copy_back(cumulant_function, K)) return rc;
    return c.finish();
}

size_t ffk_second_order_workspace_bytes(int W, int N, int A, int G, int d) {
    if (W < 1 || N < 1 || A < 1 || G < 1 || !d_templated_ok(d)) return 0;
    const size_t dd = size_t(d)*d;
    size_t b = 0;
    b += align_up(8*size_t(G)*ffk::seg_stride(d)) + align_up(16*size_t(G)*dd);        // segtab, Tc
    b += align_up(16*size_t(G)*(1 + A)*dd);                                           // ops
    b += align_up(16*size_t(A)*G*dd) + align_up(16*size_t(G)*dd);                     // nt, ep
    b += align_up(16*size_t(G)*N*dd);                                                 // bt
    b += ffk::second_order_workspace_bytes(G, A, N, d);                               // NB, M
    return b;
}

int ffk_second_order_filter_function_dev(const double* eigvals, const double* eigvecs,
                                         const double* propagators, const double* omega, int W,
                                         const double* basis, int N, const double* n_opers, int A,
                                         const double* n_coeffs, const double* dt, const double* t,
                                         int G, int d, double* filter_function_2, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    FFK_REQUIRE(d_templated_ok(d), "unsupported dimension d=%d (need 2 <= d <= %d)", d, FFK_MAX_D_TEMPLATED);
    FFK_REQUIRE(W >= 1 && N >= 1 && A >= 1 && G >= 1, "empty axis: W=%d N=%d A=%d G=%d", W, N, A, G);
    FFK_REQUIRE(eigvals && eigvecs && propagators && omega && basis && n_opers && n_coeffs && dt && t &&
                    filter_function_2 && workspace, "NULL argument");
    FFK_REQUIRE(size_t(A)*N <= 65535, "A*N = %zu too large", size_t(A)*N);
    FFK_REQUIRE(workspace_bytes >= ffk_second_order_workspace_bytes(W, N, A, G, d), "workspace too small");
    const size_t dd = size_t(d)*d;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Bump a(workspace, workspace_bytes);
    double* segtab = a.take<double>(size_t(G)*ffk::seg_stride(d));
    cplx* Tc = a.take<cplx>(size_t(G)*dd);
    cplx* ops = a.take<cplx>(size_t(G)*(1 + A)*dd);
    cplx* dnt = a.take<cplx>(size_t(A)*G*dd);
    cplx* dep = a.take<cplx>(size_t(G)*dd);
    cplx* dbt = a.take<cplx>(size_t(G)*N*dd);
    void* ws = a.take<unsigned char>(ffk::second_order_workspace_bytes(G, A, N, d));
    FFK_REQUIRE(ws, "internal: workspace too small");
    FFK_HIP(ffk::launch_prologue(eigvals, reinterpret_cast<const cplx*>(eigvecs),
                                 reinterpret_cast<const cplx*>(propagators),
                                 reinterpret_cast<const cplx*>(n_opers), n_coeffs, dt, t, G, d, A, segtab,
                                 Tc, ops, dnt, dep, st));
    FFK_HIP(ffk::launch_basis_transformed(Tc, reinterpret_cast<const cplx*>(basis), G, N, d, dbt, st));
    FFK_HIP(ffk::launch_second_order_filter_function(omega, W, eigvals, dt, t, dnt, dbt, G, d, A, N,
                                                     reinterpret_cast<cplx*>(filter_function_2), ws, st));
    return FFK_OK;
}

size_t ffk_frequency_shifts_workspace_bytes(int W, int n_idx, int s_ndim) {
    if (W < 1 || n_idx < 1 || s_ndim < 1 || s_ndim > 3) return 0;
    return align_up(16*size_t(W)*spectrum_shape(s_ndim, n_idx).rows);
}

int ffk_frequency_shifts_shard_dev(const double* filter_function_2, int A, int N, int W_block,
                                   const double* spectrum, int s_ndim, const double* omega, int W,
                                   int w_offset, const int32_t* idx, int n_idx,
                                   double* frequency_shifts, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    FFK_REQUIRE(filter_function_2 && spectrum && omega && idx && frequency_shifts && workspace,
                "NULL argument");
    FFK_REQUIRE(s_ndim >= 1 && s_ndim <= 3, "Expected spectrum to have < 4 dimensions, not %d", s_ndim);
    FFK_REQUIRE(A >= 1 && N >= 1 && W_block >= 1 && n_idx >= 1, "empty axis");
    FFK_REQUIRE(w_offset >= 0 && w_offset + W_block <= W, "frequency block [%d, %d) outside [0, %d)",
                w_offset, w_offset + W_block, W);
    FFK_REQUIRE(workspace_bytes >= ffk_frequency_shifts_workspace_bytes(W_block, n_idx, s_ndim),
                "workspace too small");
    const int rows = static_cast<int>(spectrum_shape(s_ndim, n_idx).rows);
    hipStream_t st = static_cast<hipStream_t>(stream);
    cplx* scale = static_cast<cplx*>(workspace);
    FFK_HIP(ffk::launch_spectral_weights(reinterpret_cast<const cplx*>(spectrum), rows, W_block, omega, W,
                                         w_offset, scale, st));
    FFK_HIP(ffk::launch_frequency_shifts(reinterpret_cast<const cplx*>(filter_function_2), A, N, W_block,
                                         scale, s_ndim, idx, n_idx, frequency_shifts, st));
    return FFK_OK;
}

size_t ffk_cumulant_function_second_order_workspace_bytes(int batch, int N, int d) {
    if (batch < 1 || N < 1 || !d_templated_ok(d)) return 0;
    return align_up(ffk::cumulant_second_order_workspace_bytes(batch, N, d));
}

int ffk_cumulant_function_second_order_dev(const double* frequency_shifts, int batch, int N, int d,
                                           const double* basis, double* cumulant_function,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    FFK_REQUIRE(frequency_shifts && basis && cumulant_function && workspace, "NULL argument");
    FFK_REQUIRE(batch >= 1 && N >= 1, "empty axis");
    FFK_REQUIRE(d_templated_ok(d), "dimension %d outside [2, %d]", d, FFK_MAX_D_TEMPLATED);
    FFK_REQUIRE(workspace_bytes >= ffk_cumulant_function_second_order_workspace_bytes(batch, N, d),
                "workspace too small");
    FFK_HIP(ffk::launch_cumulant_second_order(frequency_shifts, batch, N, d,
                                              reinterpret_cast<const cplx*>(basis), cumulant_function,
                                              workspace, static_cast<hipStream_t>(stream)));
    return FFK_OK;
}

// ---------------------------------------------------------------------------------------------
// gradient: derivative of the filter function / infidelity w.r.t. the control amplitudes
// ---------------------------------------------------------------------------------------------
}  // extern "C"
namespace {
// What every gradient starts from, on stream `st` with its temporaries from `ws`: Bbar, T of the noise operators and
// Abar of the control operators (unit coefficients), the Hilbert-space steps of the interaction-picture noise
// operators, one chunk per segment, and their running sums.
struct GradientFront {
    cplx *ops, *abar, *E, *Y;
};
size_t gradient_front_bytes(int W, int A, int H, int G, int d) {
    const size_t dd = size_t(d)*d;
    const int HA = H > A ? H : A;
    size_t b = 0;
    b += 2*(align_up(8*size_t(G)*ffk::seg_stride(d)) + align_up(16*size_t(G)*dd) +
            align_up(16*size_t(G)*(1 + HA)*dd));                                   // segtab, Tc, ops (x2)
    b += align_up(16*size_t(A)*G*dd) + align_up(16*size_t(H)*G*dd) + 2*align_up(16*size_t(G)*dd);
    b += align_up(16*size_t(H)*G*dd);                                              // E
    b += align_up(16*size_t(G)*A*dd*W);                                            // Y steps / Ycum
    return b;
}
int gradient_front(const double* eigvals, const double* eigvecs, const double* propagators, const double* omega,
                   int W, const double* n_opers, int A, const double* n_coeffs, const double* c_opers, int H,
                   const double* dt, const double* t, int G, int d, Bump& ws, hipStream_t st, GradientFront* out) {
    const size_t dd = size_t(d)*d;
    const int HA = H > A ? H : A;
    double* segtab = ws.take<double>(size_t(G)*ffk::seg_stride(d));
    cplx* Tc = ws.take<cplx>(size_t(G)*dd);
    cplx* ops = ws.take<cplx>(size_t(G)*(1 + HA)*dd);
    double* segtab2 = ws.take<double>(size_t(G)*ffk::seg_stride(d));
    cplx* Tc2 = ws.take<cplx>(size_t(G)*dd);
    cplx* ops2 = ws.take<cplx>(size_t(G)*(1 + HA)*dd);
    cplx* dnt = ws.take<cplx>(size_t(A)*G*dd);
    cplx* dabar = ws.take<cplx>(size_t(H)*G*dd);
    cplx* dep = ws.take<cplx>(size_t(G)*dd);
    cplx* dep2 = ws.take<cplx>(size_t(G)*dd);
    cplx* dE = ws.take<cplx>(size_t(H)*G*dd);
    cplx* Y = ws.take<cplx>(size_t(G)*A*dd*W);
    FFK_REQUIRE(segtab && Tc && ops && segtab2 && Tc2 && ops2 && dnt && dabar && dep && dep2 && dE && Y,
                "internal: workspace too small");
    const cplx* V = reinterpret_cast<const cplx*>(eigvecs);
    const cplx* Q = reinterpret_cast<const cplx*>(propagators);
    FFK_HIP(ffk::launch_prologue(eigvals, V, Q, reinterpret_cast<const cplx*>(n_opers), n_coeffs, dt, t, G,
                                 d, A, segtab, Tc, ops, dnt, dep, st));
    FFK_HIP(ffk::launch_prologue(eigvals, V, Q, reinterpret_cast<const cplx*>(c_opers), nullptr, dt, t, G,
                                 d, H, segtab2, Tc2, ops2, dabar, dep2, st));
    ffk::AccumGeometry geo = ffk::accumulate_geometry(W, A, G, d, G);
    FFK_HIP(ffk::launch_accumulate(omega, W, segtab, ops, G, d, A, geo, Y, st));
    FFK_HIP(ffk::launch_segment_prefix_sum(Y, G, size_t(A)*dd*W, st));
    *out = {ops, dabar, dE, Y};
    return FFK_OK;
}
}  // namespace
extern "C" {

int ffk_filter_function_derivative(const double* eigvals, const double* eigvecs,
                                   const double* propagators, const double* omega, int W,
                                   const double* n_opers, int A, const double* n_coeffs,
                                   const double* c_opers, int H, const double* n_coeffs_ratio,
                                   const double* dt, const double* t, int G, int d,
                                   const double* spectrum, int s_ndim,
                                   double* filter_function_derivative,
                                   double* infidelity_derivative) {
    FFK_REQUIRE(d >= 2 && d <= 8, "the gradient kernels support 2 <= d <= 8, not d=%d", d);
    FFK_REQUIRE(W >= 1 && A >= 1 && H >= 1 && G >= 1, "empty axis: W=%d A=%d H=%d G=%d", W, A, H, G);
    FFK_REQUIRE(eigvals && eigvecs && propagators && omega && n_opers && n_coeffs && c_opers && dt && t,
                "NULL argument");
    FFK_REQUIRE(filter_function_derivative || infidelity_derivative, "no output requested");
    FFK_REQUIRE(!infidelity_derivative || (spectrum && (s_ndim == 1 || s_ndim == 2)),
                "infidelity derivative needs a spectrum of shape (W,) or (A, W)");
    FFK_REQUIRE(size_t(G)*A <= 65535, "G*A = %zu too large", size_t(G)*A);
    StagedCall c;
    const bool want_dI = infidelity_derivative != nullptr;
    const size_t wsb = ffk_filter_function_derivative_workspace_bytes(W, A, H, G, d);
    const PulseSlices p = stage_pulse(c, eigvals, eigvecs, propagators, omega, W, nullptr, 0, n_opers, A, n_coeffs,
                                      dt, t, G, d);
    const auto cop = c.in<double>(c_opers, 2*size_t(H)*d*d);
    const auto ratio = c.in<double>(n_coeffs_ratio, size_t(A)*H*G);
    const auto S = c.in<double>(spectrum, want_dI ? 2*size_t(W)*(s_ndim == 2 ? A : 1) : 0);
    const auto dF = c.out<double>(size_t(A)*G*H*W);      // the device pass always writes it
    const auto dI = c.out<double>(size_t(A)*G*H);
    const auto ws = c.workspace(wsb);
    if (int rc = c.stage()) return rc;
    if (int rc = ffk_filter_function_derivative_shard_dev(
            c[p.eigvals], c[p.eigvecs], c[p.propagators], c[p.omega], W, c[p.n_opers], A, c[p.n_coeffs], c[cop], H,
            n_coeffs_ratio ? c[ratio] : nullptr, c[p.dt], c[p.t], G, d, want_dI ? c[S] : nullptr, s_ndim, c[p.omega],
            W, 0, c[dF], want_dI ? c[dI] : nullptr, c[ws], wsb, nullptr))
        return rc;
    if (want_dI)
        if (int rc = c.copy_back(infidelity_derivative, dI)) return rc;
    if (filter_function_derivative)
        if (int rc = c.copy_back(filter_function_derivative, dF)) return rc;
    return c.finish_with_fault_status();
}

int ffk_control_matrix_derivative(const double* eigvals, const double* eigvecs, const double* propagators,
                                  const double* omega, int W, const double* basis, int N,
                                  const double* n_opers, int A, const double* n_coeffs,
                                  const double* c_opers, int H, const double* n_coeffs_ratio,
                                  const double* dt, const double* t, int G, int d,
                                  double* control_matrix_derivative) {
    FFK_REQUIRE(d >= 2 && d <= 8, "the gradient kernels support 2 <= d <= 8, not d=%d", d);
    FFK_REQUIRE(W >= 1 && A >= 1 && H >= 1 && G >= 1 && N >= 1, "empty axis: W=%d A=%d H=%d G=%d N=%d", W,
                A, H, G, N);
    FFK_REQUIRE(eigvals && eigvecs && propagators && omega && basis && n_opers && n_coeffs && c_opers && dt &&
                    t && control_matrix_derivative, "NULL argument");
    FFK_REQUIRE(size_t(G)*A <= 65535, "G*A = %zu too large", size_t(G)*A);
    StagedCall c;
    const PulseSlices p = stage_pulse(c, eigvals, eigvecs, propagators, omega, W, basis, N, n_opers, A, n_coeffs, dt,
                                      t, G, d);
    const auto cop = c.in<double>(c_opers, 2*size_t(H)*d*d);
    const auto ratio = c.in<double>(n_coeffs_ratio, size_t(A)*H*G);
    const auto R = c.out<cplx>(size_t(H)*W*G*A*N);
    const auto ws = c.workspace(gradient_front_bytes(W, A, H, G, d));
    if (int rc = c.stage()) return rc;
    Bump a = c.bump(ws);
    GradientFront f;
    if (int rc = gradient_front(c[p.eigvals], c[p.eigvecs], c[p.propagators], c[p.omega], W, c[p.n_opers], A,
                                c[p.n_coeffs], c[cop], H, c[p.dt], c[p.t], G, d, a, nullptr, &f))
        return rc;
    FFK_HIP(ffk::launch_control_matrix_derivative(c[p.omega], W, c[p.eigvals], c[p.dt], c[p.t], f.ops, f.abar, f.Y,
                                                  n_coeffs_ratio ? c[ratio] : nullptr,
                                                  reinterpret_cast<const cplx*>(c[p.basis]), N, G, d, A, H, f.E,
                                                  c[R], nullptr));
    if (int rc = c.copy_back(control_matrix_derivative, R)) return rc;
    return c.finish_with_fault_status();
}

int ffk_filter_function_derivative_from_control_matrix(const double* control_matrix,
                                                       const double* control_matrix_derivative, int A,
                                                       int N, int W, int G, int H,
                                                       double* filter_function_derivative) {
    FFK_REQUIRE(control_matrix && control_matrix_derivative && filter_function_derivative, "NULL argument");
    FFK_REQUIRE(A >= 1 && N >= 1 && W >= 1 && G >= 1 && H >= 1, "empty axis: A=%d N=%d W=%d G=%d H=%d", A, N,
                W, G, H);
    StagedCall c;
    const auto R = c.in<cplx>(control_matrix, size_t(A)*N*W);
    const auto D = c.in<cplx>(control_matrix_derivative, size_t(H)*W*G*A*N);
    const auto F = c.out<double>(size_t(A)*G*H*W);
    if (int rc = c.stage()) return rc;
    FFK_HIP(ffk::launch_filter_function_derivative_from_control_matrix(c[R], c[D], A, N, W, G, H, c[F], nullptr));
    if (int rc = c.copy_back(filter_function_derivative, F)) return rc;
    return c.finish();
}

size_t ffk_filter_function_derivative_workspace_bytes(int W, int A, int H, int G, int d) {
    if (W < 1 || A < 1 || H < 1 || G < 1 || d < 2 || d > 8) return 0;
    return gradient_front_bytes(W, A, H, G, d) + align_up(16*size_t(W)*A);         // + spectral weights
}

int ffk_filter_function_derivative_shard_dev(const double* eigvals, const double* eigvecs,
                                             const double* propagators, const double* omega_block,
                                             int W_block, const double* n_opers, int A,
                                             const double* n_coeffs, const double* c_opers, int H,
                                             const double* n_coeffs_ratio, const double* dt,
                                             const double* t, int G, int d, const double* spectrum,
                                             int s_ndim, const double* omega, int W, int w_offset,
                                             double* filter_function_derivative,
                                             double* infidelity_derivative, void* workspace,
                                             size_t workspace_bytes, void* stream) {
    FFK_REQUIRE(d >= 2 && d <= 8, "the gradient kernels support 2 <= d <= 8, not d=%d", d);
    FFK_REQUIRE(W_block >= 1 && A >= 1 && H >= 1 && G >= 1, "empty axis");
    FFK_REQUIRE(eigvals && eigvecs && propagators && omega_block && n_opers && n_coeffs && c_opers && dt &&
                    t && filter_function_derivative && workspace, "NULL argument");
    FFK_REQUIRE(!infidelity_derivative || (spectrum && omega && (s_ndim == 1 || s_ndim == 2)),
                "infidelity derivative needs a spectrum of shape (W,) or (A, W) and the global grid");
    FFK_REQUIRE(!infidelity_derivative || (w_offset >= 0 && w_offset + W_block <= W),
                "frequency block [%d, %d) outside [0, %d)", w_offset, w_offset + W_block, W);
    FFK_REQUIRE(size_t(G)*A <= 65535, "G*A = %zu too large", size_t(G)*A);
    FFK_REQUIRE(workspace_bytes >= ffk_filter_function_derivative_workspace_bytes(W_block, A, H, G, d),
                "workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    Bump a(workspace, workspace_bytes);
    GradientFront f;
    if (int rc = gradient_front(eigvals, eigvecs, propagators, omega_block, W_block, n_opers, A, n_coeffs, c_opers,
                                H, dt, t, G, d, a, st, &f))
        return rc;
    cplx* dscale = a.take<cplx>(size_t(W_block)*A);
    FFK_REQUIRE(dscale, "internal: workspace too small");
    FFK_HIP(ffk::launch_filter_function_derivative(omega_block, W_block, eigvals, dt, t, f.ops, f.abar, f.Y,
                                                   n_coeffs_ratio, G, d, A, H, f.E,
                                                   filter_function_derivative, st));
    if (infidelity_derivative) {
        const int srows = s_ndim == 2 ? A : 1;
        FFK_HIP(ffk::launch_spectral_weights(reinterpret_cast<const cplx*>(spectrum), srows, W_block, omega,
                                             W, w_offset, dscale, st));
        FFK_HIP(ffk::launch_infidelity_derivative(filter_function_derivative, A, G, H, W_block, dscale,
                                                  s_ndim, d, infidelity_derivative, st));
    }
    return FFK_OK;
}

}  // extern "C"

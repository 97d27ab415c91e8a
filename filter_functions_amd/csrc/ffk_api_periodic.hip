// ffk_api_periodic.hip -- periodic driving of many pulses at many repeat counts in one pass (ff.periodic_*;
// periodic_batch.hip): the workspace query, the device-pointer entry and the host-pointer entry, which reads
// resident control matrices where they lie and stages everything else through StagedCall.
#include "ffk_api_common.h"

namespace {

// stage: 1 filter functions, 2 infidelities, 3 decay amplitudes
bool periodic_shape_ok(int P, int K, int n_host, int A, int W, int d, int n_ops, int s_ndim, int stage) {
    return ffk::periodic_supported(P, K, d, W, n_ops) && n_host >= 0 && n_host <= P && A >= 1 && n_ops <= A &&
           stage >= 1 && stage <= 3 && (stage == 1 || ((s_ndim == 1 || s_ndim == 2) && W >= 2));
}

size_t periodic_out_count(int P, int K, int W, int d, int n_ops, int stage) {
    const size_t rows = size_t(P)*K*n_ops, dd = size_t(d)*d;
    return stage == 1 ? rows*W : (stage == 2 ? rows : rows*dd*dd);
}

// the weights of the integral into `scale` (stage 2, 3), then the one kernel of the stage
int periodic_enqueue(const cplx* const* tab, int P, int W, int d, const double* omega, const cplx* basis,
                     const cplx* V, const double* phi, const double* period, const int32_t* repeats, int K,
                     const cplx* spectrum, int s_ndim, const int32_t* ops, int n_ops, int d_infidelity, int stage,
                     cplx* scale, double* out, hipStream_t s) {
    if (stage >= 2)
        FFK_HIP(ffk::launch_spectral_weights(spectrum, s_ndim == 1 ? 1 : n_ops, W, omega, W, 0, scale, s));
    if (stage == 3)
        FFK_HIP(ffk::launch_periodic_decay(tab, P, d, W, basis, V, phi, period, omega, repeats, K, ops, n_ops, scale,
                                           s_ndim, out, s));
    else
        FFK_HIP(ffk::launch_periodic_fejer(tab, P, d, W, basis, V, phi, period, omega, repeats, K, ops, n_ops,
                                           stage == 2 ? scale : nullptr, s_ndim, d_infidelity,
                                           stage == 1 ? out : nullptr, stage == 2 ? out : nullptr, s));
    return FFK_OK;
}

int check_periodic_host_args(const int32_t* repeats, int K, const int32_t* ops, int n_ops, int A) {
    for (int k = 0; k < K; ++k) FFK_REQUIRE(repeats[k] >= 1, "repeats[%d] = %d is below 1", k, repeats[k]);
    for (int i = 0; i < n_ops; ++i)
        FFK_REQUIRE(ops[i] >= 0 && ops[i] < A, "idx[%d] = %d outside [0, %d)", i, ops[i], A);
    return FFK_OK;
}

// ---- second order by period doubling ------------------------------------------------------------------------------
bool periodic_shifts_shape_ok(int P, int K, int S, int n_host, int A, int W, int d, int n_ops, int s_ndim) {
    return ffk::periodic_shifts_supported(P, K, S, d, W, n_ops) && n_host >= 0 && n_host <= P && A >= 1 &&
           n_ops <= A && (s_ndim == 1 || s_ndim == 2);
}

struct ShiftsScratch {
    size_t scale, tiles, table, total;
};

// the device-pointer entry's workspace: the weights, the steps' tiles, the result table
ShiftsScratch periodic_shifts_scratch(int P, int S, int W, int d, int n_ops, int s_ndim) {
    const size_t tile = 8*size_t(P)*n_ops*size_t(d)*d*d*d, rows = s_ndim == 1 ? 1 : size_t(n_ops);
    ShiftsScratch at;
    at.scale = 0;
    at.tiles = align_up(16*rows*W);
    at.table = at.tiles + align_up(tile*S);
    at.total = at.table + align_up(tile*(size_t(S) + 1));
    return at;
}

// the weights and the steps' tiles (none with S = 0: every count is 1), then the walk
int periodic_shifts_enqueue(const cplx* const* tab, int P, int W, int d, const double* omega, const cplx* basis,
                            const cplx* V, const double* phi, const double* period, const int32_t* steps, int S,
                            const int32_t* count_slots, int K, const cplx* spectrum, int s_ndim, const int32_t* ops,
                            int n_ops, const double* delta1, cplx* scale, double* tiles, double* table, double* out,
                            hipStream_t s) {
    if (S > 0) {
        FFK_HIP(ffk::launch_spectral_weights(spectrum, s_ndim == 1 ? 1 : n_ops, W, omega, W, 0, scale, s));
        FFK_HIP(ffk::launch_periodic_shift_gram(tab, P, d, W, basis, V, phi, period, omega, steps, S, ops, n_ops,
                                                scale, s_ndim, tiles, s));
    }
    FFK_HIP(ffk::launch_periodic_shift_combine(P, d, basis, V, phi, steps, S, count_slots, K, n_ops, delta1, tiles,
                                               table, out, s));
    return FFK_OK;
}

int check_periodic_shifts_host_args(const int32_t* steps, int S, const int32_t* count_slots, int K,
                                    const int32_t* ops, int n_ops, int A) {
    for (int s = 0; s < S; ++s) {
        const int32_t* step = steps + 4*s;
        FFK_REQUIRE(step[0] >= 1 && step[1] >= 1 && step[0] <= INT32_MAX - step[1],
                    "steps[%d] = (%d, %d): counts must be >= 1 and sum to at most 2^31 - 1", s, step[0], step[1]);
        FFK_REQUIRE(step[2] >= 0 && step[2] <= s && step[3] >= 0 && step[3] <= s,
                    "steps[%d] reads the slots (%d, %d), outside [0, %d]", s, step[2], step[3], s);
    }
    for (int k = 0; k < K; ++k)
        FFK_REQUIRE(count_slots[k] >= 0 && count_slots[k] <= S, "count_slots[%d] = %d outside [0, %d]", k,
                    count_slots[k], S);
    for (int i = 0; i < n_ops; ++i)
        FFK_REQUIRE(ops[i] >= 0 && ops[i] < A, "idx[%d] = %d outside [0, %d)", i, ops[i], A);
    return FFK_OK;
}

#define FFK_SHIFTS_SHAPE_MESSAGE                                                                                     \
    "unsupported shape P=%d K=%d S=%d A=%d W=%d d=%d n_idx=%d s_ndim=%d (need 1 <= P, K <= 65535, 0 <= S <= 65535, " \
    "2 <= d <= 4, 1 <= n_idx <= A, s_ndim 1 or 2 and W >= 2)"

}  // namespace

extern "C" {

size_t ffk_periodic_shifts_workspace_bytes(int P, int K, int S, int n_host, int A, int W, int d, int n_idx,
                                           int s_ndim) {
    if (!periodic_shifts_shape_ok(P, K, S, n_host, A, W, d, n_idx, s_ndim)) return 0;
    const size_t dd = size_t(d)*d, tile = 8*size_t(P)*n_idx*dd*dd;
    const size_t rows = s_ndim == 1 ? 1 : size_t(n_idx);
    size_t o = 0;
    auto put = [&o](size_t bytes) { o += align_up(bytes); };
    put(8*size_t(P));                            // pointer table
    put(8*size_t(W));                            // omega
    put(16*dd*dd);                               // basis
    put(16*size_t(P)*dd);                        // eigenvectors
    put(16*size_t(P)*dd);                        // phase differences
    put(8*size_t(P));                            // periods
    put(16*size_t(S));                           // steps
    put(4*size_t(K));                            // count slots
    put(4*size_t(n_idx));                        // idx
    put(16*rows*W);                              // spectrum
    put(16*dd*size_t(A)*W*size_t(n_host));       // host rows
    put(tile);                                   // Delta_1
    put(16*rows*W);                              // weights
    put(tile*S);                                 // the steps' tiles
    put(tile*(size_t(S) + 1));                   // the result table
    put(tile*K);                                 // out
    return o;
}

int ffk_periodic_shifts_dev(const void* const* control_matrices, int P, int A, int W, int d, const double* omega,
                            const double* basis, const double* eigvecs, const double* phase_differences,
                            const double* periods, const int32_t* steps, int S, const int32_t* count_slots, int K,
                            const double* spectrum, int s_ndim, const int32_t* idx, int n_idx, const double* delta1,
                            double* out, void* workspace, size_t workspace_bytes, void* stream) {
    FFK_REQUIRE(control_matrices && omega && basis && eigvecs && phase_differences && periods && count_slots &&
                    spectrum && idx && delta1 && out && (steps || S == 0),
                "NULL argument");
    FFK_REQUIRE(periodic_shifts_shape_ok(P, K, S, 0, A, W, d, n_idx, s_ndim), FFK_SHIFTS_SHAPE_MESSAGE, P, K, S, A, W,
                d, n_idx, s_ndim);
    const ShiftsScratch at = periodic_shifts_scratch(P, S, W, d, n_idx, s_ndim);
    FFK_REQUIRE(workspace && workspace_bytes >= at.total, "workspace of %zu bytes, need %zu", workspace_bytes,
                at.total);
    unsigned char* base = static_cast<unsigned char*>(workspace);
    return periodic_shifts_enqueue(reinterpret_cast<const cplx* const*>(control_matrices), P, W, d, omega,
                                   reinterpret_cast<const cplx*>(basis), reinterpret_cast<const cplx*>(eigvecs),
                                   phase_differences, periods, steps, S, count_slots, K,
                                   reinterpret_cast<const cplx*>(spectrum), s_ndim, idx, n_idx, delta1,
                                   reinterpret_cast<cplx*>(base + at.scale), reinterpret_cast<double*>(base + at.tiles),
                                   reinterpret_cast<double*>(base + at.table), out, static_cast<hipStream_t>(stream));
}

int ffk_resident_periodic_shifts(ffk_resident* const* pulses, const int32_t* slots, const double* control_matrices,
                                 int P, int A, int W, int d, const double* omega, const double* basis,
                                 const double* eigvecs, const double* phase_differences, const double* periods,
                                 const int32_t* steps, int S, const int32_t* count_slots, int K,
                                 const double* spectrum, int s_ndim, const int32_t* idx, int n_idx,
                                 const double* delta1, double* out) {
    FFK_REQUIRE(pulses && slots && omega && basis && eigvecs && phase_differences && periods && count_slots &&
                    spectrum && idx && delta1 && out && (steps || S == 0),
                "NULL argument");
    FFK_REQUIRE(periodic_shifts_shape_ok(P, K, S, 0, A, W, d, n_idx, s_ndim), FFK_SHIFTS_SHAPE_MESSAGE, P, K, S, A, W,
                d, n_idx, s_ndim);
    if (int rc = check_periodic_shifts_host_args(steps, S, count_slots, K, idx, n_idx, A)) return rc;
    if (int rc = kernel_fault_stale()) return rc;
    int dev = 0;
    FFK_HIP(hipGetDevice(&dev));
    const int N = d*d;
    const size_t dd = size_t(N), row = 2*dd*size_t(A)*W;      // doubles of one control matrix
    const size_t tile = size_t(P)*n_idx*dd*dd;                // doubles of one N x N tile per pulse and operator
    std::vector<const unsigned char*> tab;
    int n_host = 0;
    if (int rc = resident_locate_control_matrices(pulses, slots, P, dev, A, N, W, "pulse", &tab, &n_host)) return rc;
    FFK_REQUIRE(n_host == 0 || control_matrices, "control_matrices is NULL but %d pulse(s) have no handle", n_host);
    const size_t rows = s_ndim == 1 ? 1 : size_t(n_idx);
    StagedCall call;
    const auto s_tab = call.out<const unsigned char*>(P);
    const auto s_omega = call.in<double>(omega, W);
    const auto s_basis = call.in<double>(basis, 2*dd*dd);
    const auto s_V = call.in<double>(eigvecs, 2*size_t(P)*dd);
    const auto s_phi = call.in<double>(phase_differences, 2*size_t(P)*dd);
    const auto s_T = call.in<double>(periods, P);
    const auto s_steps = call.in<int32_t>(steps, 4*size_t(S));
    const auto s_slots = call.in<int32_t>(count_slots, K);
    const auto s_idx = call.in<int32_t>(idx, n_idx);
    const auto s_S = call.in<double>(spectrum, 2*rows*W);
    const auto s_host = call.in<double>(control_matrices, row*size_t(n_host));
    const auto s_delta1 = call.in<double>(delta1, tile);
    const auto s_scale = call.out<double>(2*rows*W);
    const auto s_tiles = call.out<double>(tile*S);
    const auto s_table = call.out<double>(tile*(size_t(S) + 1));
    const auto s_out = call.out<double>(tile*K);
    if (int rc = call.stage()) return rc;
    FFK_REQUIRE(call[s_tab] && call[s_table] && call[s_out], "internal: arena too small");
    const unsigned char* host_rows = reinterpret_cast<const unsigned char*>(call[s_host]);
    size_t placed = 0;
    for (const unsigned char*& at : tab)
        if (!at) at = host_rows + 8*row*placed++;
    FFK_HIP(hipMemcpyAsync(call[s_tab], tab.data(), 8*size_t(P), hipMemcpyHostToDevice, nullptr));
    if (int rc = periodic_shifts_enqueue(reinterpret_cast<const cplx* const*>(call[s_tab]), P, W, d, call[s_omega],
                                         reinterpret_cast<const cplx*>(call[s_basis]),
                                         reinterpret_cast<const cplx*>(call[s_V]), call[s_phi], call[s_T],
                                         call[s_steps], S, call[s_slots], K, reinterpret_cast<const cplx*>(call[s_S]),
                                         s_ndim, call[s_idx], n_idx, call[s_delta1],
                                         reinterpret_cast<cplx*>(call[s_scale]), call[s_tiles], call[s_table],
                                         call[s_out], nullptr))
        return rc;
    if (int rc = call.copy_back(out, s_out)) return rc;
    return call.finish_with_fault_status();
}

size_t ffk_periodic_workspace_bytes(int P, int K, int n_host, int A, int W, int d, int n_idx, int s_ndim, int stage) {
    if (!periodic_shape_ok(P, K, n_host, A, W, d, n_idx, s_ndim, stage)) return 0;
    const size_t dd = size_t(d)*d;
    const size_t rows = stage == 1 ? 0 : (s_ndim == 1 ? 1 : size_t(n_idx));
    size_t o = 0;
    auto put = [&o](size_t bytes) { o += align_up(bytes); };
    put(8*size_t(P));                            // pointer table
    put(8*size_t(W));                            // omega
    put(16*dd*dd);                               // basis
    put(16*size_t(P)*dd);                        // eigenvectors
    put(16*size_t(P)*dd);                        // phase differences
    put(8*size_t(P));                            // periods
    put(4*size_t(K));                            // repeats
    put(4*size_t(n_idx));                        // idx
    put(16*rows*W);                              // spectrum
    put(16*dd*size_t(A)*W*size_t(n_host));       // host rows
    put(16*rows*W);                              // weights
    put(8*periodic_out_count(P, K, W, d, n_idx, stage));
    return o;
}

int ffk_periodic_dev(const void* const* control_matrices, int P, int A, int W, int d, const double* omega,
                     const double* basis, const double* eigvecs, const double* phase_differences, const double* periods,
                     const int32_t* repeats, int K, const double* spectrum, int s_ndim, const int32_t* idx,
                     int n_idx, int d_infidelity, int stage, double* out, void* workspace, size_t workspace_bytes,
                     void* stream) {
    FFK_REQUIRE(control_matrices && omega && basis && eigvecs && phase_differences && periods && repeats && idx && out,
                "NULL argument");
    FFK_REQUIRE(periodic_shape_ok(P, K, 0, A, W, d, n_idx, s_ndim, stage),
                "unsupported shape P=%d K=%d A=%d W=%d d=%d n_idx=%d s_ndim=%d stage=%d (need 1 <= P, K <= 65535, "
                "2 <= d <= 4, 1 <= n_idx <= A, stage 1..3, and for stage 2, 3 s_ndim 1 or 2 and W >= 2)",
                P, K, A, W, d, n_idx, s_ndim, stage);
    const size_t rows = s_ndim == 1 ? 1 : size_t(n_idx);
    FFK_REQUIRE(stage == 1 || (spectrum && d_infidelity >= 1), "stage %d needs a spectrum and d_infidelity >= 1", stage);
    FFK_REQUIRE(stage == 1 || (workspace && workspace_bytes >= align_up(16*rows*W)),
                "workspace of %zu bytes, need %zu", workspace_bytes, align_up(16*rows*W));
    return periodic_enqueue(reinterpret_cast<const cplx* const*>(control_matrices), P, W, d, omega,
                            reinterpret_cast<const cplx*>(basis), reinterpret_cast<const cplx*>(eigvecs), phase_differences,
                            periods, repeats, K, reinterpret_cast<const cplx*>(spectrum), s_ndim, idx, n_idx,
                            d_infidelity, stage, static_cast<cplx*>(workspace), out, static_cast<hipStream_t>(stream));
}

int ffk_resident_periodic(ffk_resident* const* pulses, const int32_t* slots, const double* control_matrices, int P,
                          int A, int W, int d, const double* omega, const double* basis, const double* eigvecs,
                          const double* phase_differences, const double* periods, const int32_t* repeats, int K,
                          const double* spectrum, int s_ndim, const int32_t* idx, int n_idx, int d_infidelity,
                          int stage, double* out) {
    FFK_REQUIRE(pulses && slots && omega && basis && eigvecs && phase_differences && periods && repeats && idx && out,
                "NULL argument");
    FFK_REQUIRE(periodic_shape_ok(P, K, 0, A, W, d, n_idx, s_ndim, stage),
                "unsupported shape P=%d K=%d A=%d W=%d d=%d n_idx=%d s_ndim=%d stage=%d (need 1 <= P, K <= 65535, "
                "2 <= d <= 4, 1 <= n_idx <= A, stage 1..3, and for stage 2, 3 s_ndim 1 or 2 and W >= 2)",
                P, K, A, W, d, n_idx, s_ndim, stage);
    FFK_REQUIRE(stage == 1 || (spectrum && d_infidelity >= 1), "stage %d needs a spectrum and d_infidelity >= 1", stage);
    if (int rc = check_periodic_host_args(repeats, K, idx, n_idx, A)) return rc;
    if (int rc = kernel_fault_stale()) return rc;
    int dev = 0;
    FFK_HIP(hipGetDevice(&dev));
    const int N = d*d;
    const size_t dd = size_t(N), row = 2*dd*size_t(A)*W;      // doubles of one control matrix
    std::vector<const unsigned char*> tab;
    int n_host = 0;
    if (int rc = resident_locate_control_matrices(pulses, slots, P, dev, A, N, W, "pulse", &tab, &n_host)) return rc;
    FFK_REQUIRE(n_host == 0 || control_matrices, "control_matrices is NULL but %d pulse(s) have no handle", n_host);
    const size_t rows = stage == 1 ? 0 : (s_ndim == 1 ? 1 : size_t(n_idx));
    StagedCall call;
    const auto s_tab = call.out<const unsigned char*>(P);
    const auto s_omega = call.in<double>(omega, W);
    const auto s_basis = call.in<double>(basis, 2*dd*dd);
    const auto s_V = call.in<double>(eigvecs, 2*size_t(P)*dd);
    const auto s_phi = call.in<double>(phase_differences, 2*size_t(P)*dd);
    const auto s_T = call.in<double>(periods, P);
    const auto s_rep = call.in<int32_t>(repeats, K);
    const auto s_idx = call.in<int32_t>(idx, n_idx);
    const auto s_S = call.in<double>(spectrum, 2*rows*W);
    const auto s_host = call.in<double>(control_matrices, row*size_t(n_host));
    const auto s_scale = call.out<double>(2*rows*W);
    const auto s_out = call.out<double>(periodic_out_count(P, K, W, d, n_idx, stage));
    if (int rc = call.stage()) return rc;
    FFK_REQUIRE(call[s_tab] && call[s_out], "internal: arena too small");
    const unsigned char* host_rows = reinterpret_cast<const unsigned char*>(call[s_host]);
    size_t placed = 0;
    for (const unsigned char*& at : tab)
        if (!at) at = host_rows + 8*row*placed++;
    FFK_HIP(hipMemcpyAsync(call[s_tab], tab.data(), 8*size_t(P), hipMemcpyHostToDevice, nullptr));
    if (int rc = periodic_enqueue(reinterpret_cast<const cplx* const*>(call[s_tab]), P, W, d, call[s_omega],
                                  reinterpret_cast<const cplx*>(call[s_basis]),
                                  reinterpret_cast<const cplx*>(call[s_V]), call[s_phi], call[s_T], call[s_rep], K,
                                  reinterpret_cast<const cplx*>(call[s_S]), s_ndim, call[s_idx], n_idx, d_infidelity,
                                  stage, reinterpret_cast<cplx*>(call[s_scale]), call[s_out], nullptr))
        return rc;
    if (int rc = call.copy_back(out, s_out)) return rc;
    return call.finish_with_fault_status();
}

}  // extern "C"

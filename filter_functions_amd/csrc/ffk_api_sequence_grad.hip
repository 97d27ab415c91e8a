// ffk_api_sequence_grad.hip -- the gradient of the filter function / infidelity of P gate sequences, given as index
// arrays into one gate set, in ONE pass (ffk_sequence_infidelity_derivatives; kernels: sequence_gradient.hip and the
// prologue, totals and reduce kernels of grad_batch.hip).  As in ffk_api_batch_grad.hip the inputs are packed into one
// pinned staging block and cross in one H2D copy; the launches follow on the same stream without a synchronisation;
// one D2H copy per requested output.  The number of launches and copies does not depend on P.
#include "ffk_api_common.h"

namespace {

// the one layout of the pass: [inputs, in the order they are staged][scratch][outputs].  With base NULL it only
// measures.  The input block is the same in the pinned staging block and at the front of the device block.
struct SeqGradWs {
    double *D, *V, *Q, *B, *nc, *C, *dt, *t, *om, *S, *U, *tau, *occ_weight, *gate_start;   // inputs
    int32_t *gate_segments, *offsets, *index, *occ_offsets, *occ_length;
    int64_t *seg_start, *occ_row;
    size_t input_bytes;
    cplx *scale, *rec, *totals;
    double *partial, *dI, *dF, *gate_dI;
};

struct SeqGradShape {
    int T, Gmax, P, W, A, H, d, srows;
    size_t n_index, n_segments;
    bool want_dI, want_dF, want_gate;
};

size_t slice_sequence_grad(void* base, size_t bytes, const SeqGradShape& s, SeqGradWs* w) {
    Bump ws(base, base ? bytes : ~size_t(0)/2);
    const size_t dd = size_t(s.d)*s.d, T = size_t(s.T), G = size_t(s.Gmax), A = size_t(s.A), H = size_t(s.H);
    const size_t tiles = size_t(s.W + 63)/64, rows = s.n_segments*A*H;
    *w = SeqGradWs{};
    w->D = ws.take<double>(T*G*s.d);
    w->V = ws.take<double>(2*T*G*dd);
    w->Q = ws.take<double>(2*T*(G + 1)*dd);
    w->B = ws.take<double>(2*T*A*dd);
    w->nc = ws.take<double>(T*A*G);
    w->C = ws.take<double>(2*T*H*dd);
    w->dt = ws.take<double>(T*G);
    w->t = ws.take<double>(T*(G + 1));
    w->om = ws.take<double>(size_t(s.W));
    if (s.srows > 0) w->S = ws.take<double>(2*size_t(s.srows)*s.W);
    w->U = ws.take<double>(2*T*dd);
    w->tau = ws.take<double>(T);
    w->gate_segments = ws.take<int32_t>(T);
    w->offsets = ws.take<int32_t>(size_t(s.P) + 1);
    w->index = ws.take<int32_t>(s.n_index);
    w->seg_start = ws.take<int64_t>(size_t(s.P) + 1);
    if (s.want_gate) {
        w->occ_offsets = ws.take<int32_t>(T + 1);
        w->occ_row = ws.take<int64_t>(s.n_index);
        w->occ_length = ws.take<int32_t>(s.n_index);
        w->occ_weight = ws.take<double>(s.n_index);
        w->gate_start = ws.take<double>(T*A*G*H);
    }
    w->input_bytes = ws.used;
    if (s.srows > 0) w->scale = ws.take<cplx>(size_t(s.srows)*s.W);
    w->rec = ws.take<cplx>(T*G*ffk::grad_batch_record_elems(s.d, s.A, s.H));
    w->totals = ws.take<cplx>(T*A*dd*s.W);
    if (s.want_gate) w->gate_dI = ws.take<double>(T*A*G*H);
    if (s.want_dI) {
        w->partial = ws.take<double>(tiles*rows);
        w->dI = ws.take<double>(rows);
    }
    if (s.want_dF) w->dF = ws.take<double>(rows*s.W);
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

size_t ffk_sequence_infidelity_derivatives_workspace_bytes(int T, int Gmax, int P, long long n_index,
                                                           long long n_segments, int W, int A, int H, int d,
                                                           int want_dF) {
    if (!ffk::sequence_gradient_supported(T, Gmax, P, W, A, H, d) || n_index < P || n_segments < n_index) return 0;
    // what does not depend on the walked segments (counted for a spectrum per operator and for the per-gate sums),
    // plus the segments' rows: an upper bound of the packed layout, linear in n_segments
    SeqGradWs w;
    const SeqGradShape fixed{T, Gmax, P, W, A, H, d, A, size_t(n_index), 0, true, true, true};
    const size_t tiles = size_t(W + 63)/64;
    const size_t per_segment = 8*size_t(A)*H*(want_dF ? size_t(W) : tiles + 1);
    return slice_sequence_grad(nullptr, 0, fixed, &w) + 3*256 + size_t(n_segments)*per_segment;
}

int ffk_sequence_infidelity_derivatives(int T, int Gmax, const int32_t* gate_segments, const double* eigvals,
                                        const double* eigvecs, const double* propagators, const double* n_opers,
                                        int A, const double* n_coeffs, const double* c_opers, int H, const double* dt,
                                        int d, const int32_t* offsets, const int32_t* index, int P,
                                        const double* omega, int W, const double* spectrum, int s_ndim,
                                        const int32_t* occ_offsets, const int32_t* occ_sequence,
                                        const int32_t* occ_position, const double* weights,
                                        double* filter_function_derivative, double* infidelity_derivative,
                                        double* gate_infidelity_derivative) {
    FFK_REQUIRE(d >= 2 && d <= 4, "the sequence gradient kernels support 2 <= d <= 4, not d=%d", d);
    FFK_REQUIRE(W >= 1 && A >= 1 && H >= 1 && T >= 1 && P >= 1 && Gmax >= 1, "empty axis: W=%d A=%d H=%d T=%d P=%d Gmax=%d",
                W, A, H, T, P, Gmax);
    FFK_REQUIRE(A <= 4 && H <= 8, "the sequence gradient takes A <= 4 noise and H <= 8 control operators, not A=%d H=%d",
                A, H);
    FFK_REQUIRE(T <= 65535 && P <= 65535 && Gmax <= 65535, "need at most 65535 gates, sequences and segments of a gate, "
                "got T=%d P=%d Gmax=%d", T, P, Gmax);
    FFK_REQUIRE(gate_segments && eigvals && eigvecs && propagators && n_opers && n_coeffs && c_opers && dt && offsets &&
                index && omega, "NULL argument");
    const bool want_dF = filter_function_derivative != nullptr, want_gate = gate_infidelity_derivative != nullptr;
    const bool want_dI = infidelity_derivative != nullptr || want_gate;
    FFK_REQUIRE(want_dF || want_dI, "no output requested");
    FFK_REQUIRE(!want_dI || (spectrum && (s_ndim == 1 || s_ndim == 2)),
                "infidelity derivative needs a spectrum of shape (W,) or (A, W), not s_ndim=%d", s_ndim);
    FFK_REQUIRE(!want_gate || (occ_offsets && occ_sequence && occ_position && weights),
                "the per-gate sums need the occurrence lists and the weights");
    FFK_REQUIRE(ffk::sequence_gradient_supported(T, Gmax, P, W, A, H, d), "shape too large for one pass: W=%d", W);
    for (int k = 0; k < T; ++k)
        FFK_REQUIRE(gate_segments[k] >= 1 && gate_segments[k] <= Gmax, "gate %d has %d segments, expected 1 to %d", k,
                    gate_segments[k], Gmax);
    FFK_REQUIRE(offsets[0] == 0, "offsets[0] = %d, expected 0", offsets[0]);
    for (int p = 0; p < P; ++p)
        FFK_REQUIRE(offsets[p + 1] > offsets[p], "sequence %d is empty (offsets %d -> %d)", p, offsets[p],
                    offsets[p + 1]);
    const size_t n_index = size_t(offsets[P]);
    for (size_t i = 0; i < n_index; ++i)
        FFK_REQUIRE(index[i] >= 0 && index[i] < T, "index[%zu] = %d outside [0, %d)", i, index[i], T);
    // segments before every position and every sequence
    std::vector<int64_t> seg_start(size_t(P) + 1, 0), before(n_index);
    for (int p = 0; p < P; ++p) {
        int64_t run = 0;
        for (int32_t i = offsets[p]; i < offsets[p + 1]; ++i) {
            before[size_t(i)] = run;
            run += gate_segments[index[i]];
        }
        seg_start[size_t(p) + 1] = seg_start[size_t(p)] + run;
    }
    const size_t n_segments = size_t(seg_start[size_t(P)]);
    FFK_REQUIRE((n_segments*A*H + 255)/256 <= 0x7fffffffull, "too many segments for one pass: %zu", n_segments);
    if (want_gate) {
        FFK_REQUIRE(occ_offsets[0] == 0 && size_t(occ_offsets[T]) == n_index,
                    "the occurrence lists must name every position once: occ_offsets[0]=%d occ_offsets[T]=%d", occ_offsets[0],
                    occ_offsets[T]);
        for (int k = 0; k < T; ++k) {
            FFK_REQUIRE(occ_offsets[k + 1] >= occ_offsets[k], "occ_offsets not ascending at gate %d", k);
            for (int32_t o = occ_offsets[k]; o < occ_offsets[k + 1]; ++o) {
                const int32_t p = occ_sequence[o], g = occ_position[o];
                FFK_REQUIRE(p >= 0 && p < P && g >= 0 && g < offsets[p + 1] - offsets[p] && index[offsets[p] + g] == k,
                            "occurrence %d of gate %d names sequence %d, position %d, where that gate does not stand", o,
                            k, p, g);
            }
        }
    }
    const int srows = want_dI ? (s_ndim == 2 ? A : 1) : 0;
    const SeqGradShape shape{T, Gmax, P, W, A, H, d, srows, n_index, n_segments, want_dI, want_dF, want_gate};
    std::lock_guard<std::mutex> lock(g_arena.mu);
    SeqGradWs m;
    const size_t total = slice_sequence_grad(nullptr, 0, shape, &m);
    void *base, *stage;
    if (int rc = arena_reserve(total, &base)) return rc;
    if (int rc = stage_reserve(m.input_bytes, &stage)) return rc;
    SeqGradWs h, w;
    SeqGradShape inputs = shape;
    inputs.want_dI = inputs.want_dF = false;
    slice_sequence_grad(stage, m.input_bytes, inputs, &h);
    slice_sequence_grad(base, g_arena.size, shape, &w);
    FFK_REQUIRE(h.seg_start && (!want_gate || h.occ_weight), "internal: staging block too small");
    FFK_REQUIRE(w.totals && (!want_gate || w.gate_dI) && (!want_dI || w.dI) && (!want_dF || w.dF),
                "internal: arena too small");
    const size_t dd = size_t(d)*d, t = size_t(T), G = size_t(Gmax);
    std::memcpy(h.D, eigvals, 8*t*G*d);
    std::memcpy(h.V, eigvecs, 16*t*G*dd);
    std::memcpy(h.Q, propagators, 16*t*(G + 1)*dd);
    std::memcpy(h.nc, n_coeffs, 8*t*A*G);
    std::memcpy(h.dt, dt, 8*t*G);
    for (size_t k = 0; k < t; ++k) {
        // every gate carries the same operators; its start times, duration and total propagator follow from dt and
        // from the propagator behind its last segment (the padding repeats it)
        std::memcpy(h.B + 2*k*A*dd, n_opers, 16*size_t(A)*dd);
        std::memcpy(h.C + 2*k*H*dd, c_opers, 16*size_t(H)*dd);
        double run = 0.0;
        for (size_t s = 0; s < G; ++s) {
            h.t[k*(G + 1) + s] = run;
            run += dt[k*G + s];
        }
        h.t[k*(G + 1) + G] = run;
        h.tau[k] = run;
        std::memcpy(h.U + 2*k*dd, propagators + 2*(k*(G + 1) + G)*dd, 16*dd);
    }
    std::memcpy(h.om, omega, 8*size_t(W));
    if (srows > 0) std::memcpy(h.S, spectrum, 16*size_t(srows)*W);
    std::memcpy(h.gate_segments, gate_segments, 4*t);
    std::memcpy(h.offsets, offsets, 4*(size_t(P) + 1));
    std::memcpy(h.index, index, 4*n_index);
    std::memcpy(h.seg_start, seg_start.data(), 8*(size_t(P) + 1));
    if (want_gate) {
        std::memcpy(h.occ_offsets, occ_offsets, 4*(t + 1));
        for (size_t o = 0; o < n_index; ++o) {
            const int32_t p = occ_sequence[o];
            h.occ_row[o] = seg_start[size_t(p)]*A + before[size_t(offsets[p] + occ_position[o])];
            h.occ_length[o] = int32_t(seg_start[size_t(p) + 1] - seg_start[size_t(p)]);
            h.occ_weight[o] = weights[p];
        }
        std::memcpy(h.gate_start, gate_infidelity_derivative, 8*t*A*G*H);
    }
    hipStream_t st = nullptr;
    StreamDrain drain{st};
    FFK_HIP(hipMemcpyAsync(base, stage, m.input_bytes, hipMemcpyHostToDevice, st));
    if (want_dI)
        FFK_HIP(ffk::launch_spectral_weights(reinterpret_cast<const cplx*>(w.S), srows, W, w.om, W, 0, w.scale, st));
    FFK_HIP(ffk::launch_grad_batch_records(T, w.D, reinterpret_cast<const cplx*>(w.V),
                                           reinterpret_cast<const cplx*>(w.Q), reinterpret_cast<const cplx*>(w.B), A,
                                           w.nc, reinterpret_cast<const cplx*>(w.C), H, w.dt, w.t, Gmax, d, w.rec, st));
    FFK_HIP(ffk::launch_grad_batch_pulse_totals(T, w.om, W, w.rec, Gmax, d, A, H, w.totals, st));
    FFK_HIP(ffk::launch_sequence_gradient_walk(w.om, W, w.rec, w.totals, reinterpret_cast<const cplx*>(w.U), w.tau,
                                               w.gate_segments, Gmax, w.offsets, w.index, w.seg_start, P, d, A, H,
                                               want_dI ? w.scale : nullptr, s_ndim, w.dF, w.partial, st));
    const size_t rows = n_segments*A*H;
    if (want_dI) FFK_HIP(ffk::launch_grad_batch_reduce(w.partial, (W + 63)/64, rows, d, w.dI, st));
    if (want_gate) {
        FFK_HIP(ffk::launch_sequence_gradient_gather(w.dI, w.occ_offsets, w.occ_row, w.occ_length, w.occ_weight,
                                                     w.gate_segments, T, Gmax, A, H, w.gate_start, w.gate_dI, st));
        FFK_HIP(hipMemcpyAsync(gate_infidelity_derivative, w.gate_dI, 8*t*A*G*H, hipMemcpyDeviceToHost, st));
    }
    if (infidelity_derivative) FFK_HIP(hipMemcpyAsync(infidelity_derivative, w.dI, 8*rows, hipMemcpyDeviceToHost, st));
    if (want_dF)
        FFK_HIP(hipMemcpyAsync(filter_function_derivative, w.dF, 8*rows*W, hipMemcpyDeviceToHost, st));
    FFK_HIP(hipStreamSynchronize(st));
    return FFK_OK;
}

}  // extern "C"

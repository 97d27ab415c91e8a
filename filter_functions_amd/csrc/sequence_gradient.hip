// sequence_gradient.hip -- the gradient of the filter function / infidelity of gate sequences given as index arrays
// into one gate set (ffk_sequence_infidelity_derivatives; ff.sequence_infidelity_derivatives,
// ff.sequence_filter_function_derivatives, ff.gate_infidelity_derivatives), 2 <= d <= 4.
//
// Same mathematics as grad_batch.hip (read its header and grad.hip's first): the derivative at segment s needs the
// segment's own record, the total Y_a(w) of the interaction-picture noise operator and its running sum Ycum up to s.
// A sequence of gates repeats the segments of its gates, moved in time and rotated by what stands before them.  With
// P_g the propagator before position g and b_g its start time, work in the frame of the current position,
//
//     X^ = e^{-i w b_g} P_g X P_g^dag                                  (X = Ytot, Ycum)
//
// in which a segment's step, its T, E and t are the gate's own: ONE record per gate segment (gradwalk::record_elems,
// written by grad_batch.hip's prologue over the gate set) serves every position of every sequence.  Both terms of
//
//     2 Re tr(Y^_a^dag Y')  -  2 Re tr(E_hs [Y^_a^dag, Y^cum])
//
// do not change under the change of frame (the phases of Y^^dag and Y^cum cancel, the rotations cancel under the
// trace), and the frame advances per position by  X^ <- e^{-i w tau_k} U_k X^ U_k^dag  with the gate's total
// propagator and duration.  Nothing of the size of a sequence is ever formed:
//
//   gradb_prologue_kernel, gradb_totals_kernel (grad_batch.hip)   records and totals Y_{k,a}(w) (T, A, d, d, W) of
//                                              the GATES, one chunk per gate; short gates are padded on the host with
//                                              segments of zero duration, whose steps are exact zeros
//   sequence_gradient_walk_kernel<D> (A, P, W/64)   lane = frequency.  Pass 1, backward over the positions:
//                                                  Z <- Y_{k_g} + e^{i w tau_k} U_k^dag Z U_k
//                                              leaves Ytot in the frame of the first position.  Pass 2, forward:
//                                              gradwalk::segment_terms -- the body of grad_batch_kernel -- over the
//                                              gate's G_k records, then Y^tot^dag and Y^cum move to the next frame.
//                                              Stores dF, or one partial per (tile, a, segment, h) after the lane sum
//   gradb_reduce_kernel (grad_batch.hip)       partials added in tile order, times 1/d
//   sequence_gradient_gather_kernel (A Gmax H/64, T)   per gate: sum_p w_p sum_{g: s_p[g] = k} of the position's rows,
//                                              one thread per entry over the host-built occurrence list, in list order,
//                                              added to the caller's starting values (the passes before this one)
//
// One wavefront walks a whole sequence for its (operator, tile); the gate numbers are read in chunks of 64 positions.
// The tile width and the order of every sum depend on the shape alone, no atomics, no block waits for another: a
// sequence's result is the same bits alone or among others, at any place in the pass.
#include "ffk_internal.h"
#include "grad_walk.h"
#include "sequence_walk.h"

namespace ffk {
namespace {

// X <- ph U X U^dag (DAGGER false) or ph U^dag X U (DAGGER true); U is the same for every lane
template <int D, bool DAGGER>
__device__ __forceinline__ void change_frame(cplx (&X)[D*D], const cplx* __restrict__ U, cplx ph) {
    cplx tmp[D*D];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            cplx acc = {0.0, 0.0};
#pragma unroll
            for (int k = 0; k < D; ++k) {
                if (DAGGER) cmac_conj(acc, U[k*D + i], X[k*D + j]);
                else cmac(acc, U[i*D + k], X[k*D + j]);
            }
            tmp[i*D + j] = acc;
        }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            cplx acc = {0.0, 0.0};
#pragma unroll
            for (int k = 0; k < D; ++k) {
                if (DAGGER) {
                    cmac(acc, tmp[i*D + k], U[k*D + j]);
                } else {
                    const cplx u = U[j*D + k];
                    cmac(acc, tmp[i*D + k], cplx{u.re, -u.im});
                }
            }
            X[i*D + j] = cmul(ph, acc);
        }
}

template <int D>
__global__ __launch_bounds__(64) void sequence_gradient_walk_kernel(
    const double* __restrict__ omega, int W, const cplx* __restrict__ rec, const cplx* __restrict__ totals,
    const cplx* __restrict__ U, const double* __restrict__ tau, const int32_t* __restrict__ gate_segments, int Gmax,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, const int64_t* __restrict__ seg_start,
    int P, int A, int H, const cplx* __restrict__ scale, int s_ndim, double* __restrict__ dF,
    double* __restrict__ partial) {
    constexpr int D2 = D*D;
    extern __shared__ unsigned char smem[];
    const int lane = threadIdx.x;
    const gradwalk::SegmentLds<D> lds(smem, H, lane);
    const int a = blockIdx.x, p = blockIdx.y, tile = blockIdx.z;
    const int w = tile*64 + lane;
    const bool valid = w < W;
    const int wc = valid ? w : W - 1;
    const double om = omega[wc];
    double weight = 0.0;
    if (scale != nullptr && valid) weight = scale[(s_ndim == 2 ? static_cast<size_t>(a)*W : 0) + w].re;
    const int32_t* list = index + offsets[p];
    const int n = offsets[p + 1] - offsets[p];
    cplx Yd[D2], Yq[D2];                                   // Y^tot^dag, Y^cum
    // pass 1, backward: Z (in Yq) = Ytot in the frame of the first position
#pragma unroll
    for (int e = 0; e < D2; ++e) Yq[e] = {0.0, 0.0};
#pragma unroll 1
    for (int c1 = n; c1 > 0;) {
        const int c0 = (c1 - 1)/64*64;
        const int chunk = seqwalk::chunk_gates(list, true, c0, c1, lane);
#pragma unroll 1
        for (int at = c1 - c0 - 1; at >= 0; --at) {
            const int k = seqwalk::gate_at(chunk, at);
            change_frame<D, true>(Yq, U + static_cast<size_t>(k)*D2, cexp(om*tau[k]));
            const cplx* tot = totals + (static_cast<size_t>(k)*A + a)*D2*W + wc;
#pragma unroll
            for (int e = 0; e < D2; ++e) {
                const cplx v = tot[static_cast<size_t>(e)*W];
                Yq[e].re += v.re;
                Yq[e].im += v.im;
            }
        }
        c1 = c0;
    }
#pragma unroll
    for (int x = 0; x < D; ++x)
#pragma unroll
        for (int y = 0; y < D; ++y) Yd[x*D + y] = {Yq[y*D + x].re, -Yq[y*D + x].im};
#pragma unroll
    for (int e = 0; e < D2; ++e) Yq[e] = {0.0, 0.0};
    // pass 2, forward: this block's rows are (a, segment) of sequence p, H entries each
    const size_t rs = gradwalk::record_elems(D, A, H);
    const size_t segments = static_cast<size_t>(seg_start[p + 1] - seg_start[p]);
    size_t row = (static_cast<size_t>(seg_start[p])*A + static_cast<size_t>(a)*segments)*H;
    const size_t rows = static_cast<size_t>(seg_start[P])*A*H;
    const int b_off = 1 + (2 + a)*D2, ae_off = 1 + (2 + A)*D2;
    if (dF) dF += w;
    if (partial) partial += static_cast<size_t>(tile)*rows;
#pragma unroll 1
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int c1 = c0 + 64 < n ? c0 + 64 : n;
        const int chunk = seqwalk::chunk_gates(list, true, c0, c1, lane);
#pragma unroll 1
        for (int at = 0; at < c1 - c0; ++at) {
            const int k = seqwalk::gate_at(chunk, at);
            const int Gk = gate_segments[k];
            const cplx* r = rec + static_cast<size_t>(k)*Gmax*rs;
#pragma unroll 1
            for (int s = 0; s < Gk; ++s, row += H) {
                lds.load(r + s*rs, b_off, ae_off, H, lane);
                gradwalk::segment_terms<D>(lds, om, H, lane, Yd, Yq, [&](int h, double val, double) {
                    if (dF != nullptr && valid) dF[(row + h)*W] = val;
                    if (partial != nullptr) {
                        double sum = val*weight;           // (lanes past W: weight 0)
                        if (!valid) sum = 0.0;
                        sum = gradwalk::lane_sum(sum);
                        if (lane == 0) partial[row + h] = sum;
                    }
                });
            }
            if (c0 + at + 1 < n) {                         // to the frame of the next position
                const cplx ph = cexp(om*tau[k]);
                const cplx* Uk = U + static_cast<size_t>(k)*D2;
                change_frame<D, false>(Yd, Uk, ph);
                change_frame<D, false>(Yq, Uk, cplx{ph.re, -ph.im});
            }
        }
    }
}

__global__ __launch_bounds__(64) void sequence_gradient_gather_kernel(
    const double* __restrict__ dI, const int32_t* __restrict__ occ_offsets, const int64_t* __restrict__ occ_row,
    const int32_t* __restrict__ occ_length, const double* __restrict__ occ_weight,
    const int32_t* __restrict__ gate_segments, int Gmax, int A, int H, const double* __restrict__ start,
    double* __restrict__ out) {
    const int k = blockIdx.y;
    const int e = blockIdx.x*64 + threadIdx.x;             // (a, s, h)
    if (e >= A*Gmax*H) return;
    const int h = e % H, s = e / H % Gmax, a = e / H / Gmax;
    double acc = start[static_cast<size_t>(k)*A*Gmax*H + e];
    if (s < gate_segments[k])
        for (int o = occ_offsets[k]; o < occ_offsets[k + 1]; ++o) {
            const size_t row = static_cast<size_t>(occ_row[o]) + static_cast<size_t>(a)*occ_length[o] + s;
            acc += occ_weight[o]*dI[row*H + h];
        }
    out[static_cast<size_t>(k)*A*Gmax*H + e] = acc;
}

}  // namespace

bool sequence_gradient_supported(int T, int Gmax, int P, int W, int A, int H, int d) {
    return T >= 1 && T <= 65535 && Gmax >= 1 && Gmax <= 65535 && P >= 1 && P <= 65535 && W >= 1 &&
           (W + 63)/64 <= 65535 && A >= 1 && A <= 4 && H >= 1 && H <= 8 && d >= 2 && d <= 4;
}

hipError_t launch_sequence_gradient_walk(const double* omega, int W, const cplx* rec, const cplx* totals,
                                         const cplx* U, const double* tau, const int32_t* gate_segments, int Gmax,
                                         const int32_t* offsets, const int32_t* index, const int64_t* seg_start,
                                         int P, int d, int A, int H, const cplx* scale, int s_ndim, double* dF,
                                         double* partial, hipStream_t stream) {
    if (P < 1 || P > 65535 || (W + 63)/64 > 65535 || A < 1 || A > 4 || H < 1 || H > 8 ||
        (partial != nullptr && scale == nullptr) || (dF == nullptr && partial == nullptr))
        return hipErrorInvalidValue;
    const dim3 grid(A, P, (W + 63)/64);
    const size_t lds = gradwalk::segment_lds_bytes(d, H);
    switch (d) {
#define FFK_SEQGRAD_CASE(D)                                                                                        \
    case D:                                                                                                        \
        hipLaunchKernelGGL((sequence_gradient_walk_kernel<D>), grid, dim3(64), lds, stream, omega, W, rec, totals, \
                           U, tau, gate_segments, Gmax, offsets, index, seg_start, P, A, H, scale, s_ndim, dF,     \
                           partial);                                                                               \
        break;
        FFK_SEQGRAD_CASE(2) FFK_SEQGRAD_CASE(3) FFK_SEQGRAD_CASE(4)
#undef FFK_SEQGRAD_CASE
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_sequence_gradient_gather(const double* dI, const int32_t* occ_offsets, const int64_t* occ_row,
                                           const int32_t* occ_length, const double* occ_weight,
                                           const int32_t* gate_segments, int T, int Gmax, int A, int H,
                                           const double* start, double* out, hipStream_t stream) {
    if (T < 1 || T > 65535 || Gmax < 1 || A < 1 || H < 1) return hipErrorInvalidValue;
    const unsigned blocks = static_cast<unsigned>((static_cast<size_t>(A)*Gmax*H + 63)/64);
    hipLaunchKernelGGL(sequence_gradient_gather_kernel, dim3(blocks, T), dim3(64), 0, stream, dI, occ_offsets,
                       occ_row, occ_length, occ_weight, gate_segments, Gmax, A, H, start, out);
    return hipGetLastError();
}

}  // namespace ffk

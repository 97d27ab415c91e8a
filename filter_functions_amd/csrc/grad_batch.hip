// grad_batch.hip -- the gradient of the filter function / infidelity for P pulses of one shape in one pass
// (ffk_batch_filter_function_derivative; ff.infidelity_derivatives, ff.filter_function_derivatives), 2 <= d <= 4.
//
// Same mathematics as grad.hip (read its header first): per segment s the d^2 first-order integrals I1(w + W_mn),
// the generator E_hs, the running sum Ycum_sa of the interaction-picture noise operator's steps and its total Ytot_a.
// grad.hip reads Ycum (G, A, d, d, W) from HBM -- 805 MB per pulse at d = 4, G = 256, A = 3, W = 4096, written by the
// accumulate kernel, rewritten by a prefix sum, read three times.  Here Ycum never exists:
//
//   gradb_prologue_kernel  (G, P)              T_s = V^dag Q_s, Bbar_a, Abar_h, E_hs: one record per segment
//   gradb_totals_kernel<D> (C A, P, W/64)      the sum of the steps of each chunk of L segments: (P, C, A, d, d, W)
//   gradb_prefix_kernel    (A d^2 W/256, P)    exclusive prefix over a pulse's C chunk totals in place, and Ytot
//   grad_batch_kernel<D>   (C A, P, W/64)      walks its L segments: forms the segment's step
//                                                  e^{i w t_s} T^dag (Bbar_a o I1) T
//                                              from the SAME I1 it needs for the first term anyway, adds it to the
//                                              running Ycum (registers) and evaluates grad_kernel's three terms.
//                                              Either stores dF, or multiplies by the spectral weight, adds up the 64
//                                              lanes and stores ONE partial per (tile, pulse, a, s, h)
//   gradb_reduce_kernel    (P A G H/256)       partials added in tile order, times 1/d
//
// Both walking kernels form a step with the same device function, so the totals are sums of exactly the steps the
// gradient kernel adds up again.  The chunk length L is a function of G alone (grad_batch_chunk): a pulse's result
// does not depend on the batch it is part of.  No atomics; no block waits for another.
#include <algorithm>

#include "ffk_internal.h"
#include "grad_walk.h"

namespace ffk {

int grad_batch_chunk(int G, int d, int W) {
    (void)d;
    (void)W;
    // at most 16 chunks per pulse (their totals are 16/G of the Ycum tensor), at least 8 segments per chunk (a
    // chunk's start costs 2 A d^2 reads per lane); short pulses: one chunk per 8 segments
    const int L = std::max(8, (G + 15)/16);
    return std::max(1, std::min(L, G));
}

namespace {

using gradwalk::integrals_and_half_step;
using gradwalk::record_elems;
using gradwalk::record_header;
using gradwalk::step_entry;

__global__ __launch_bounds__(64) void gradb_prologue_kernel(
    const double* __restrict__ eigvals, const cplx* __restrict__ eigvecs, const cplx* __restrict__ propagators,
    const cplx* __restrict__ n_opers, const double* __restrict__ n_coeffs, const cplx* __restrict__ c_opers,
    const double* __restrict__ dt, const double* __restrict__ t, int G, int d, int A, int H, cplx* __restrict__ rec) {
    __shared__ cplx V[16], Q[16], T[16], M[16], X[16];
    const int s = blockIdx.x, p = blockIdx.y, e = threadIdx.x;
    const int d2 = d*d;
    const size_t seg = static_cast<size_t>(p)*G + s;
    const bool on = e < d2;
    const int m = on ? e / d : 0, n = on ? e % d : 0;
    double* hdr = reinterpret_cast<double*>(rec + seg*record_elems(d, A, H));
    cplx* out = rec + seg*record_elems(d, A, H) + record_header(d);
    const double dts = dt[seg];
    double dE = 0.0;
    if (on) {
        dE = eigvals[seg*d + m] - eigvals[seg*d + n];
        hdr[2 + e] = dE;
        hdr[2 + d2 + e] = derivative_integral_rcp(dE, dts);
        V[e] = eigvecs[seg*d2 + e];
        Q[e] = propagators[(static_cast<size_t>(p)*(G + 1) + s)*d2 + e];
    }
    if (e == 0) {
        hdr[0] = dts;
        hdr[1] = t[static_cast<size_t>(p)*(G + 1) + s];
    }
    __syncthreads();
    if (on) {
        cplx acc = {0.0, 0.0};
        for (int k = 0; k < d; ++k) cmac_conj(acc, V[k*d + m], Q[k*d + n]);
        T[e] = acc;
        out[e] = acc;
    }
    __syncthreads();
    for (int a = 0; a < A; ++a) {
        const cplx* B = n_opers + (static_cast<size_t>(p)*A + a)*d2;
        if (on) {
            cplx acc = {0.0, 0.0};
            for (int k = 0; k < d; ++k) cmac(acc, B[m*d + k], V[k*d + n]);
            M[e] = acc;
        }
        __syncthreads();
        if (on) {
            const double c = n_coeffs[(static_cast<size_t>(p)*A + a)*G + s];
            cplx acc = {0.0, 0.0};
            for (int k = 0; k < d; ++k) cmac_conj(acc, V[k*d + m], M[k*d + n]);
            out[static_cast<size_t>(1 + a)*d2 + e] = {acc.re*c, acc.im*c};
        }
        __syncthreads();
    }
    for (int h = 0; h < H; ++h) {
        const cplx* C = c_opers + (static_cast<size_t>(p)*H + h)*d2;
        if (on) {
            cplx acc = {0.0, 0.0};
            for (int k = 0; k < d; ++k) cmac(acc, C[m*d + k], V[k*d + n]);
            M[e] = acc;
        }
        __syncthreads();
        if (on) {
            cplx acc = {0.0, 0.0};
            for (int k = 0; k < d; ++k) cmac_conj(acc, V[k*d + m], M[k*d + n]);
            out[static_cast<size_t>(1 + A + h)*d2 + e] = acc;                  // Abar_h
            X[e] = cmul(acc, first_order_integral(0.0, dE, dts));              // Abar_h o I1(0)
        }
        __syncthreads();
        if (on) {
            // E_hs = -i T^dag X T, entry [x][y] = [m][n]  (grad_generator_kernel)
            cplx acc = {0.0, 0.0};
            for (int k = 0; k < d; ++k) {
                cplx row = {0.0, 0.0};
                for (int j = 0; j < d; ++j) cmac(row, X[k*d + j], T[j*d + n]);
                cmac_conj(acc, T[k*d + m], row);
            }
            out[static_cast<size_t>(1 + A + H + h)*d2 + e] = {acc.im, -acc.re};
        }
        __syncthreads();
    }
}

template <int D>
__global__ __launch_bounds__(64) void gradb_totals_kernel(const double* __restrict__ omega, int W,
                                                          const cplx* __restrict__ rec, int G, int A, int H, int L,
                                                          int C, cplx* __restrict__ totals) {
    constexpr int D2 = D*D;
    __shared__ cplx head[1 + 2*D2];                        // the record's header and T
    __shared__ cplx Bs[D2];
    const double* hdr = reinterpret_cast<const double*>(head);
    const double* dE = hdr + 2;
    const cplx* Ts = head + 1 + D2;
    __shared__ cplx I1s[D2*64], Zs[D2*64];
    const int c = blockIdx.x / A, a = blockIdx.x % A, p = blockIdx.y;
    const int lane = threadIdx.x;
    const int w = blockIdx.z*64 + lane;
    const double om = omega[w < W ? w : W - 1];
    cplx* I1 = I1s + lane;
    cplx* Z = Zs + lane;
    cplx acc[D2];
#pragma unroll
    for (int e = 0; e < D2; ++e) acc[e] = {0.0, 0.0};
    const int s_end = (c + 1)*L < G ? (c + 1)*L : G;
    const size_t rs = record_elems(D, A, H);
#pragma unroll 1
    for (int s = c*L; s < s_end; ++s) {
        const size_t seg = static_cast<size_t>(p)*G + s;
        __syncthreads();
        if (lane < 1 + 2*D2) head[lane] = rec[seg*rs + lane];
        if (lane < D2) Bs[lane] = rec[seg*rs + 1 + static_cast<size_t>(2 + a)*D2 + lane];
        __syncthreads();
        const cplx ph = cexp(om*hdr[1]);
        integrals_and_half_step<D>(om, hdr[0], dE, Ts, Bs, I1, Z);
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const cplx st = step_entry<D>(Ts, Z, ph, i, j);
                acc[i*D + j].re += st.re;
                acc[i*D + j].im += st.im;
            }
    }
    if (w >= W) return;
    cplx* dst = totals + ((static_cast<size_t>(p)*C + c)*A + a)*D2*W + w;
#pragma unroll
    for (int e = 0; e < D2; ++e) dst[static_cast<size_t>(e)*W] = acc[e];
}

// per pulse and element: totals[c] <- sum of totals[0..c-1] (in chunk order), ytot <- sum of all
__global__ __launch_bounds__(256) void gradb_prefix_kernel(cplx* __restrict__ totals, int C, size_t slab,
                                                           cplx* __restrict__ ytot) {
    const size_t i = static_cast<size_t>(blockIdx.x)*256 + threadIdx.x;
    if (i >= slab) return;
    const int p = blockIdx.y;
    cplx* col = totals + static_cast<size_t>(p)*C*slab + i;
    cplx run = {0.0, 0.0};
    for (int c = 0; c < C; ++c) {
        const cplx v = col[static_cast<size_t>(c)*slab];
        col[static_cast<size_t>(c)*slab] = run;
        run.re += v.re;
        run.im += v.im;
    }
    ytot[static_cast<size_t>(p)*slab + i] = run;
}

template <int D>
__global__ __launch_bounds__(64) void grad_batch_kernel(
    const double* __restrict__ omega, int W, const cplx* __restrict__ rec, const cplx* __restrict__ prefix,
    const cplx* __restrict__ ytot, const double* __restrict__ ratio, const cplx* __restrict__ scale, int s_ndim,
    int G, int A, int H, int L, int C, int P, double* __restrict__ dF, double* __restrict__ partial) {
    constexpr int D2 = D*D;
    extern __shared__ unsigned char smem[];
    const int lane = threadIdx.x;
    const gradwalk::SegmentLds<D> lds(smem, H, lane);
    const int c = blockIdx.x / A, a = blockIdx.x % A, p = blockIdx.y, tile = blockIdx.z;
    const int w = tile*64 + lane;
    const bool valid = w < W;
    const int wc = valid ? w : W - 1;
    const double om = omega[wc];
    double weight = 0.0;
    if (scale != nullptr && valid) weight = scale[(s_ndim == 2 ? static_cast<size_t>(a)*W : 0) + w].re;
    cplx Yd[D2], Yq[D2];                                   // Ytot^dag, Ycum
    {
        const cplx* tot = ytot + (static_cast<size_t>(p)*A + a)*D2*W + wc;
        const cplx* pre = prefix + ((static_cast<size_t>(p)*C + c)*A + a)*D2*W + wc;
#pragma unroll
        for (int x = 0; x < D; ++x)
#pragma unroll
            for (int y = 0; y < D; ++y) {
                const cplx v = tot[static_cast<size_t>(y*D + x)*W];
                Yd[x*D + y] = {v.re, -v.im};
                Yq[x*D + y] = pre[static_cast<size_t>(x*D + y)*W];
            }
    }
    const int s_end = (c + 1)*L < G ? (c + 1)*L : G;
    const size_t rs = record_elems(D, A, H);
    // everything below is addressed from this block's own rows: (p, a) fixed
    const size_t row0 = (static_cast<size_t>(p)*A + a)*G*H;
    rec += static_cast<size_t>(p)*G*rs;
    const int b_off = 1 + (2 + a)*D2, ae_off = 1 + (2 + A)*D2;
    if (ratio) ratio += (static_cast<size_t>(p)*A + a)*H*G;
    if (dF) dF += row0*W + w;
    if (partial) partial += static_cast<size_t>(tile)*P*A*G*H + row0;
#pragma unroll 1
    for (int s = c*L; s < s_end; ++s) {
        lds.load(rec + s*rs, b_off, ae_off, H, lane);
        gradwalk::segment_terms<D>(lds, om, H, lane, Yd, Yq, [&](int h, double val, double tr_step) {
            if (ratio) val += ratio[static_cast<size_t>(h)*G + s]*tr_step;
            const size_t row = static_cast<size_t>(s)*H + h;
            if (dF != nullptr && valid) dF[row*W] = val;
            if (partial != nullptr) {
                double sum = val*weight;                   // (lanes past W: weight 0)
                if (!valid) sum = 0.0;
                sum = gradwalk::lane_sum(sum);
                if (lane == 0) partial[row] = sum;
            }
        });
    }
}

// out[row] = (sum over tiles, in tile order, of partial[tile][row]) / d
__global__ __launch_bounds__(256) void gradb_reduce_kernel(const double* __restrict__ partial, int tiles, size_t rows,
                                                           double inv_d, double* __restrict__ out) {
    const size_t row = static_cast<size_t>(blockIdx.x)*256 + threadIdx.x;
    if (row >= rows) return;
    double sum = 0.0;
    for (int k = 0; k < tiles; ++k) sum += partial[static_cast<size_t>(k)*rows + row];
    out[row] = sum*inv_d;
}

template <int D>
hipError_t launch_walkers(const double* omega, int W, const cplx* rec, const double* ratio, const cplx* scale, int s_ndim, int P, int G, int A,
                          int H, int L, int C, cplx* totals, cplx* ytot, double* dF, double* partial,
                          hipStream_t stream) {
    const int tiles = (W + 63)/64;
    const dim3 grid(C*A, P, tiles);
    hipLaunchKernelGGL((gradb_totals_kernel<D>), grid, dim3(64), 0, stream, omega, W, rec, G, A, H, L, C,
                       totals);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const size_t slab = static_cast<size_t>(A)*D*D*W;
    hipLaunchKernelGGL(gradb_prefix_kernel, dim3(static_cast<unsigned>((slab + 255)/256), P), dim3(256), 0, stream,
                       totals, C, slab, ytot);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    const size_t lds = gradwalk::segment_lds_bytes(D, H);
    hipLaunchKernelGGL((grad_batch_kernel<D>), grid, dim3(64), lds, stream, omega, W, rec, totals, ytot, ratio, scale, s_ndim, G, A, H, L, C, P, dF, partial);
    return hipGetLastError();
}

}  // namespace

size_t grad_batch_record_elems(int d, int A, int H) { return record_elems(d, A, H); }

bool grad_batch_supported(int P, int W, int A, int H, int G, int d) {
    if (P < 1 || P > 65535 || W < 1 || A < 1 || A > 4 || H < 1 || H > 8 || G < 1 || G > 65535 || d < 2 || d > 4)
        return false;
    const int C = (G + grad_batch_chunk(G, d, W) - 1)/grad_batch_chunk(G, d, W);
    return (W + 63)/64 <= 65535 && static_cast<size_t>(C)*A <= 0x7fffffffull &&
           (static_cast<size_t>(A)*d*d*W + 255)/256 <= 0x7fffffffull;
}

hipError_t launch_grad_batch(int P, const double* eigvals, const cplx* eigvecs, const cplx* propagators,
                             const double* omega, int W, const cplx* n_opers, int A, const double* n_coeffs,
                             const cplx* c_opers, int H, const double* ratio, const double* dt, const double* t,
                             int G, int d, const cplx* scale, int s_ndim, cplx* rec, cplx* totals, cplx* ytot,
                             double* partial, double* dF, double* dI, hipStream_t stream) {
    if (!grad_batch_supported(P, W, A, H, G, d) || (dI != nullptr && (scale == nullptr || partial == nullptr)))
        return hipErrorInvalidValue;
    const int L = grad_batch_chunk(G, d, W), C = (G + L - 1)/L;
    hipLaunchKernelGGL(gradb_prologue_kernel, dim3(G, P), dim3(64), 0, stream, eigvals, eigvecs, propagators, n_opers,
                       n_coeffs, c_opers, dt, t, G, d, A, H, rec);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    double* part = dI != nullptr ? partial : nullptr;
    const cplx* sc = dI != nullptr ? scale : nullptr;
    switch (d) {
#define FFK_GRADB_CASE(D)                                                                                          \
    case D:                                                                                                        \
        err = launch_walkers<D>(omega, W, rec, ratio, sc, s_ndim, P, G, A, H, L, C, totals, ytot,  \
                                dF, part, stream);                                                                 \
        break;
        FFK_GRADB_CASE(2) FFK_GRADB_CASE(3) FFK_GRADB_CASE(4)
#undef FFK_GRADB_CASE
    default: return hipErrorInvalidValue;
    }
    if (err != hipSuccess || dI == nullptr) return err;
    const size_t rows = static_cast<size_t>(P)*A*G*H;
    if ((rows + 255)/256 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gradb_reduce_kernel, dim3(static_cast<unsigned>((rows + 255)/256)), dim3(256), 0, stream,
                       partial, (W + 63)/64, rows, 1.0/d, dI);
    return hipGetLastError();
}

// ---- the pieces of the pass that sequence_gradient.hip runs over a gate set (one "pulse" per gate) ----------------
hipError_t launch_grad_batch_records(int P, const double* eigvals, const cplx* eigvecs, const cplx* propagators,
                                     const cplx* n_opers, int A, const double* n_coeffs, const cplx* c_opers, int H,
                                     const double* dt, const double* t, int G, int d, cplx* rec, hipStream_t stream) {
    if (P < 1 || P > 65535 || G < 1 || G > 65535 || d < 2 || d > 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gradb_prologue_kernel, dim3(G, P), dim3(64), 0, stream, eigvals, eigvecs, propagators, n_opers,
                       n_coeffs, c_opers, dt, t, G, d, A, H, rec);
    return hipGetLastError();
}

hipError_t launch_grad_batch_pulse_totals(int P, const double* omega, int W, const cplx* rec, int G, int d, int A,
                                          int H, cplx* totals, hipStream_t stream) {
    if (P < 1 || P > 65535 || (W + 63)/64 > 65535) return hipErrorInvalidValue;
    const dim3 grid(A, P, (W + 63)/64);
    switch (d) {
#define FFK_GRADB_CASE(D)                                                                                          \
    case D:                                                                                                        \
        hipLaunchKernelGGL((gradb_totals_kernel<D>), grid, dim3(64), 0, stream, omega, W, rec, G, A, H, G, 1,      \
                           totals);                                                                                \
        break;
        FFK_GRADB_CASE(2) FFK_GRADB_CASE(3) FFK_GRADB_CASE(4)
#undef FFK_GRADB_CASE
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_grad_batch_reduce(const double* partial, int tiles, size_t rows, int d, double* out,
                                    hipStream_t stream) {
    if (rows < 1 || (rows + 255)/256 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gradb_reduce_kernel, dim3(static_cast<unsigned>((rows + 255)/256)), dim3(256), 0, stream,
                       partial, tiles, rows, 1.0/d, out);
    return hipGetLastError();
}

}  // namespace ffk

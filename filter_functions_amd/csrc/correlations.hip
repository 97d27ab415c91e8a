// correlations.hip -- the pulse-correlation infidelities I[g, h, alpha] of many gate sequences drawn from ONE table
// of distinct gates, in one pass (ff.correlation_infidelities, ffk_sequence_correlation_infidelities).  Single-qubit
// gates (d = 2, a Hermitian basis of N = 4 elements), A <= 4 noise operators, sequences of at most 256 positions.
//
// With the summands of the concatenation rule
//     X_g[alpha, k, w] = phi_g(w) sum_j v_{k_g}[alpha, j, w] Q^{(g-1)}[j, k],    phi_g = phi_{g-1} p_{k_{g-1}},
// (v_k the control matrix of distinct gate k, p_k = exp(i w tau_k), Q^{(g-1)} the Liouville representation of the
// propagator accumulated before position g) the result is
//     I[g, h, alpha] = sum_w (trapezoid weight S_alpha(w) / 2 pi d) Re sum_k conj(X_g[alpha, k, w]) X_h[alpha, k, w]:
// per noise operator a real Gram matrix Z diag(weights) Z^T of the G rows Z[g] = (Re X_g, Im X_g), inner length
// 2 N W, on v_mfma_f64_16x16x4_f64.  Neither the summands X nor anything of size G^2 W is written to memory.
//
//   correlation_prefix_kernel   thread = sequence: Q^{(g-1)} of every position, (n_index, 4, 4) f64
//   correlation_gram_kernel     grid (sequence, frequency slab, noise operator): per chunk of frequencies the block
//                               generates Z in LDS (position fastest), then every wavefront accumulates its own
//                               16 x 16 tile pairs (i <= j); one partial result per slab
//   correlation_reduce_kernel   thread = output element: the slabs summed in index order, the lower triangle the mirror
//                               of the upper
// The slabs are a function of W alone and a frequency's place in the accumulation order does not depend on the
// chunking: a sequence's result is the same bits in every pass and at every slot.
#include <algorithm>

#include "ffk_internal.h"

namespace ffk {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kCorrN = 4;                 // basis elements of d = 2
constexpr int kCorrLN = kCorrN*kCorrN;
constexpr int kCorrThreads = 256;
constexpr int kCorrWaves = kCorrThreads/64;
constexpr int kCorrQStride = kCorrLN + 1;  // doubles between the Q of two positions in LDS (odd: no bank conflicts)
constexpr int kCorrClasses = 4;

// Sequences are served by the instantiation of their length class: at most NT tiles of 16 positions, whose upper tile
// pairs are dealt to the four wavefronts by rows, FC frequencies per chunk.
template <int C> struct CorrClass;
template <> struct CorrClass<0> { static constexpr int NT = 2, FC = 16; };
template <> struct CorrClass<1> { static constexpr int NT = 4, FC = 16; };
template <> struct CorrClass<2> { static constexpr int NT = 8, FC = 8; };
template <> struct CorrClass<3> { static constexpr int NT = 16, FC = 4; };

template <int C>
constexpr size_t corr_lds_bytes() {
    return sizeof(double)*(static_cast<size_t>(CorrClass<C>::FC)*2*CorrClass<C>::NT*64 +
                           static_cast<size_t>(CorrClass<C>::NT)*16*kCorrQStride);
}

// Q^{(g-1)} for every position g of sequence p: the identity in front of the first, then each gate's Liouville
// representation multiplied on from the left (numeric.calculate_control_matrix_from_atomic's propagators_liouville,
// util.adot).
__global__ __launch_bounds__(kCorrThreads) void correlation_prefix_kernel(
    const double* __restrict__ Lpulse, const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, int P,
    double* __restrict__ Qc) {
    const int p = blockIdx.x*kCorrThreads + threadIdx.x;
    if (p >= P) return;
    double Q[kCorrLN];
#pragma unroll
    for (int e = 0; e < kCorrLN; ++e) Q[e] = (e % (kCorrN + 1)) == 0 ? 1.0 : 0.0;
    const int g_end = offsets[p + 1];
    for (int g = offsets[p]; g < g_end; ++g) {
        double* dst = Qc + static_cast<size_t>(g)*kCorrLN;
#pragma unroll
        for (int e = 0; e < kCorrLN; ++e) dst[e] = Q[e];
        if (g + 1 == g_end) break;
        const double* Lsrc = Lpulse + static_cast<size_t>(index[g])*kCorrLN;
        double Lk[kCorrLN], Nw[kCorrLN];
#pragma unroll
        for (int e = 0; e < kCorrLN; ++e) Lk[e] = Lsrc[e];
#pragma unroll
        for (int i = 0; i < kCorrN; ++i)
#pragma unroll
            for (int j = 0; j < kCorrN; ++j) {
                double acc = 0.0;
#pragma unroll
                for (int m = 0; m < kCorrN; ++m) acc = fma(Lk[i*kCorrN + m], Q[m*kCorrN + j], acc);
                Nw[i*kCorrN + j] = acc;
            }
#pragma unroll
        for (int e = 0; e < kCorrLN; ++e) Q[e] = Nw[e];
    }
}

// Block (member, slab, operator).  LDS: Z [frequency of the chunk][re | im][tile][k][position in tile] -- a
// wavefront's operand of one tile and one K-step (frequency, re | im) is 64 consecutive doubles, the lane map of both
// MFMA operands (position on lane & 15, basis element on lane >> 4) -- and the Q^{(g-1)} of the sequence's positions.
// The weight multiplies the A operand only (it may be negative).
template <int C>
__global__ __launch_bounds__(kCorrThreads) void correlation_gram_kernel(
    const cplx* __restrict__ phases, const cplx* const* __restrict__ Rtab, const double* __restrict__ Qc,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, const int64_t* __restrict__ out_offsets,
    const int32_t* __restrict__ members, int W, int slab_width, const cplx* __restrict__ scale, int s_ndim,
    const int32_t* __restrict__ idx, int n_idx, double inv_d, int64_t total, double* __restrict__ part) {
    constexpr int NT = CorrClass<C>::NT, FC = CorrClass<C>::FC;
    constexpr int NM = (NT + 7)/8, RP = NT + 1;     // row pairs per wavefront, tile pairs per row pair
    constexpr int PL = NT >= 4 ? NT/4 : 1;          // positions per lane while generating
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double* Zs = reinterpret_cast<double*>(lds_raw);
    double* Qs = Zs + static_cast<size_t>(FC)*2*NT*64;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p = members[blockIdx.x];
    const int slab = blockIdx.y, ia = blockIdx.z;
    const int a = idx[ia];
    const int g0 = offsets[p], G = offsets[p + 1] - g0;
    const int nt = (G + 15) >> 4;
    const int w_begin = slab*slab_width, w_end = min(W, w_begin + slab_width);
    const cplx* wrow = scale + static_cast<size_t>(s_ndim == 2 ? ia : 0)*W;

    for (int e = tid; e < G*kCorrLN; e += kCorrThreads)
        Qs[(e >> 4)*kCorrQStride + (e & 15)] = Qc[static_cast<size_t>(g0)*kCorrLN + e];
    // what a lane needs of its positions lane * PL ... lane * PL + PL - 1 at every frequency
    const cplx* vsrc[PL];
    int kprev[PL];
#pragma unroll
    for (int i = 0; i < PL; ++i) {
        const int g = lane*PL + i;
        vsrc[i] = g < G ? Rtab[index[g0 + g]] + static_cast<size_t>(a)*kCorrN*W : nullptr;
        kprev[i] = (g >= 1 && g < G) ? index[g0 + g - 1] : -1;
    }
    __syncthreads();
    // This wavefront's tile pairs: tile row i = wave + 4 m together with row nt - 1 - i, nt + 1 upper pairs in all --
    // pair r is (i, i + r) while r < nt - i, then (nt - 1 - i, r - 1).  Every B operand lies at a compile-time offset
    // from the row's or the image's first tile, the A operand is one register per row.
    int rowA[NM], rowB[NM], nA[NM], nAB[NM];          // (nA pairs in row A, nAB in both rows; 0: no row pair)
    f64x4 acc[NM][RP];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        rowA[m] = wave + kCorrWaves*m;
        rowB[m] = nt - 1 - rowA[m];
        nA[m] = rowA[m] <= rowB[m] ? nt - rowA[m] : 0;
        nAB[m] = rowA[m] < rowB[m] ? nt + 1 : nA[m];
#pragma unroll
        for (int r = 0; r < RP; ++r) acc[m][r] = f64x4{0.0, 0.0, 0.0, 0.0};
    }

    for (int c0 = w_begin; c0 < w_end; c0 += FC) {
        const int nf = min(FC, w_end - c0);
        __syncthreads();                      // the previous chunk's operands have been read
        // ---- generate: one wavefront per frequency, the running product of the phases as a wavefront scan
        for (int fl = wave; fl < nf; fl += kCorrWaves) {
            const int w = c0 + fl;
            cplx ph[PL];
            cplx run = {1.0, 0.0};
#pragma unroll
            for (int i = 0; i < PL; ++i) {
                if (kprev[i] >= 0) run = cmul(run, phases[static_cast<size_t>(kprev[i])*W + w]);
                ph[i] = run;
            }
            cplx t = run;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const cplx o = {__shfl_up(t.re, off, 64), __shfl_up(t.im, off, 64)};
                if (lane >= off) t = cmul(o, t);
            }
            cplx before = {__shfl_up(t.re, 1, 64), __shfl_up(t.im, 1, 64)};
            if (lane == 0) before = {1.0, 0.0};
#pragma unroll
            for (int i = 0; i < PL; ++i) {
                const int g = lane*PL + i;
                const int tile = g >> 4, pos = g & 15;
                if (tile >= nt) continue;
                cplx X[kCorrN];
#pragma unroll
                for (int k = 0; k < kCorrN; ++k) X[k] = {0.0, 0.0};
                if (g < G) {               // (a padded position of the last tile stays exactly zero)
                    const cplx phi = cmul(before, ph[i]);
                    const double* Qg = Qs + g*kCorrQStride;
                    cplx s[kCorrN];
#pragma unroll
                    for (int k = 0; k < kCorrN; ++k) s[k] = {0.0, 0.0};
#pragma unroll
                    for (int j = 0; j < kCorrN; ++j) {
                        const cplx v = vsrc[i][static_cast<size_t>(j)*W + w];
#pragma unroll
                        for (int k = 0; k < kCorrN; ++k) {
                            const double q = Qg[j*kCorrN + k];
                            s[k].re = fma(v.re, q, s[k].re);
                            s[k].im = fma(v.im, q, s[k].im);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < kCorrN; ++k) X[k] = cmul(phi, s[k]);
                }
                double* zre = Zs + (static_cast<size_t>(fl*2)*nt + tile)*64 + pos;
                double* zim = zre + static_cast<size_t>(nt)*64;
#pragma unroll
                for (int k = 0; k < kCorrN; ++k) {
                    zre[k*16] = X[k].re;
                    zim[k*16] = X[k].im;
                }
            }
        }
        __syncthreads();
        // ---- accumulate: two K-steps (re, im) per frequency for each of the wavefront's tile pairs
        for (int fl = 0; fl < nf; ++fl) {
            const double wgt = wrow[c0 + fl].re*inv_d;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const double* base = Zs + static_cast<size_t>(fl*2 + c)*nt*64 + lane;
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    // (the counts pass through an empty asm statement: compared in front of every MFMA, they cost a
                    // scalar compare each; hoisted out of the loops, the 2 x 34 results do not fit the scalar registers)
                    int n_a = nA[m], n_ab = nAB[m];
                    asm volatile("" : "+s"(n_a), "+s"(n_ab));
                    if (n_a == 0) continue;
                    const double* in_row = base + rowA[m]*64;
                    const double za = in_row[0]*wgt;
                    const double zb = base[rowB[m]*64]*wgt;
#pragma unroll
                    for (int r = 0; r < RP; ++r) {
                        if (r < n_a)
                            acc[m][r] = __builtin_amdgcn_mfma_f64_16x16x4f64(za, in_row[r*64], acc[m][r], 0, 0, 0);
                        else if (r < n_ab)
                            acc[m][r] = __builtin_amdgcn_mfma_f64_16x16x4f64(zb, base[(r - 1)*64], acc[m][r], 0, 0, 0);
                    }
                }
            }
        }
    }
    // D of v_mfma_f64_16x16x4_f64: column lane & 15, row (lane >> 4) + 4 reg
    double* dst = part + (static_cast<size_t>(slab)*n_idx + ia)*static_cast<size_t>(total) + out_offsets[p];
    const int col = lane & 15, row0 = lane >> 4;
#pragma unroll
    for (int m = 0; m < NM; ++m) {
#pragma unroll
        for (int r = 0; r < RP; ++r) {
            if (r >= nAB[m]) continue;
            const int ti = r < nA[m] ? rowA[m] : rowB[m], tj = r < nA[m] ? rowA[m] + r : r - 1;
            const int h = tj*16 + col;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int g = ti*16 + row0 + 4*reg;
                if (g < G && h < G) dst[static_cast<size_t>(g)*G + h] = acc[m][r][reg];
            }
        }
    }
}

// out[(cell, ia)] = sum over the slabs, in index order, of the partial of the cell's upper-triangle twin
__global__ __launch_bounds__(kCorrThreads) void correlation_reduce_kernel(
    const double* __restrict__ part, const int64_t* __restrict__ out_offsets, const int32_t* __restrict__ offsets,
    int P, int n_idx, int slabs, int64_t total, double* __restrict__ out) {
    const int64_t e = static_cast<int64_t>(blockIdx.x)*kCorrThreads + threadIdx.x;
    if (e >= total*n_idx) return;
    const int64_t cell = e / n_idx;
    const int ia = static_cast<int>(e % n_idx);
    int lo = 0, hi = P - 1;                 // the sequence p with out_offsets[p] <= cell < out_offsets[p + 1]
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (out_offsets[mid] <= cell) lo = mid; else hi = mid - 1;
    }
    const int G = offsets[lo + 1] - offsets[lo];
    const int64_t local = cell - out_offsets[lo];
    const int g = static_cast<int>(local / G), h = static_cast<int>(local % G);
    const int64_t src = out_offsets[lo] + static_cast<int64_t>(min(g, h))*G + max(g, h);
    double sum = 0.0;
    for (int s = 0; s < slabs; ++s) sum += part[(static_cast<size_t>(s)*n_idx + ia)*static_cast<size_t>(total) + src];
    out[e] = sum;
}

template <int C>
hipError_t launch_gram_class(const cplx* phases, const cplx* const* Rtab, const double* Qc, const int32_t* offsets,
                             const int32_t* index, const int64_t* out_offsets, const int32_t* members, int count, int W,
                             const cplx* scale, int s_ndim, const int32_t* idx, int n_idx, int d, int64_t total,
                             double* part, hipStream_t stream) {
    if (count < 1) return hipSuccess;
    constexpr size_t lds = corr_lds_bytes<C>();
    static_assert(lds <= 160*1024, "LDS of a CU");
    if (lds > 48*1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(correlation_gram_kernel<C>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) return e;
    }
    int width = 0;
    const int slabs = correlation_slabs(W, &width);
    hipLaunchKernelGGL(correlation_gram_kernel<C>, dim3(count, slabs, n_idx), dim3(kCorrThreads), lds, stream, phases,
                       Rtab, Qc, offsets, index, out_offsets, members, W, width, scale, s_ndim, idx, n_idx, 1.0/d,
                       total, part);
    return hipGetLastError();
}

}  // namespace

int correlation_max_length() { return CorrClass<kCorrClasses - 1>::NT*16; }

int correlation_class(int G) {
    if (G <= CorrClass<0>::NT*16) return 0;
    if (G <= CorrClass<1>::NT*16) return 1;
    if (G <= CorrClass<2>::NT*16) return 2;
    return 3;
}

int correlation_slabs(int W, int* width) {
    const int w = 16*((W + 511)/512);
    if (width) *width = w;
    return (W + w - 1)/w;
}

hipError_t launch_correlation_prefix(const double* Lpulse, const int32_t* offsets, const int32_t* index, int P,
                                     double* Qc, hipStream_t stream) {
    if (P < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(correlation_prefix_kernel, dim3((P + kCorrThreads - 1)/kCorrThreads), dim3(kCorrThreads), 0,
                       stream, Lpulse, offsets, index, P, Qc);
    return hipGetLastError();
}

hipError_t launch_correlation_gram(const cplx* phases, const cplx* const* Rtab, const double* Qc,
                                   const int32_t* offsets, const int32_t* index, const int64_t* out_offsets,
                                   const int32_t* members, const int* class_counts, int W, const cplx* scale,
                                   int s_ndim, const int32_t* idx, int n_idx, int d, int64_t total, double* part,
                                   hipStream_t stream) {
    if (W < 1 || n_idx < 1 || n_idx > 4 || (s_ndim != 1 && s_ndim != 2) || d < 1 || total < 1)
        return hipErrorInvalidValue;
    const int32_t* m = members;
#define FFK_CORR_CLASS(C)                                                                                          \
    if (hipError_t e = launch_gram_class<C>(phases, Rtab, Qc, offsets, index, out_offsets, m, class_counts[C], W,     \
                                            scale, s_ndim, idx, n_idx, d, total, part, stream))                       \
        return e;                                                                                                  \
    m += class_counts[C];
    FFK_CORR_CLASS(0) FFK_CORR_CLASS(1) FFK_CORR_CLASS(2) FFK_CORR_CLASS(3)
#undef FFK_CORR_CLASS
    return hipSuccess;
}

hipError_t launch_correlation_reduce(const double* part, const int64_t* out_offsets, const int32_t* offsets, int P,
                                     int n_idx, int W, int64_t total, double* out, hipStream_t stream) {
    const int64_t blocks = (total*n_idx + kCorrThreads - 1)/kCorrThreads;
    if (P < 1 || blocks < 1 || blocks > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(correlation_reduce_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kCorrThreads), 0, stream,
                       part, out_offsets, offsets, P, n_idx, correlation_slabs(W, nullptr), total, out);
    return hipGetLastError();
}

}  // namespace ffk

// correlations_d4.hip -- the pulse-correlation infidelities of correlations.hip for two-qubit gates (d = 4, a Hermitian
// basis of N = 16 elements, A <= 4 noise operators, sequences of at most 256 positions):
// ff.sequence_correlation_infidelities, ffk_sequence_correlation_infidelities4.
//
// The same arithmetic,
//     X_g[alpha, k, w] = phi_g(w) sum_j v_{k_g}[alpha, j, w] Q^{(g-1)}[j, k],    phi_g = prod_{j < g} p_{k_j},
//     I[g, h, alpha] = sum_w (trapezoid weight S_alpha(w) / 2 pi d) Re sum_k conj(X_g[alpha, k, w]) X_h[alpha, k, w],
// per noise operator a real Gram matrix of the G rows (Re X_g, Im X_g) with an inner length of 32 per frequency: eight
// K-steps of v_mfma_f64_16x16x4_f64 per tile pair and frequency (re | im, four basis elements each).
//
//   correlations4_prefix_kernel   block = sequence, thread = element of the 16 x 16 product: Q^{(g-1)} of every
//                                 position, (n_index, 16, 16) f64
//   correlations4_gram_kernel     grid (sequence, frequency slab, noise operator), the structure of
//                                 correlation_gram_kernel: per chunk of frequencies the block generates the summands in
//                                 LDS -- thread = (position, frequency), vector FMAs, Q^{(g-1)} read from L2 --, then
//                                 every wavefront accumulates its own 16 x 16 tile pairs (i <= j); one partial result
//                                 per slab, added by correlation_reduce_kernel
// Slabs, length classes and the reduction are those of correlations.hip: the slabs are a function of W alone, a
// frequency's place in the order of the sum and the association of a position's phase product depend on the sequence
// alone, so a sequence's result is the same bits in every pass and at every slot.
#include "ffk_internal.h"

namespace ffk {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kC4N = 16;                  // basis elements of d = 4
constexpr int kC4LN = kC4N*kC4N;
constexpr int kC4Threads = 256;
constexpr int kC4Waves = kC4Threads/64;
constexpr int kC4Steps = 2*kC4N/4;        // K-steps per frequency: (re | im) x four groups of four basis elements

// A length class serves at most NT tiles of 16 positions; a chunk is the 256 / (16 NT) frequencies at which the
// block's threads are one (position, frequency) each.  The image of a chunk is 64 KiB in every class.
template <int C> struct Corr4Class;
template <> struct Corr4Class<0> { static constexpr int NT = 2; };
template <> struct Corr4Class<1> { static constexpr int NT = 4; };
template <> struct Corr4Class<2> { static constexpr int NT = 8; };
template <> struct Corr4Class<3> { static constexpr int NT = 16; };

template <int C>
constexpr size_t corr4_lds_bytes() {
    constexpr int FC = kC4Threads/(16*Corr4Class<C>::NT);
    return sizeof(double)*(static_cast<size_t>(FC)*kC4Steps*Corr4Class<C>::NT*64) + sizeof(cplx)*kC4Waves;
}

// Q^{(g-1)} for every position g of sequence blockIdx.x: the identity in front of the first, then each gate's
// Liouville representation multiplied on from the left.  Thread (i, j) keeps element [i, j]; the previous product is
// read from LDS (two buffers, one barrier per position).
__global__ __launch_bounds__(kC4Threads) void correlations4_prefix_kernel(
    const double* __restrict__ Lpulse, const int32_t* __restrict__ offsets, const int32_t* __restrict__ index,
    double* __restrict__ Qc) {
    __shared__ double Qs[2][kC4LN];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int i = tid >> 4, j = tid & 15;
    double q = i == j ? 1.0 : 0.0;
    int buf = 0;
    const int g_end = offsets[p + 1];
    for (int g = offsets[p]; g < g_end; ++g) {
        Qc[static_cast<size_t>(g)*kC4LN + tid] = q;
        if (g + 1 == g_end) break;
        Qs[buf][tid] = q;
        __syncthreads();
        const double* Lrow = Lpulse + static_cast<size_t>(index[g])*kC4LN + i*kC4N;
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < kC4N; ++m) acc = fma(Lrow[m], Qs[buf][m*kC4N + j], acc);
        q = acc;
        buf ^= 1;
    }
}

// Block (member, slab, operator).  LDS: Z [frequency of the chunk][re | im][group of four basis elements][tile]
// [k in the group][position in tile] -- a wavefront's operand of one tile and one K-step is 64 consecutive doubles, the
// lane map of both MFMA operands (position on lane & 15, basis element on lane >> 4) -- and the wavefronts' phase
// products.  The weight multiplies the A operand only (it may be negative).
template <int C>
__global__ __launch_bounds__(kC4Threads) void correlations4_gram_kernel(
    const cplx* __restrict__ phases, const cplx* const* __restrict__ Rtab, const double* __restrict__ Qc,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, const int64_t* __restrict__ out_offsets,
    const int32_t* __restrict__ members, int W, int slab_width, const cplx* __restrict__ scale, int s_ndim,
    const int32_t* __restrict__ idx, int n_idx, double inv_d, int64_t total, double* __restrict__ part) {
    constexpr int NT = Corr4Class<C>::NT;
    constexpr int POS = 16*NT, FC = kC4Threads/POS;  // positions of the longest member, frequencies per chunk
    constexpr int SEG = POS < 64 ? POS : 64;         // lanes of a wavefront that share a frequency
    constexpr int WPF = POS/SEG;                     // wavefronts per frequency
    constexpr int NM = (NT + 7)/8, RP = NT + 1;      // row pairs per wavefront, tile pairs per row pair
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double* Zs = reinterpret_cast<double*>(lds_raw);
    cplx* carry = reinterpret_cast<cplx*>(Zs + static_cast<size_t>(FC)*kC4Steps*NT*64);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p = members[blockIdx.x];
    const int slab = blockIdx.y, ia = blockIdx.z;
    const int a = idx[ia];
    const int g0 = offsets[p], G = offsets[p + 1] - g0;
    const int nt = (G + 15) >> 4;
    const int w_begin = slab*slab_width, w_end = min(W, w_begin + slab_width);
    const cplx* wrow = scale + static_cast<size_t>(s_ndim == 2 ? ia : 0)*W;

    // what this thread generates in every chunk: position g at the chunk's frequency gen_f
    const int g = tid % POS, gen_f = tid / POS;
    const cplx* vsrc = g < G ? Rtab[index[g0 + g]] + static_cast<size_t>(a)*kC4N*W : nullptr;
    const int kprev = (g >= 1 && g < G) ? index[g0 + g - 1] : -1;
    const double* Qg = Qc + static_cast<size_t>(g0 + (g < G ? g : 0))*kC4LN;
    // This wavefront's tile pairs, as in correlation_gram_kernel: tile row i = wave + 4 m together with row
    // nt - 1 - i, nt + 1 upper pairs in all -- pair r is (i, i + r) while r < nt - i, then (nt - 1 - i, r - 1).
    int rowA[NM], rowB[NM], nA[NM], nAB[NM];          // (nA pairs in row A, nAB in both rows; 0: no row pair)
    f64x4 acc[NM][RP];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        rowA[m] = wave + kC4Waves*m;
        rowB[m] = nt - 1 - rowA[m];
        nA[m] = rowA[m] <= rowB[m] ? nt - rowA[m] : 0;
        nAB[m] = rowA[m] < rowB[m] ? nt + 1 : nA[m];
#pragma unroll
        for (int r = 0; r < RP; ++r) acc[m][r] = f64x4{0.0, 0.0, 0.0, 0.0};
    }

    for (int c0 = w_begin; c0 < w_end; c0 += FC) {
        const int nf = min(FC, w_end - c0);
        const int w = min(c0 + gen_f, w_end - 1);
        // ---- the phase in front of every position: a scan over the lanes that share a frequency, then the products
        // of the wavefronts in front (every thread takes part, whatever it generates)
        cplx t = {1.0, 0.0};
        if (kprev >= 0) t = phases[static_cast<size_t>(kprev)*W + w];
#pragma unroll
        for (int off = 1; off < SEG; off <<= 1) {
            const cplx o = {__shfl_up(t.re, off, SEG), __shfl_up(t.im, off, SEG)};
            if ((lane & (SEG - 1)) >= off) t = cmul(o, t);
        }
        __syncthreads();                      // the previous chunk's operands and products have been read
        if (WPF > 1) {
            if (lane == 63) carry[wave] = t;
            __syncthreads();
            for (int v = wave - wave % WPF; v < wave; ++v) t = cmul(carry[v], t);
        }
        // ---- generate: X[k] = phi sum_j v[j] Q[j, k]; a padded position of the last tile stays exactly zero
        if (gen_f < nf && (g >> 4) < nt) {
            cplx s[kC4N];
#pragma unroll
            for (int k = 0; k < kC4N; ++k) s[k] = {0.0, 0.0};
            if (g < G) {
#pragma unroll 2
                for (int j = 0; j < kC4N; ++j) {
                    const cplx v = vsrc[static_cast<size_t>(j)*W + w];
                    const double* Qrow = Qg + j*kC4N;
#pragma unroll
                    for (int k = 0; k < kC4N; ++k) {
                        const double q = Qrow[k];
                        s[k].re = fma(v.re, q, s[k].re);
                        s[k].im = fma(v.im, q, s[k].im);
                    }
                }
#pragma unroll
                for (int k = 0; k < kC4N; ++k) s[k] = cmul(t, s[k]);
            }
            double* zre = Zs + (static_cast<size_t>(gen_f)*kC4Steps*nt + (g >> 4))*64 + (g & 15);
            double* zim = zre + static_cast<size_t>(4*nt)*64;
#pragma unroll
            for (int k = 0; k < kC4N; ++k) {
                zre[static_cast<size_t>(k >> 2)*nt*64 + (k & 3)*16] = s[k].re;
                zim[static_cast<size_t>(k >> 2)*nt*64 + (k & 3)*16] = s[k].im;
            }
        }
        __syncthreads();
        // ---- accumulate: eight K-steps per frequency for each of the wavefront's tile pairs
        for (int fl = 0; fl < nf; ++fl) {
            const double wgt = wrow[c0 + fl].re*inv_d;
#pragma unroll 1
            for (int c = 0; c < kC4Steps; ++c) {
                const double* base = Zs + static_cast<size_t>(fl*kC4Steps + c)*nt*64 + lane;
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    // (the counts pass through an empty asm statement, as in correlation_gram_kernel: compared in
                    // front of every MFMA they cost a scalar compare each and stay out of the scalar registers)
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
                const int gr = ti*16 + row0 + 4*reg;
                if (gr < G && h < G) dst[static_cast<size_t>(gr)*G + h] = acc[m][r][reg];
            }
        }
    }
}

template <int C>
hipError_t launch_gram4_class(const cplx* phases, const cplx* const* Rtab, const double* Qc, const int32_t* offsets,
                              const int32_t* index, const int64_t* out_offsets, const int32_t* members, int count,
                              int W, const cplx* scale, int s_ndim, const int32_t* idx, int n_idx, int d, int64_t total,
                              double* part, hipStream_t stream) {
    if (count < 1) return hipSuccess;
    constexpr size_t lds = corr4_lds_bytes<C>();
    static_assert(lds <= 160*1024, "LDS of a CU");
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(correlations4_gram_kernel<C>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) return e;
    int width = 0;
    const int slabs = correlation_slabs(W, &width);
    hipLaunchKernelGGL(correlations4_gram_kernel<C>, dim3(count, slabs, n_idx), dim3(kC4Threads), lds, stream, phases,
                       Rtab, Qc, offsets, index, out_offsets, members, W, width, scale, s_ndim, idx, n_idx, 1.0/d,
                       total, part);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_correlations4_prefix(const double* Lpulse, const int32_t* offsets, const int32_t* index, int P,
                                       double* Qc, hipStream_t stream) {
    if (P < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(correlations4_prefix_kernel, dim3(P), dim3(kC4Threads), 0, stream, Lpulse, offsets, index, Qc);
    return hipGetLastError();
}

hipError_t launch_correlations4_gram(const cplx* phases, const cplx* const* Rtab, const double* Qc,
                                     const int32_t* offsets, const int32_t* index, const int64_t* out_offsets,
                                     const int32_t* members, const int* class_counts, int W, const cplx* scale,
                                     int s_ndim, const int32_t* idx, int n_idx, int d, int64_t total, double* part,
                                     hipStream_t stream) {
    if (W < 1 || n_idx < 1 || n_idx > 4 || (s_ndim != 1 && s_ndim != 2) || d < 1 || total < 1)
        return hipErrorInvalidValue;
    static_assert(Corr4Class<3>::NT*16 == 256, "the classes of correlation_class");
    const int32_t* m = members;
#define FFK_CORR4_CLASS(C)                                                                                         \
    if (hipError_t e = launch_gram4_class<C>(phases, Rtab, Qc, offsets, index, out_offsets, m, class_counts[C], W,    \
                                             scale, s_ndim, idx, n_idx, d, total, part, stream))                      \
        return e;                                                                                                  \
    m += class_counts[C];
    FFK_CORR4_CLASS(0) FFK_CORR4_CLASS(1) FFK_CORR4_CLASS(2) FFK_CORR4_CLASS(3)
#undef FFK_CORR4_CLASS
    return hipSuccess;
}

}  // namespace ffk

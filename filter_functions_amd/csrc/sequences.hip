// sequences.hip -- many gate sequences drawn from ONE table of distinct gates, concatenated in one pass
// (ff.concatenate_sequences, ffk_concatenate_sequences_resident).  Single-qubit gates (d = 2, a Hermitian
// basis of N = 4 elements) with A <= 4 noise operators.
//
// The concatenation rule of a sequence k_0 ... k_{G-1} as the backward recurrence of the single block kernel
// (atomic.hip, the comment above its Lpulse branch), here over a WHOLE sequence:
//     S_g = v_{k_g} + p_{k_g} (S_{g+1} L_{k_g}),    S_G = 0,    R = S_0
// with v_k the control matrix of distinct gate k, p_k = exp(i omega tau_k) and L_k the Liouville representation
// of its total propagator.  Every operand comes from a table of the T distinct gates, shared by all sequences of
// the pass: no cumulative propagator and no phase prefix is formed, and a sequence's result does not depend on
// which other sequences share the pass.
//
//   sequences_front_kernel   one launch: phases (T, W), L_k (T, N, N) and each sequence's total propagator
//   sequences_rule_kernel    grid (omega tiles of 64, sequence groups): a block stages the T tables of its tile in
//                            LDS once (STAGED) or reads them from L2, every wavefront walks whole sequences
//                            (lane = frequency) and writes R (P, A, N, W) and F (P, A, A, W)
#include <algorithm>

#include "ffk_internal.h"

namespace ffk {
namespace {

constexpr int kSeqN = 4;               // basis elements of d = 2
constexpr int kSeqFrontThreads = 256;
constexpr int kSeqGlobalWaves = 4;
// STAGED: one block per CU holds the tables, sixteen wavefronts share them (eight for A = 4: its 16 accumulators
// need more than the 128 registers a wavefront of a 1024-thread block may hold)
constexpr int seq_staged_waves(int A) { return A >= 4 ? 8 : 16; }

// L[i,j] = tr(U^dag C_i U C_j) of a 2 x 2 propagator (superoperator.py:51-84), the contraction order of
// sequence_front_kernel's representation
__device__ __forceinline__ void represent_d2(const cplx (&M)[4], const cplx* __restrict__ C, double* __restrict__ dst) {
    for (int i = 0; i < kSeqN; ++i) {
        const cplx* Ci = C + i*4;
        cplx CM[4], CB[4];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                cplx acc = {0.0, 0.0};
#pragma unroll
                for (int k = 0; k < 2; ++k) cmac(acc, Ci[r*2 + k], M[k*2 + c]);
                CM[r*2 + c] = acc;
            }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                cplx acc = {0.0, 0.0};
#pragma unroll
                for (int k = 0; k < 2; ++k) cmac_conj(acc, M[k*2 + a], CM[k*2 + b]);
                CB[a*2 + b] = acc;
            }
        for (int j = 0; j < kSeqN; ++j) {
            const cplx* Cj = C + j*4;
            cplx acc = {0.0, 0.0};
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) cmac(acc, CB[a*2 + b], Cj[b*2 + a]);
            dst[i*kSeqN + j] = acc.re;
        }
    }
}

// Blocks [0, phase_blocks): phases[k, w] = exp(i omega_w tau_k) (util.cexp).  Blocks [phase_blocks,
// phase_blocks + seq_blocks): thread p forms sequence p's total propagator U_{k_{G-1}} ... U_{k_0} as an ordered
// product (the single path's scan associates the same factors differently).  The remaining blocks: L_k of the
// distinct gates.
__global__ __launch_bounds__(kSeqFrontThreads) void sequences_front_kernel(
    const cplx* __restrict__ U, const double* __restrict__ tau, const double* __restrict__ omega, int T, int W,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, int P, const cplx* __restrict__ basis,
    unsigned phase_blocks, unsigned seq_blocks, cplx* __restrict__ phases, double* __restrict__ Lpulse,
    cplx* __restrict__ Qtot) {
    const unsigned b = blockIdx.x;
    if (b < phase_blocks) {
        const size_t e = static_cast<size_t>(b)*kSeqFrontThreads + threadIdx.x;
        if (e < static_cast<size_t>(T)*W) {
            const int k = static_cast<int>(e / W), w = static_cast<int>(e % W);
            phases[e] = cexp(omega[w]*tau[k]);
        }
        return;
    }
    if (b < phase_blocks + seq_blocks) {
        const int p = static_cast<int>(b - phase_blocks)*kSeqFrontThreads + threadIdx.x;
        if (p >= P) return;
        cplx M[4] = {{1.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {1.0, 0.0}};
        for (int g = offsets[p]; g < offsets[p + 1]; ++g) {
            const cplx* Ug = U + static_cast<size_t>(index[g])*4;
            cplx E[4], Pm[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) E[e] = Ug[e];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    cplx acc = {0.0, 0.0};
#pragma unroll
                    for (int k = 0; k < 2; ++k) cmac(acc, E[i*2 + k], M[k*2 + j]);
                    Pm[i*2 + j] = acc;
                }
#pragma unroll
            for (int e = 0; e < 4; ++e) M[e] = Pm[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) Qtot[static_cast<size_t>(p)*4 + e] = M[e];
        return;
    }
    __shared__ cplx Cs[kSeqN*4];
    if (threadIdx.x < kSeqN*4) Cs[threadIdx.x] = basis[threadIdx.x];
    __syncthreads();
    const int k = static_cast<int>(b - phase_blocks - seq_blocks)*kSeqFrontThreads + threadIdx.x;
    if (k >= T) return;
    cplx Uk[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) Uk[e] = U[static_cast<size_t>(k)*4 + e];
    represent_d2(Uk, Cs, Lpulse + static_cast<size_t>(k)*kSeqN*kSeqN);
}

// One block: 64 frequencies (lane = frequency) and one group of sequences.  Work item j (sequences sorted by
// length, longest first: order[j]) goes to wavefront q = j mod Q of the Q = n_groups x waves wavefronts of the
// tile, q = wave * n_groups + group: each block gets every n_groups-th item, its wavefronts every Q-th.
// STAGED: the T control matrices and phases of the tile in LDS, T (4 A + 1) KiB; else read where they lie (L2).
template <int A, bool STAGED>
__global__ __launch_bounds__(STAGED ? 64*seq_staged_waves(A) : 64*kSeqGlobalWaves) void sequences_rule_kernel(
    const cplx* __restrict__ phases, const cplx* const* __restrict__ Rtab, const double* __restrict__ Lpulse,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, const int32_t* __restrict__ order,
    int P, int T, int W, int n_groups, cplx* __restrict__ R, cplx* __restrict__ F) {
    constexpr int N = kSeqN;
    constexpr int ROWS = A*N;
    constexpr int LN = N*N;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_waves = blockDim.x >> 6;
    const int w = blockIdx.x*64 + lane;
    const int wc = w < W ? w : W - 1;
    cplx* Rs = reinterpret_cast<cplx*>(lds_raw);                      // [T][ROWS][64]
    cplx* Ps = Rs + static_cast<size_t>(T)*ROWS*64;                   // [T][64]
    if (STAGED) {
        for (int e = wave; e < T*ROWS; e += n_waves) {
            const int k = e / ROWS, r = e % ROWS;
            Rs[static_cast<size_t>(e)*64 + lane] = Rtab[k][static_cast<size_t>(r)*W + wc];
        }
        for (int k = wave; k < T; k += n_waves) Ps[k*64 + lane] = phases[static_cast<size_t>(k)*W + wc];
        __syncthreads();
    }
    const int Q = n_groups*n_waves;
    for (int j = wave*n_groups + blockIdx.y; j < P; j += Q) {
        const int p = order[j];
        const int g_begin = offsets[p], g_end = offsets[p + 1];
        cplx S[ROWS];
#pragma unroll
        for (int e = 0; e < ROWS; ++e) S[e] = {0.0, 0.0};
        // positions from the last to the first, 64 at a time: the chunk's gate numbers in one coalesced load
        // (lane l holds position c0 + l), one v_readlane per position
        for (int c1 = g_end; c1 > g_begin; c1 -= 64) {
            const int c0 = max(g_begin, c1 - 64);
            const int my_index = c0 + lane < c1 ? index[c0 + lane] : 0;
            for (int g = c1 - 1; g >= c0; --g) {
                const int k = __builtin_amdgcn_readlane(my_index, g - c0);
                double Lk[LN];
                const double* Lsrc = Lpulse + static_cast<size_t>(k)*LN;
#pragma unroll
                for (int e = 0; e < LN; ++e) Lk[e] = Lsrc[e];
                const cplx* Rg = STAGED ? Rs + static_cast<size_t>(k)*ROWS*64 + lane : Rtab[k] + wc;
                const size_t rstride = STAGED ? 64 : static_cast<size_t>(W);
                const cplx ph = STAGED ? Ps[k*64 + lane] : phases[static_cast<size_t>(k)*W + wc];
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    cplx t[N];
#pragma unroll
                    for (int jj = 0; jj < N; ++jj) t[jj] = {0.0, 0.0};
#pragma unroll
                    for (int kk = 0; kk < N; ++kk)
#pragma unroll
                        for (int jj = 0; jj < N; ++jj) {
                            const double q = Lk[kk*N + jj];
                            t[jj].re = fma(q, S[a*N + kk].re, t[jj].re);
                            t[jj].im = fma(q, S[a*N + kk].im, t[jj].im);
                        }
#pragma unroll
                    for (int jj = 0; jj < N; ++jj) {
                        const cplx v = Rg[(a*N + jj)*rstride];
                        S[a*N + jj] = {fma(ph.re, t[jj].re, fma(-ph.im, t[jj].im, v.re)),
                                       fma(ph.re, t[jj].im, fma(ph.im, t[jj].re, v.im))};
                    }
                }
            }
        }
        if (w < W) {
            // (R == NULL: ffk_sequence_infidelities keeps the filter function only)
            if (R) {
                cplx* Rp = R + static_cast<size_t>(p)*ROWS*W + w;
#pragma unroll
                for (int e = 0; e < ROWS; ++e) Rp[static_cast<size_t>(e)*W] = S[e];
            }
            // F[a,b] = sum_k conj(R[a,k]) R[b,k] with the arithmetic of ff_fidelity_kernel (a <= b, mirrored,
            // diagonal imaginary part 0)
            cplx* Fp = F + static_cast<size_t>(p)*A*A*W + w;
#pragma unroll
            for (int a = 0; a < A; ++a)
#pragma unroll
                for (int bb = a; bb < A; ++bb) {
                    cplx f = {0.0, 0.0};
#pragma unroll
                    for (int kk = 0; kk < N; ++kk) cmac_conj(f, S[a*N + kk], S[bb*N + kk]);
                    if (a == bb) f.im = 0.0;
                    Fp[static_cast<size_t>(a*A + bb)*W] = f;
                    if (a != bb) Fp[static_cast<size_t>(bb*A + a)*W] = {f.re, -f.im};
                }
        }
    }
}

size_t staged_lds_bytes(int T, int A) {
    return static_cast<size_t>(T)*(A*kSeqN + 1)*64*sizeof(cplx);
}

}  // namespace

bool sequences_supported(int d, int N, int A) {
    return d == 2 && N == kSeqN && A >= 1 && A <= 4;
}

bool sequences_staged(int T, int A) {
    return staged_lds_bytes(T, A) <= 150*1024;
}

int sequences_groups(int P, int W, int A, bool staged) {
    const long tiles = (W + 63)/64;
    const long waves = staged ? seq_staged_waves(A) : kSeqGlobalWaves;
    // enough blocks for every CU (staged: one block per CU, its LDS holds the tables), never more groups than
    // there are wavefronts' worth of sequences
    const long target = staged ? 512 : 2048;
    long groups = (target + tiles - 1)/tiles;
    groups = std::min(groups, (P + waves - 1)/waves);
    return static_cast<int>(std::max(1L, std::min(groups, 65535L)));
}

hipError_t launch_sequences_front(const cplx* U, const double* tau, const double* omega, int T, int W,
                                  const int32_t* offsets, const int32_t* index, int P, const cplx* basis,
                                  cplx* phases, double* Lpulse, cplx* Qtot, hipStream_t stream) {
    const size_t pb = (static_cast<size_t>(T)*W + kSeqFrontThreads - 1)/kSeqFrontThreads;
    const size_t sb = (static_cast<size_t>(P) + kSeqFrontThreads - 1)/kSeqFrontThreads;
    const size_t lb = (static_cast<size_t>(T) + kSeqFrontThreads - 1)/kSeqFrontThreads;
    if (pb + sb + lb > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sequences_front_kernel, dim3(static_cast<unsigned>(pb + sb + lb)), dim3(kSeqFrontThreads), 0,
                       stream, U, tau, omega, T, W, offsets, index, P, basis, static_cast<unsigned>(pb),
                       static_cast<unsigned>(sb), phases, Lpulse, Qtot);
    return hipGetLastError();
}

hipError_t launch_sequences_rule(const cplx* phases, const cplx* const* Rtab, const double* Lpulse,
                                 const int32_t* offsets, const int32_t* index, const int32_t* order, int P, int T,
                                 int A, int W, cplx* R, cplx* F, hipStream_t stream) {
    if (A < 1 || A > 4 || P < 1 || T < 1 || W < 1) return hipErrorInvalidValue;
    const bool staged = sequences_staged(T, A);
    const int groups = sequences_groups(P, W, A, staged);
    const dim3 grid((W + 63)/64, groups);
    auto launch = [&](auto kern, int waves, size_t lds) -> hipError_t {
        if (lds > 48*1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     static_cast<int>(lds));
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, grid, dim3(64*waves), lds, stream, phases, Rtab, Lpulse, offsets, index, order, P, T,
                           W, groups, R, F);
        return hipGetLastError();
    };
#define FFK_SEQ_RULE(AA)                                                                                        \
    case AA:                                                                                                    \
        return staged ? launch(sequences_rule_kernel<AA, true>, seq_staged_waves(AA), staged_lds_bytes(T, AA))      \
                      : launch(sequences_rule_kernel<AA, false>, kSeqGlobalWaves, 0);
    switch (A) {
        FFK_SEQ_RULE(1) FFK_SEQ_RULE(2) FFK_SEQ_RULE(3) FFK_SEQ_RULE(4)
        default: return hipErrorInvalidValue;
    }
#undef FFK_SEQ_RULE
}

}  // namespace ffk

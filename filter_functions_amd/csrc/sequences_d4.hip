// sequences_d4.hip -- the sequence pass of sequences.hip for two-qubit gates (d = 4, a Hermitian basis of N = 16
// elements, A <= 4 noise operators): ff.sequence_infidelities, ffk_sequence_infidelities.
//
// The same backward recurrence over a whole sequence k_0 ... k_{G-1},
//     S_g = v_{k_g} + p_{k_g} (S_{g+1} L_{k_g}),    S_G = 0,    R = S_0,
// with the 16 x 16 product on v_mfma_f64_16x16x4_f64 (A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
// D[row = (lane >> 4) + 4 r][col = lane & 15] in register r).  A tile is one noise operator at sixteen frequencies
// (col = frequency); the product is taken transposed, T^T = L^T S^T, and K-step r carries the basis elements
// {q + 4 r : q = 0..3}: its A operand is L[(q + 4 r) 16 + i] at lane (i, q), its B operand is register r of the
// previous position's result -- D's row map is that choice of K-steps, so S never leaves its registers and is never
// transposed.
// Real and imaginary parts are two accumulator tiles on the same lanes: the phase multiplies B lane by lane
// (p (S L) = (p S) L), v is the C input of the first K-step, and one chain of four instructions per tile yields S_g.
// A wavefront walks whole sequences at 64 frequencies: 4 tiles x A x 2 independent chains, 64 A accumulator registers
// (A = 3 and 4: 32 frequencies, two tiles, so that nothing spills).
//
//   sequences4_front_kernel   one launch: phases (T, W), L_k (T, 16, 16) and each sequence's total propagator
//   sequences4_rule_kernel    grid (omega tiles of 64, sequence groups): F (P, A, A, W) from the registers; the control
//                             matrix R is never written
#include <algorithm>

#include "sequence_walk.h"

namespace ffk {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kD = 4;
constexpr int kDD = kD*kD;
constexpr int kN = 16;                  // basis elements of d = 4
constexpr int kFrontThreads = 256;
constexpr int kRuleWaves = 4;           // one wavefront per SIMD: the whole register file of 512 each

// C = A B of 4 x 4 matrices in registers
__device__ __forceinline__ void matmul4(const cplx (&A)[kDD], const cplx (&B)[kDD], cplx (&C)[kDD]) {
#pragma unroll
    for (int i = 0; i < kD; ++i)
#pragma unroll
        for (int j = 0; j < kD; ++j) {
            cplx acc = {0.0, 0.0};
#pragma unroll
            for (int k = 0; k < kD; ++k) cmac(acc, A[i*kD + k], B[k*kD + j]);
            C[i*kD + j] = acc;
        }
}

// Blocks [0, phase_blocks): phases[k, w] = exp(i omega_w tau_k) (util.cexp).  Blocks [phase_blocks, phase_blocks +
// seq_blocks): thread p forms sequence p's total propagator U_{k_{G-1}} ... U_{k_0} as an ordered product.  The
// remaining blocks: thread (k, i) forms row i of L_k[i, j] = tr(U_k^dag C_i U_k C_j) (superoperator.py:51-84, the
// contraction order of represent_d2).
__global__ __launch_bounds__(kFrontThreads) void sequences4_front_kernel(
    const cplx* __restrict__ U, const double* __restrict__ tau, const double* __restrict__ omega, int T, int W,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, int P, const cplx* __restrict__ basis,
    unsigned phase_blocks, unsigned seq_blocks, cplx* __restrict__ phases, double* __restrict__ Lpulse,
    cplx* __restrict__ Qtot) {
    const unsigned b = blockIdx.x;
    if (b < phase_blocks) {
        const size_t e = static_cast<size_t>(b)*kFrontThreads + threadIdx.x;
        if (e < static_cast<size_t>(T)*W) {
            const int k = static_cast<int>(e / W), w = static_cast<int>(e % W);
            phases[e] = cexp(omega[w]*tau[k]);
        }
        return;
    }
    if (b < phase_blocks + seq_blocks) {
        const int p = static_cast<int>(b - phase_blocks)*kFrontThreads + threadIdx.x;
        if (p >= P) return;
        cplx M[kDD];
#pragma unroll
        for (int e = 0; e < kDD; ++e) M[e] = {e % (kD + 1) == 0 ? 1.0 : 0.0, 0.0};
        for (int g = offsets[p]; g < offsets[p + 1]; ++g) {
            const cplx* Ug = U + static_cast<size_t>(index[g])*kDD;
            cplx E[kDD], Pm[kDD];
#pragma unroll
            for (int e = 0; e < kDD; ++e) E[e] = Ug[e];
            matmul4(E, M, Pm);
#pragma unroll
            for (int e = 0; e < kDD; ++e) M[e] = Pm[e];
        }
#pragma unroll
        for (int e = 0; e < kDD; ++e) Qtot[static_cast<size_t>(p)*kDD + e] = M[e];
        return;
    }
    __shared__ cplx Cs[kN*kDD];
    for (int e = threadIdx.x; e < kN*kDD; e += kFrontThreads) Cs[e] = basis[e];
    __syncthreads();
    const int item = static_cast<int>(b - phase_blocks - seq_blocks)*kFrontThreads + threadIdx.x;
    if (item >= T*kN) return;
    const int k = item / kN, i = item % kN;
    cplx Uk[kDD], Ci[kDD], CM[kDD], CB[kDD];
#pragma unroll
    for (int e = 0; e < kDD; ++e) {
        Uk[e] = U[static_cast<size_t>(k)*kDD + e];
        Ci[e] = Cs[i*kDD + e];
    }
    matmul4(Ci, Uk, CM);
#pragma unroll
    for (int a = 0; a < kD; ++a)
#pragma unroll
        for (int c = 0; c < kD; ++c) {
            cplx acc = {0.0, 0.0};
#pragma unroll
            for (int m = 0; m < kD; ++m) cmac_conj(acc, Uk[m*kD + a], CM[m*kD + c]);
            CB[a*kD + c] = acc;
        }
    double* dst = Lpulse + (static_cast<size_t>(k)*kN + i)*kN;
    for (int j = 0; j < kN; ++j) {
        const cplx* Cj = Cs + j*kDD;
        cplx acc = {0.0, 0.0};
#pragma unroll
        for (int a = 0; a < kD; ++a)
#pragma unroll
            for (int c = 0; c < kD; ++c) cmac(acc, CB[a*kD + c], Cj[c*kD + a]);
        dst[j] = acc.re;
    }
}

using seqwalk::seq4_tiles;               // tiles of sixteen frequencies a wavefront walks at once

// One block: 16 TILES frequencies and one group of sequences, dealt out as in sequences_rule_kernel (work item j of
// the sequences sorted by length, longest first, goes to wavefront j mod Q).  Lane (c, q) = (lane & 15, lane >> 4)
// holds, in register r of tile t of noise operator a, S[a, q + 4 r] at frequency 16 TILES blockIdx.x + 16 t + c.
// STAGED: the T control matrices and phases of the block's frequencies in LDS, T (16 A + 1) TILES / 4 KiB; else read
// where they lie (L2).
template <int A, bool STAGED>
__global__ __launch_bounds__(64*kRuleWaves) void sequences4_rule_kernel(
    const cplx* __restrict__ phases, const cplx* const* __restrict__ Rtab, const double* __restrict__ Lpulse,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, const int32_t* __restrict__ order,
    int P, int T, int W, int n_groups, cplx* __restrict__ F) {
    constexpr int N = kN;
    constexpr int ROWS = A*N;
    constexpr int TILES = seq4_tiles(A);
    constexpr int WT = 16*TILES;                                      // frequencies of a block
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_waves = blockDim.x >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int w0 = blockIdx.x*WT;
    cplx* Rs = reinterpret_cast<cplx*>(lds_raw);                      // [T][ROWS][WT]
    cplx* Ps = Rs + static_cast<size_t>(T)*ROWS*WT;                   // [T][WT]
    if (STAGED) {
        const int x = lane % WT, wl = min(w0 + x, W - 1);
        for (int e = wave*(64/WT) + lane/WT; e < T*ROWS; e += n_waves*(64/WT)) {
            const int k = e / ROWS, r = e % ROWS;
            Rs[static_cast<size_t>(e)*WT + x] = Rtab[k][static_cast<size_t>(r)*W + wl];
        }
        for (int k = wave*(64/WT) + lane/WT; k < T; k += n_waves*(64/WT))
            Ps[k*WT + x] = phases[static_cast<size_t>(k)*W + wl];
        __syncthreads();
    }
    // the column of this lane in tile t: in LDS, or the (clamped) frequency in memory
    size_t col[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t) col[t] = STAGED ? size_t(16*t + c) : size_t(min(w0 + 16*t + c, W - 1));
    const size_t rstride = STAGED ? WT : static_cast<size_t>(W);
    const int Q = n_groups*n_waves;
    for (int j = wave*n_groups + blockIdx.y; j < P; j += Q) {
        const int p = order[j];
        const int g_begin = offsets[p], g_end = offsets[p + 1];
        f64x4 Sre[A][TILES], Sim[A][TILES];
#pragma unroll
        for (int a = 0; a < A; ++a)
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                Sre[a][t] = {0.0, 0.0, 0.0, 0.0};
                Sim[a][t] = {0.0, 0.0, 0.0, 0.0};
            }
        // positions from the last to the first, 64 at a time: the chunk's gate numbers in one coalesced load
        // (lane l holds position c0 + l), one v_readlane per position
        for (int c1 = g_end; c1 > g_begin; c1 -= 64) {
            const int c0 = max(g_begin, c1 - 64);
            const int my_index = c0 + lane < c1 ? index[c0 + lane] : 0;
            for (int g = c1 - 1; g >= c0; --g) {
                const int k = __builtin_amdgcn_readlane(my_index, g - c0);
                const double* Lsrc = Lpulse + static_cast<size_t>(k)*N*N + c;
                double La[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) La[r] = Lsrc[(q + 4*r)*N];
                const cplx* Rg = STAGED ? Rs + static_cast<size_t>(k)*ROWS*WT : Rtab[k];
                const cplx* Pg = STAGED ? Ps + k*WT : phases + static_cast<size_t>(k)*W;
#pragma unroll
                for (int t = 0; t < TILES; ++t) {
                    const cplx ph = Pg[col[t]];
#pragma unroll
                    for (int a = 0; a < A; ++a) {
                        f64x4 bre, bim, vre, vim;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            bre[r] = fma(ph.re, Sre[a][t][r], -(ph.im*Sim[a][t][r]));
                            bim[r] = fma(ph.re, Sim[a][t][r], ph.im*Sre[a][t][r]);
                            const cplx v = Rg[(a*N + q + 4*r)*rstride + col[t]];
                            vre[r] = v.re;
                            vim[r] = v.im;
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            vre = __builtin_amdgcn_mfma_f64_16x16x4f64(La[r], bre[r], vre, 0, 0, 0);
                            vim = __builtin_amdgcn_mfma_f64_16x16x4f64(La[r], bim[r], vim, 0, 0, 0);
                        }
                        Sre[a][t] = vre;
                        Sim[a][t] = vim;
                    }
                }
            }
        }
        // F[a,b] = sum_k conj(R[a,k]) R[b,k] (a <= b, mirrored, diagonal imaginary part 0): the four registers of a
        // lane, then the four lane groups in the order 0..3.  Lane group q < TILES keeps tile q: frequency w0 + lane.
        const int w = lane < WT ? w0 + lane : W;
        cplx* Fp = F + static_cast<size_t>(p)*A*A*W + w;
#pragma unroll
        for (int a = 0; a < A; ++a)
#pragma unroll
            for (int bb = a; bb < A; ++bb) {
                cplx mine = {0.0, 0.0};
#pragma unroll
                for (int t = 0; t < TILES; ++t) {
                    cplx f = {0.0, 0.0};
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        cmac_conj(f, cplx{Sre[a][t][r], Sim[a][t][r]}, cplx{Sre[bb][t][r], Sim[bb][t][r]});
                    cplx sum = {__shfl(f.re, c), __shfl(f.im, c)};
#pragma unroll
                    for (int qq = 1; qq < 4; ++qq) {
                        sum.re += __shfl(f.re, c + 16*qq);
                        sum.im += __shfl(f.im, c + 16*qq);
                    }
                    if (q == t) mine = sum;
                }
                if (a == bb) mine.im = 0.0;
                if (w < W) {
                    Fp[static_cast<size_t>(a*A + bb)*W] = mine;
                    if (a != bb) Fp[static_cast<size_t>(bb*A + a)*W] = {mine.re, -mine.im};
                }
            }
    }
}

size_t staged_lds_bytes(int T, int A) {
    return static_cast<size_t>(T)*(A*kN + 1)*16*seq4_tiles(A)*sizeof(cplx);
}

}  // namespace

bool sequences4_supported(int d, int N, int A) {
    return d == kD && N == kN && A >= 1 && A <= 4;
}

bool sequences4_staged(int T, int A) {
    return staged_lds_bytes(T, A) <= 150*1024;
}

int sequences4_groups(int P, int W, int A, bool staged) {
    const long tiles = (W + 16*seq4_tiles(A) - 1)/(16*seq4_tiles(A));
    // staged: one block per CU (its LDS holds the tables); else a few blocks per CU.  Never more groups than there are
    // wavefronts' worth of sequences
    const long target = staged ? 256 : 1024;
    long groups = (target + tiles - 1)/tiles;
    groups = std::min(groups, (static_cast<long>(P) + kRuleWaves - 1)/kRuleWaves);
    return static_cast<int>(std::max(1L, std::min(groups, 65535L)));
}

hipError_t launch_sequences4_front(const cplx* U, const double* tau, const double* omega, int T, int W,
                                   const int32_t* offsets, const int32_t* index, int P, const cplx* basis,
                                   cplx* phases, double* Lpulse, cplx* Qtot, hipStream_t stream) {
    const size_t pb = (static_cast<size_t>(T)*W + kFrontThreads - 1)/kFrontThreads;
    const size_t sb = (static_cast<size_t>(P) + kFrontThreads - 1)/kFrontThreads;
    const size_t lb = (static_cast<size_t>(T)*kN + kFrontThreads - 1)/kFrontThreads;
    if (pb + sb + lb > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sequences4_front_kernel, dim3(static_cast<unsigned>(pb + sb + lb)), dim3(kFrontThreads), 0,
                       stream, U, tau, omega, T, W, offsets, index, P, basis, static_cast<unsigned>(pb),
                       static_cast<unsigned>(sb), phases, Lpulse, Qtot);
    return hipGetLastError();
}

hipError_t launch_sequences4_rule(const cplx* phases, const cplx* const* Rtab, const double* Lpulse,
                                  const int32_t* offsets, const int32_t* index, const int32_t* order, int P, int T,
                                  int A, int W, cplx* F, hipStream_t stream) {
    if (A < 1 || A > 4 || P < 1 || T < 1 || W < 1) return hipErrorInvalidValue;
    const bool staged = sequences4_staged(T, A);
    const int groups = sequences4_groups(P, W, A, staged);
    const int wt = 16*seq4_tiles(A);
    const dim3 grid((W + wt - 1)/wt, groups);
    auto launch = [&](auto kern, size_t lds) -> hipError_t {
        if (lds > 48*1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     static_cast<int>(lds));
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, grid, dim3(64*kRuleWaves), lds, stream, phases, Rtab, Lpulse, offsets, index, order,
                           P, T, W, groups, F);
        return hipGetLastError();
    };
#define FFK_SEQ4_RULE(AA)                                                                                       \
    case AA:                                                                                                    \
        return staged ? launch(sequences4_rule_kernel<AA, true>, staged_lds_bytes(T, AA))                        \
                      : launch(sequences4_rule_kernel<AA, false>, 0);
    switch (A) {
        FFK_SEQ4_RULE(1) FFK_SEQ4_RULE(2) FFK_SEQ4_RULE(3) FFK_SEQ4_RULE(4)
        default: return hipErrorInvalidValue;
    }
#undef FFK_SEQ4_RULE
}

}  // namespace ffk

// sequence_processes.hip -- decay amplitudes of many gate sequences drawn from one table of distinct gates, formed from
// the registers of the concatenation rule at the end of each sequence (ff.sequence_decay_amplitudes,
// ff.sequence_cumulant_functions, ff.sequence_error_transfer_matrices; ffk_sequence_processes).
//
// The walk is the one of sequences.hip (d = 2) and sequences_d4.hip (d = 4): the same grid (frequency tiles x
// sequence groups), the same dealing of the sequences sorted by length, the same recurrence
//     S_g = v_{k_g} + p_{k_g} (S_{g+1} L_{k_g}),    S_G = 0,    R = S_0
// with the same arithmetic, so R in registers is what those kernels hold.  Only the epilogue differs:
//     Gamma[a, k, l] = sum_w c_w S_a(w) (Re R[a,k,w] Re R[a,l,w] + Im R[a,k,w] Im R[a,l,w])
// over the block's frequencies, c_w S_a(w) the real weights of launch_spectral_weights, for every selected operator
// and every spectrum of the call.  Nothing of size W is stored per sequence: a block writes its partial tile to
// partial[frequency block][p][spectrum][i_idx][N][N] and sequence_processes_reduce_kernel adds the frequency blocks
// in index order.  No atomics, no waits between wavefronts or blocks, a block width that depends on A alone: a
// sequence's Gamma is the same bits whatever else is in the pass.
//
//   sequences_gamma_kernel    d = 2: lane = frequency; per lane the ten products k <= l, summed over the wavefront
//                             with a fixed butterfly, lane 0 stores the tile and mirrors it
//   sequences4_gamma_kernel   d = 4: a 16 x 16 Gram matrix over the frequency axis on v_mfma_f64_16x16x4_f64 (operand
//                             maps: header comment of sequences_d4.hip).  After the walk lane (c, q) holds
//                             R[a, q + 4 r] at frequency 16 t + c; the A operand of K-step s of tile t is
//                             R[a, k = lane & 15] at frequency 16 t + 4 s + (lane >> 4), the B operand the same entry
//                             times the weight.  That is the transpose of what the registers hold: each wavefront
//                             moves one (operator, tile) pair of 16 x 16 blocks (real, imaginary) through two padded
//                             LDS tiles of its own and reads them back transposed -- a wavefront reads only what it
//                             wrote, no block barrier.  Real and imaginary products go to accumulators of their own
//                             and are added at the end; spectra beyond the first reuse the transposed R and only
//                             change the weights.
#include "sequence_walk.h"

namespace ffk {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

using seqwalk::seq4_tiles;
using seqwalk::weight_row;

// ---- d = 2 -------------------------------------------------------------------------------------------------------
constexpr int kSeqN = 4;
constexpr int kSeqGlobalWaves = 4;
constexpr int seq_staged_waves(int A) { return A >= 4 ? 8 : 16; }      // (as sequences.hip)

template <int A, bool STAGED>
__global__ __launch_bounds__(STAGED ? 64*seq_staged_waves(A) : 64*kSeqGlobalWaves) void sequences_gamma_kernel(
    const cplx* __restrict__ phases, const cplx* const* __restrict__ Rtab, const double* __restrict__ Lpulse,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, const int32_t* __restrict__ order,
    int P, int T, int W, int n_groups, const cplx* __restrict__ scale, int s_ndim, int n_spectra,
    const int32_t* __restrict__ idx, int n_idx, double* __restrict__ partial) {
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
        // Gamma of this tile: lanes beyond W carry weight 0 (the clamped column they hold does not contribute)
        double* tile0 = partial + ((static_cast<size_t>(blockIdx.x)*P + p)*n_spectra)*n_idx*LN;
#pragma unroll
        for (int a = 0; a < A; ++a)
            for (int i = 0; i < n_idx; ++i) {
                if (idx[i] != a) continue;
                for (int sp = 0; sp < n_spectra; ++sp) {
                    const double wt = w < W ? weight_row(scale, s_ndim, n_idx, sp, i, W)[wc].re : 0.0;
                    double gsum[10];
                    int e = 0;
#pragma unroll
                    for (int k = 0; k < N; ++k) {
                        const double bre = wt*S[a*N + k].re, bim = wt*S[a*N + k].im;
#pragma unroll
                        for (int l = k; l < N; ++l, ++e) gsum[e] = fma(S[a*N + l].re, bre, S[a*N + l].im*bim);
                    }
#pragma unroll
                    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
                        for (int x = 0; x < 10; ++x) gsum[x] += __shfl_xor(gsum[x], m);
                    if (lane == 0) {
                        double* o = tile0 + (static_cast<size_t>(sp)*n_idx + i)*LN;
                        e = 0;
#pragma unroll
                        for (int k = 0; k < N; ++k)
#pragma unroll
                            for (int l = k; l < N; ++l, ++e) {
                                o[k*N + l] = gsum[e];
                                o[l*N + k] = gsum[e];
                            }
                    }
                }
            }
    }
}

size_t staged2_lds_bytes(int T, int A) {
    return static_cast<size_t>(T)*(A*kSeqN + 1)*64*sizeof(cplx);
}

// ---- d = 4 -------------------------------------------------------------------------------------------------------
constexpr int kN = 16;
constexpr int kRuleWaves = 4;
constexpr int kPad = 17;                                   // doubles of a row of the transposition tiles
constexpr int kScratch = 2*kN*kPad;                        // doubles of one wavefront's two tiles (4352 bytes)

template <int A, bool STAGED>
__global__ __launch_bounds__(64*kRuleWaves) void sequences4_gamma_kernel(
    const cplx* __restrict__ phases, const cplx* const* __restrict__ Rtab, const double* __restrict__ Lpulse,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, const int32_t* __restrict__ order,
    int P, int T, int W, int n_groups, const cplx* __restrict__ scale, int s_ndim, int n_spectra,
    const int32_t* __restrict__ idx, int n_idx, double* __restrict__ partial) {
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
    // the wavefronts' transposition tiles first, the staged tables behind them
    double* scr = reinterpret_cast<double*>(lds_raw) + wave*kScratch;
    cplx* Rs = reinterpret_cast<cplx*>(lds_raw + kRuleWaves*kScratch*sizeof(double));      // [T][ROWS][WT]
    cplx* Ps = Rs + static_cast<size_t>(T)*ROWS*WT;                                       // [T][WT]
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
        // Gamma of this block's frequencies.  Tiles t = 0 .. TILES - 1 in order, K-steps 0 .. 3 inside; the lane's
        // frequency of K-step s of tile t is w0 + 16 t + 4 s + q, weight 0 beyond W.
        double* tile0 = partial + ((static_cast<size_t>(blockIdx.x)*P + p)*n_spectra)*n_idx*N*N;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            bool selected = false;
            for (int i = 0; i < n_idx; ++i) selected |= idx[i] == a;
            if (!selected) continue;
            double Tre[TILES][4], Tim[TILES][4];
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                wave_sync();                                   // (the reads of the block before are done)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    scr[(q + 4*r)*kPad + c] = Sre[a][t][r];
                    scr[kN*kPad + (q + 4*r)*kPad + c] = Sim[a][t][r];
                }
                wave_sync();
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    Tre[t][s] = scr[c*kPad + 4*s + q];
                    Tim[t][s] = scr[kN*kPad + c*kPad + 4*s + q];
                }
            }
            for (int i = 0; i < n_idx; ++i) {
                if (idx[i] != a) continue;
                for (int sp = 0; sp < n_spectra; ++sp) {
                    const cplx* sc = weight_row(scale, s_ndim, n_idx, sp, i, W);
                    f64x4 acc_re = {0.0, 0.0, 0.0, 0.0}, acc_im = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int t = 0; t < TILES; ++t)
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const int wl = w0 + 16*t + 4*s + q;
                            const double wt = wl < W ? sc[min(wl, W - 1)].re : 0.0;
                            acc_re = __builtin_amdgcn_mfma_f64_16x16x4f64(Tre[t][s], wt*Tre[t][s], acc_re, 0, 0, 0);
                            acc_im = __builtin_amdgcn_mfma_f64_16x16x4f64(Tim[t][s], wt*Tim[t][s], acc_im, 0, 0, 0);
                        }
                    f64x4 acc = acc_re + acc_im;
                    // the entries below the diagonal are those above it: symmetric bit for bit
                    wave_sync();
#pragma unroll
                    for (int r = 0; r < 4; ++r) scr[(q + 4*r)*kPad + c] = acc[r];
                    wave_sync();
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (q + 4*r > c) acc[r] = scr[c*kPad + q + 4*r];
                    double* o = tile0 + (static_cast<size_t>(sp)*n_idx + i)*N*N;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[(q + 4*r)*N + c] = acc[r];
                }
            }
        }
    }
}

size_t staged4_lds_bytes(int T, int A) {
    return static_cast<size_t>(T)*(A*kN + 1)*16*seq4_tiles(A)*sizeof(cplx);
}
constexpr size_t kScratchBytes = static_cast<size_t>(kRuleWaves)*kScratch*sizeof(double);

// out[sp][p][i] = sum over the frequency blocks, in index order, of partial[fb][p][sp][i]; tile = N*N doubles
__global__ __launch_bounds__(256) void sequence_processes_reduce_kernel(const double* __restrict__ partial, int blocks,
                                                                        int P, int n_spectra, size_t row,
                                                                        double* __restrict__ out) {
    const size_t n = static_cast<size_t>(P)*n_spectra*row;
    const size_t o = static_cast<size_t>(blockIdx.x)*256 + threadIdx.x;
    if (o >= n) return;
    const size_t e = o % row, sp_p = o / row;
    const size_t p = sp_p % P, sp = sp_p / P;
    const size_t src = (p*n_spectra + sp)*row + e;
    double acc = partial[src];
    for (int b = 1; b < blocks; ++b) acc += partial[static_cast<size_t>(b)*n + src];
    out[o] = acc;
}

}  // namespace

int sequence_processes_block_width(int d, int A) {
    return d == 2 ? 64 : 16*seq4_tiles(A);
}

bool sequence_processes_staged(int d, int T, int A) {
    if (d == 2) return staged2_lds_bytes(T, A) <= 150*1024;
    return staged4_lds_bytes(T, A) + kScratchBytes <= 150*1024;
}

hipError_t launch_sequences_gamma(int d, const cplx* phases, const cplx* const* Rtab, const double* Lpulse,
                                  const int32_t* offsets, const int32_t* index, const int32_t* order, int P, int T,
                                  int A, int W, const cplx* scale, int s_ndim, int n_spectra, const int32_t* idx,
                                  int n_idx, double* partial, double* gamma, hipStream_t stream) {
    if (A < 1 || A > 4 || P < 1 || T < 1 || W < 1 || n_spectra < 1 || n_idx < 1 || n_idx > A ||
        (s_ndim != 1 && s_ndim != 2) || (d != 2 && d != 4))
        return hipErrorInvalidValue;
    const bool staged = sequence_processes_staged(d, T, A);
    const int width = sequence_processes_block_width(d, A);
    const int blocks = (W + width - 1)/width;
    const int groups = d == 2 ? sequences_groups(P, W, A, staged) : sequences4_groups(P, W, A, staged);
    const dim3 grid(blocks, groups);
    auto launch = [&](auto kern, int waves, size_t lds) -> hipError_t {
        if (lds > 48*1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     static_cast<int>(lds));
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, grid, dim3(64*waves), lds, stream, phases, Rtab, Lpulse, offsets, index, order, P, T,
                           W, groups, scale, s_ndim, n_spectra, idx, n_idx, partial);
        return hipGetLastError();
    };
    hipError_t err = hipErrorInvalidValue;
#define FFK_SEQ_GAMMA(AA)                                                                                          \
    case AA:                                                                                                       \
        if (d == 2)                                                                                                \
            err = staged ? launch(sequences_gamma_kernel<AA, true>, seq_staged_waves(AA), staged2_lds_bytes(T, AA))  \
                         : launch(sequences_gamma_kernel<AA, false>, kSeqGlobalWaves, 0);                          \
        else                                                                                                       \
            err = staged ? launch(sequences4_gamma_kernel<AA, true>, kRuleWaves,                                   \
                                  staged4_lds_bytes(T, AA) + kScratchBytes)                                        \
                         : launch(sequences4_gamma_kernel<AA, false>, kRuleWaves, kScratchBytes);                  \
        break;
    switch (A) {
        FFK_SEQ_GAMMA(1) FFK_SEQ_GAMMA(2) FFK_SEQ_GAMMA(3) FFK_SEQ_GAMMA(4)
        default: break;
    }
#undef FFK_SEQ_GAMMA
    if (err != hipSuccess) return err;
    const size_t row = static_cast<size_t>(n_idx)*d*d*d*d;
    const size_t n = static_cast<size_t>(P)*n_spectra*row;
    if ((n + 255)/256 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sequence_processes_reduce_kernel, dim3(static_cast<unsigned>((n + 255)/256)), dim3(256), 0,
                       stream, partial, blocks, P, n_spectra, row, gamma);
    return hipGetLastError();
}

}  // namespace ffk

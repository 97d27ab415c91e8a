// sequence_second_order.hip -- frequency shifts (second order) of many gate sequences drawn from one table of distinct
// gates, in one walk of each sequence (ff.sequence_frequency_shifts; ffk_sequence_frequency_shifts).
//
// The rotated concatenation rule of the second-order filter function (numeric.
// calculate_second_order_filter_function_from_atomic), integrated against the spectrum, is
//     Delta = sum_g [ Lam_g^T Delta_gate(k_g) Lam_g  +  sum_w c_w S_a(w) Re( conj(Rs_g[k, w]) Cum_{g-1}[l, w] ) ]
// with Lam_g the Liouville matrix of the propagator before position g, Rs_g = phi_{g-1} (R_{k_g} Lam_g) the rule's
// summand and Cum_{g-1} the sum of the summands before it.  The walk goes FORWARD through the sequence and carries
//     Lam_{g+1} = L_{k_g} Lam_g                       (16 x 16 or 4 x 4 real, the same for every frequency)
//     X_g       = R_{k_g} Lam_g                       (the summand without its phase)
//     C_g       = conj(p_{k_g}) (C_{g-1} + X_g)       (= conj(phi_g) Cum_g: only the gate's own phase is needed)
//     Z        += sum_w c_w S_a(w) (Re X_g[k] Re C_{g-1}[l] + Im X_g[k] Im C_{g-1}[l])  [+ Lam_g^T Delta_gate Lam_g]
// The common phase phi_{g-1} of Rs_g and Cum_{g-1} cancels in conj(.)(.).  The forward form is chosen because the
// frequency-dependent operand of its product, the gate's control matrix, comes from the table at every position and
// can be read in either operand layout, while the other operand, Lam, lies in the accumulator layout of the matrix
// instruction, which is an operand layout for a contraction over its rows.  X_g then comes out with the frequency
// along the rows -- the layout of both operands of a Gram matrix over the frequencies -- and nothing is ever
// transposed, neither per sequence nor per position (the backward recurrence of sequences_d4.hip holds its state with
// the frequency along the columns and would need an LDS round trip per position and operator).
//
// Z is linear in the weights: a block forms the partial Z of its frequencies and seq2o_reduce_kernel adds the blocks
// in index order.  The gates' own shifts are frequency independent: frequency block 0 adds them.  No atomics, no
// waits between wavefronts or blocks, a block width that depends on d and A alone, and at most kSpectra spectra per
// walk (grid z carries the further ones): a sequence's result is the same bits whatever else is in the pass.
//
//   seq2o_walk2_kernel   d = 2: lane = frequency; Lam, C and Z (4 x 4 per operator and spectrum) per lane; one
//                        butterfly per sequence; lane 0 of block 0 carries the gates' own shifts
//   seq2o_walk4_kernel   d = 4: v_mfma_f64_16x16x4_f64 (operand maps: header comment of sequences_d4.hip).  Lam is
//                        held as D[row = q + 4 r][col = c] (c = lane & 15, q = lane >> 4, register r).  K-step s of
//                        X = R Lam has the A operand R[a, q + 4 s] at frequency 16 t + c (the read of the rule
//                        kernel) and the B operand register s of Lam; X and C are D tiles with row = frequency
//                        16 t + q + 4 r, col = basis element c.  K-step r of the Gram has the A operand register r
//                        of X and the B operand register r of C times the weight; real and imaginary products go to
//                        accumulators of their own and are added at the end.  Lam^T (Delta Lam) and L Lam are
//                        products of the same kind with Lam's registers as B (and A) operands.
//   seq2o_reduce_kernel  out[sp][p][i] = sum over the frequency blocks, in index order
#include <algorithm>

#include "ffk_internal.h"

namespace ffk {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kSpectra = 2;              // spectra of one walk (accumulator sets); grid z carries the others
constexpr int kWaves = 4;                // one wavefront per SIMD: the whole register file of 512 each

// the row of the weights of selected operator i under spectrum sp: (n_spectra, W) or (n_spectra, n_idx, W)
__device__ __forceinline__ const cplx* weight_row(const cplx* scale, int s_ndim, int n_idx, int sp, int i, int W) {
    return scale + static_cast<size_t>(s_ndim == 1 ? sp : sp*n_idx + i)*W;
}

// ---- d = 2 -------------------------------------------------------------------------------------------------------
constexpr int kN2 = 4;

template <int A, bool STAGED>
__global__ __launch_bounds__(64*kWaves) void seq2o_walk2_kernel(
    const cplx* __restrict__ phases, const cplx* const* __restrict__ Rtab, const double* __restrict__ Lpulse,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, const int32_t* __restrict__ order,
    int P, int T, int W, int n_groups, const cplx* __restrict__ scale, int s_ndim, int n_spectra,
    const int32_t* __restrict__ idx, int n_idx, const double* __restrict__ gate_shifts, double* __restrict__ partial) {
    constexpr int N = kN2;
    constexpr int ROWS = A*N;
    constexpr int LN = N*N;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_waves = blockDim.x >> 6;
    const int w = blockIdx.x*64 + lane;
    const int wc = w < W ? w : W - 1;
    const int sp0 = blockIdx.z*kSpectra;
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
    // which selected operator an operator is (-1: none), and its weights at this lane's frequency (0 beyond W)
    int sel[A];
    double wt[A][kSpectra];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        sel[a] = -1;
        for (int i = n_idx - 1; i >= 0; --i)
            if (idx[i] == a) sel[a] = i;
#pragma unroll
        for (int s = 0; s < kSpectra; ++s)
            wt[a][s] = (sel[a] >= 0 && sp0 + s < n_spectra && w < W)
                           ? weight_row(scale, s_ndim, n_idx, sp0 + s, sel[a], W)[wc].re : 0.0;
    }
    const bool shifts_here = blockIdx.x == 0 && lane == 0;
    // (the small matrices are the same for every lane; read through a vector register they stay out of the scalar
    // registers, which the pointers and counters of the walk fill)
    int vzero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
    const int Q = n_groups*n_waves;
    for (int j = wave*n_groups + blockIdx.y; j < P; j += Q) {
        const int p = order[j];
        const int g_begin = offsets[p], g_end = offsets[p + 1];
        cplx C[ROWS];
        double Lam[LN], Z[A][kSpectra][LN];
#pragma unroll
        for (int e = 0; e < ROWS; ++e) C[e] = {0.0, 0.0};
#pragma unroll
        for (int e = 0; e < LN; ++e) Lam[e] = e % (N + 1) == 0 ? 1.0 : 0.0;
#pragma unroll
        for (int a = 0; a < A; ++a)
#pragma unroll
            for (int s = 0; s < kSpectra; ++s)
#pragma unroll
                for (int e = 0; e < LN; ++e) Z[a][s][e] = 0.0;
        for (int c0 = g_begin; c0 < g_end; c0 += 64) {
            const int c1 = min(g_end, c0 + 64);
            const int my_index = c0 + lane < c1 ? index[c0 + lane] : 0;
            for (int g = c0; g < c1; ++g) {
                const int k = __builtin_amdgcn_readlane(my_index, g - c0);
                const cplx* Rg = STAGED ? Rs + static_cast<size_t>(k)*ROWS*64 + lane : Rtab[k] + wc;
                const size_t rstride = STAGED ? 64 : static_cast<size_t>(W);
                const cplx ph = STAGED ? Ps[k*64 + lane] : phases[static_cast<size_t>(k)*W + wc];
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    if (sel[a] < 0) continue;
                    cplx X[N];
#pragma unroll
                    for (int jj = 0; jj < N; ++jj) X[jj] = {0.0, 0.0};
#pragma unroll
                    for (int kk = 0; kk < N; ++kk) {
                        const cplx v = Rg[(a*N + kk)*rstride];
#pragma unroll
                        for (int jj = 0; jj < N; ++jj) {
                            X[jj].re = fma(v.re, Lam[kk*N + jj], X[jj].re);
                            X[jj].im = fma(v.im, Lam[kk*N + jj], X[jj].im);
                        }
                    }
#pragma unroll
                    for (int s = 0; s < kSpectra; ++s) {
                        if (sp0 + s >= n_spectra) continue;
#pragma unroll
                        for (int kk = 0; kk < N; ++kk) {
                            const double xre = wt[a][s]*X[kk].re, xim = wt[a][s]*X[kk].im;
#pragma unroll
                            for (int l = 0; l < N; ++l)
                                Z[a][s][kk*N + l] += fma(xre, C[a*N + l].re, xim*C[a*N + l].im);
                        }
                    }
#pragma unroll
                    for (int jj = 0; jj < N; ++jj) {
                        const double sre = C[a*N + jj].re + X[jj].re, sim = C[a*N + jj].im + X[jj].im;
                        C[a*N + jj] = {fma(ph.re, sre, ph.im*sim), fma(ph.re, sim, -(ph.im*sre))};
                    }
                    if (shifts_here) {
                        // Lam^T Delta_gate Lam of this position, for every spectrum of the walk
#pragma unroll
                        for (int s = 0; s < kSpectra; ++s) {
                            if (sp0 + s >= n_spectra) continue;
                            const double* Dg = gate_shifts +
                                ((static_cast<size_t>(sp0 + s)*T + k)*n_idx + sel[a])*LN + vzero;
                            double M[LN];
#pragma unroll
                            for (int i = 0; i < N; ++i)
#pragma unroll
                                for (int l = 0; l < N; ++l) {
                                    double acc = 0.0;
#pragma unroll
                                    for (int m = 0; m < N; ++m) acc = fma(Dg[i*N + m], Lam[m*N + l], acc);
                                    M[i*N + l] = acc;
                                }
#pragma unroll
                            for (int kk = 0; kk < N; ++kk)
#pragma unroll
                                for (int l = 0; l < N; ++l) {
                                    double acc = 0.0;
#pragma unroll
                                    for (int m = 0; m < N; ++m) acc = fma(Lam[m*N + kk], M[m*N + l], acc);
                                    Z[a][s][kk*N + l] += acc;
                                }
                        }
                    }
                }
                // Lam <- L_k Lam
                const double* Lsrc = Lpulse + static_cast<size_t>(k)*LN + vzero;
                double Ln[LN];
#pragma unroll
                for (int i = 0; i < N; ++i)
#pragma unroll
                    for (int l = 0; l < N; ++l) {
                        double acc = 0.0;
#pragma unroll
                        for (int m = 0; m < N; ++m) acc = fma(Lsrc[i*N + m], Lam[m*N + l], acc);
                        Ln[i*N + l] = acc;
                    }
#pragma unroll
                for (int e = 0; e < LN; ++e) Lam[e] = Ln[e];
            }
        }
        double* tile0 = partial + (static_cast<size_t>(blockIdx.x)*P + p)*n_spectra*n_idx*LN;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            if (sel[a] < 0) continue;
#pragma unroll
            for (int s = 0; s < kSpectra; ++s) {
                if (sp0 + s >= n_spectra) continue;
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
                    for (int e = 0; e < LN; ++e) Z[a][s][e] += __shfl_xor(Z[a][s][e], m);
                if (lane == 0)
                    for (int i = 0; i < n_idx; ++i) {
                        if (idx[i] != a) continue;
                        double* o = tile0 + (static_cast<size_t>(sp0 + s)*n_idx + i)*LN;
#pragma unroll
                        for (int e = 0; e < LN; ++e) o[e] = Z[a][s][e];
                    }
            }
        }
    }
}

size_t staged2_lds_bytes(int T, int A) {
    return static_cast<size_t>(T)*(A*kN2 + 1)*64*sizeof(cplx);
}

// ---- d = 4 -------------------------------------------------------------------------------------------------------
constexpr int kN = 16;
constexpr int seq4_tiles(int A) { return A <= 2 ? 4 : 2; }             // (as sequences_d4.hip)

template <int A, bool STAGED>
__global__ __launch_bounds__(64*kWaves) void seq2o_walk4_kernel(
    const cplx* __restrict__ phases, const cplx* const* __restrict__ Rtab, const double* __restrict__ Lpulse,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, const int32_t* __restrict__ order,
    int P, int T, int W, int n_groups, const cplx* __restrict__ scale, int s_ndim, int n_spectra,
    const int32_t* __restrict__ idx, int n_idx, const double* __restrict__ gate_shifts, double* __restrict__ partial) {
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
    const int sp0 = blockIdx.z*kSpectra;
    // the weights of the block's frequencies first ([kSpectra][A][WT], 0 beyond W and for what is not selected), the
    // staged tables behind them
    double* Ws = reinterpret_cast<double*>(lds_raw);
    cplx* Rs = reinterpret_cast<cplx*>(lds_raw + kSpectra*A*WT*sizeof(double));           // [T][ROWS][WT]
    cplx* Ps = Rs + static_cast<size_t>(T)*ROWS*WT;                                       // [T][WT]
    int sel[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        sel[a] = -1;
        for (int i = n_idx - 1; i >= 0; --i)
            if (idx[i] == a) sel[a] = i;
    }
    for (int e = threadIdx.x; e < kSpectra*A*WT; e += blockDim.x) {
        const int x = e % WT, a = (e / WT) % A, s = e / (WT*A);
        int i = -1;
        for (int m = n_idx - 1; m >= 0; --m)
            if (idx[m] == a) i = m;
        Ws[e] = (i >= 0 && sp0 + s < n_spectra && w0 + x < W)
                    ? weight_row(scale, s_ndim, n_idx, sp0 + s, i, W)[w0 + x].re : 0.0;
    }
    if (STAGED) {
        const int x = lane % WT, wl = min(w0 + x, W - 1);
        for (int e = wave*(64/WT) + lane/WT; e < T*ROWS; e += n_waves*(64/WT)) {
            const int k = e / ROWS, r = e % ROWS;
            Rs[static_cast<size_t>(e)*WT + x] = Rtab[k][static_cast<size_t>(r)*W + wl];
        }
        for (int k = wave*(64/WT) + lane/WT; k < T; k += n_waves*(64/WT))
            Ps[k*WT + x] = phases[static_cast<size_t>(k)*W + wl];
    }
    __syncthreads();
    // columns of the table reads: as A operand the frequency is 16 t + c, in a D tile 16 t + q + 4 r
    size_t colA[TILES], colD[TILES][4];
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        colA[t] = STAGED ? size_t(16*t + c) : size_t(min(w0 + 16*t + c, W - 1));
#pragma unroll
        for (int r = 0; r < 4; ++r)
            colD[t][r] = STAGED ? size_t(16*t + q + 4*r) : size_t(min(w0 + 16*t + q + 4*r, W - 1));
    }
    const size_t rstride = STAGED ? WT : static_cast<size_t>(W);
    const bool shifts_here = blockIdx.x == 0;
    const f64x4 zero = {0.0, 0.0, 0.0, 0.0};
    const int Q = n_groups*n_waves;
    for (int j = wave*n_groups + blockIdx.y; j < P; j += Q) {
        const int p = order[j];
        const int g_begin = offsets[p], g_end = offsets[p + 1];
        f64x4 Cre[A][TILES], Cim[A][TILES], Zre[A][kSpectra], Zim[A][kSpectra], Zd[A][kSpectra], Lam;
#pragma unroll
        for (int a = 0; a < A; ++a) {
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                Cre[a][t] = zero;
                Cim[a][t] = zero;
            }
#pragma unroll
            for (int s = 0; s < kSpectra; ++s) {
                Zre[a][s] = zero;
                Zim[a][s] = zero;
                Zd[a][s] = zero;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) Lam[r] = q + 4*r == c ? 1.0 : 0.0;
        for (int c0 = g_begin; c0 < g_end; c0 += 64) {
            const int c1 = min(g_end, c0 + 64);
            const int my_index = c0 + lane < c1 ? index[c0 + lane] : 0;
            for (int g = c0; g < c1; ++g) {
                const int k = __builtin_amdgcn_readlane(my_index, g - c0);
                const cplx* Rg = STAGED ? Rs + static_cast<size_t>(k)*ROWS*WT : Rtab[k];
                const cplx* Pg = STAGED ? Ps + k*WT : phases + static_cast<size_t>(k)*W;
#pragma unroll
                for (int t = 0; t < TILES; ++t) {
                    cplx ph[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) ph[r] = Pg[colD[t][r]];
#pragma unroll
                    for (int a = 0; a < A; ++a) {
                        if (sel[a] < 0) continue;
                        // X = R Lam: row = frequency 16 t + q + 4 r, col = basis element c
                        f64x4 xre = zero, xim = zero;
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const cplx v = Rg[(a*N + q + 4*s)*rstride + colA[t]];
                            xre = __builtin_amdgcn_mfma_f64_16x16x4f64(v.re, Lam[s], xre, 0, 0, 0);
                            xim = __builtin_amdgcn_mfma_f64_16x16x4f64(v.im, Lam[s], xim, 0, 0, 0);
                        }
                        // Z[k, l] += sum_w X[w, k] (weight_w C[w, l])
#pragma unroll
                        for (int s = 0; s < kSpectra; ++s) {
                            if (sp0 + s >= n_spectra) continue;
                            const double* wrow = Ws + (s*A + a)*WT + 16*t + q;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const double wt = wrow[4*r];
                                Zre[a][s] = __builtin_amdgcn_mfma_f64_16x16x4f64(xre[r], wt*Cre[a][t][r], Zre[a][s],
                                                                                 0, 0, 0);
                                Zim[a][s] = __builtin_amdgcn_mfma_f64_16x16x4f64(xim[r], wt*Cim[a][t][r], Zim[a][s],
                                                                                 0, 0, 0);
                            }
                        }
                        // C <- conj(p) (C + X)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double sre = Cre[a][t][r] + xre[r], sim = Cim[a][t][r] + xim[r];
                            Cre[a][t][r] = fma(ph[r].re, sre, ph[r].im*sim);
                            Cim[a][t][r] = fma(ph[r].re, sim, -(ph[r].im*sre));
                        }
                    }
                }
                if (shifts_here) {
                    // Lam^T (Delta_gate Lam) of this position, for every selected operator and spectrum of the walk
#pragma unroll
                    for (int a = 0; a < A; ++a) {
                        if (sel[a] < 0) continue;
#pragma unroll
                        for (int s = 0; s < kSpectra; ++s) {
                            if (sp0 + s >= n_spectra) continue;
                            const double* Dg = gate_shifts +
                                ((static_cast<size_t>(sp0 + s)*T + k)*n_idx + sel[a])*N*N + c*N + q;
                            f64x4 M = zero;
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                M = __builtin_amdgcn_mfma_f64_16x16x4f64(Dg[4*r], Lam[r], M, 0, 0, 0);
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                Zd[a][s] = __builtin_amdgcn_mfma_f64_16x16x4f64(Lam[r], M[r], Zd[a][s], 0, 0, 0);
                        }
                    }
                }
                // Lam <- L_k Lam
                const double* Lsrc = Lpulse + static_cast<size_t>(k)*N*N + c*N + q;
                f64x4 Ln = zero;
#pragma unroll
                for (int r = 0; r < 4; ++r) Ln = __builtin_amdgcn_mfma_f64_16x16x4f64(Lsrc[4*r], Lam[r], Ln, 0, 0, 0);
                Lam = Ln;
            }
        }
        double* tile0 = partial + (static_cast<size_t>(blockIdx.x)*P + p)*n_spectra*n_idx*N*N;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            if (sel[a] < 0) continue;
#pragma unroll
            for (int s = 0; s < kSpectra; ++s) {
                if (sp0 + s >= n_spectra) continue;
                f64x4 acc = Zre[a][s] + Zim[a][s];
                if (shifts_here) acc += Zd[a][s];
                for (int i = 0; i < n_idx; ++i) {
                    if (idx[i] != a) continue;
                    double* o = tile0 + (static_cast<size_t>(sp0 + s)*n_idx + i)*N*N;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[(q + 4*r)*N + c] = acc[r];
                }
            }
        }
    }
}

size_t weights4_lds_bytes(int A) {
    return static_cast<size_t>(kSpectra)*A*16*seq4_tiles(A)*sizeof(double);
}
size_t staged4_lds_bytes(int T, int A) {
    return static_cast<size_t>(T)*(A*kN + 1)*16*seq4_tiles(A)*sizeof(cplx);
}

// out[sp][p][i] = sum over the frequency blocks, in index order, of partial[fb][p][sp][i]; row = n_idx*N*N doubles
__global__ __launch_bounds__(256) void seq2o_reduce_kernel(const double* __restrict__ partial, int blocks, int P,
                                                           int n_spectra, size_t row, double* __restrict__ out) {
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

int sequence_second_order_block_width(int d, int A) {
    return d == 2 ? 64 : 16*seq4_tiles(A);
}

int sequence_second_order_spectra_per_walk() {
    return kSpectra;
}

bool sequence_second_order_staged(int d, int T, int A) {
    if (d == 2) return staged2_lds_bytes(T, A) <= 150*1024;
    return staged4_lds_bytes(T, A) + weights4_lds_bytes(A) <= 150*1024;
}

hipError_t launch_sequence_second_order(int d, const cplx* phases, const cplx* const* Rtab, const double* Lpulse,
                                        const int32_t* offsets, const int32_t* index, const int32_t* order, int P,
                                        int T, int A, int W, const cplx* scale, int s_ndim, int n_spectra,
                                        const int32_t* idx, int n_idx, const double* gate_shifts, double* partial,
                                        double* out, hipStream_t stream) {
    if (A < 1 || A > 4 || P < 1 || T < 1 || W < 1 || n_spectra < 1 || n_idx < 1 || n_idx > A ||
        (s_ndim != 1 && s_ndim != 2) || (d != 2 && d != 4))
        return hipErrorInvalidValue;
    const bool staged = sequence_second_order_staged(d, T, A);
    const int width = sequence_second_order_block_width(d, A);
    const int blocks = (W + width - 1)/width;
    const int walks = (n_spectra + kSpectra - 1)/kSpectra;
    if (walks > 65535) return hipErrorInvalidValue;
    // as sequences4_groups: staged, one block per CU; else a few; never more groups than wavefronts' worth of sequences
    long groups = ((staged ? 256L : 1024L) + static_cast<long>(blocks)*walks - 1)/(static_cast<long>(blocks)*walks);
    groups = std::min(groups, (static_cast<long>(P) + kWaves - 1)/kWaves);
    groups = std::max(1L, std::min(groups, 65535L));
    const dim3 grid(blocks, static_cast<unsigned>(groups), walks);
    const int n_groups = static_cast<int>(groups);
    auto launch = [&](auto kern, size_t lds) -> hipError_t {
        if (lds > 48*1024) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     static_cast<int>(lds));
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, grid, dim3(64*kWaves), lds, stream, phases, Rtab, Lpulse, offsets, index, order, P, T,
                           W, n_groups, scale, s_ndim, n_spectra, idx, n_idx, gate_shifts, partial);
        return hipGetLastError();
    };
    hipError_t err = hipErrorInvalidValue;
#define FFK_SEQ2O(AA)                                                                                              \
    case AA:                                                                                                       \
        if (d == 2)                                                                                                \
            err = staged ? launch(seq2o_walk2_kernel<AA, true>, staged2_lds_bytes(T, AA))                          \
                         : launch(seq2o_walk2_kernel<AA, false>, 0);                                               \
        else                                                                                                       \
            err = staged ? launch(seq2o_walk4_kernel<AA, true>, staged4_lds_bytes(T, AA) + weights4_lds_bytes(AA)) \
                         : launch(seq2o_walk4_kernel<AA, false>, weights4_lds_bytes(AA));                          \
        break;
    switch (A) {
        FFK_SEQ2O(1) FFK_SEQ2O(2) FFK_SEQ2O(3) FFK_SEQ2O(4)
        default: break;
    }
#undef FFK_SEQ2O
    if (err != hipSuccess) return err;
    const size_t row = static_cast<size_t>(n_idx)*d*d*d*d;
    const size_t n = static_cast<size_t>(P)*n_spectra*row;
    if ((n + 255)/256 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(seq2o_reduce_kernel, dim3(static_cast<unsigned>((n + 255)/256)), dim3(256), 0, stream, partial,
                       blocks, P, n_spectra, row, out);
    return hipGetLastError();
}

}  // namespace ffk

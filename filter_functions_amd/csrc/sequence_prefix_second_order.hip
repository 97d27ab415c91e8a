// sequence_prefix_second_order.hip -- frequency shifts (second order) of every PREFIX of many gate sequences drawn from
// one table of distinct gates, optionally with a closing gate behind each prefix, in one forward walk of each sequence
// (ff.sequence_prefix_frequency_shifts; ffk_sequence_prefix_frequency_shifts).
//
// The forward walk of sequence_second_order.hip holds, after position m, the running sum
//     Z_m = sum_{g <= m} [ Lam_g^T Delta_gate(k_g) Lam_g + sum_w c_w S(w) Re( conj(Rs_g[k, w]) Cum_{g-1}[l, w] ) ]
// which is the frequency shift of the first m gates.  A closing gate c behind them adds one more summand of the same
// form, with the state the walk holds after the position (Lam_{m+1}, C_m = conj(phi_m) Cum_m; the common phase cancels):
//     X_c     = R_c Lam_{m+1}
//     Delta_m = Z_m + Lam_{m+1}^T Delta_gate(c) Lam_{m+1} + sum_w c_w S(w) (Re X_c[w, k] Re C_m[w, l] + Im X_c[w, k] Im C_m[w, l])
// A prefix quantity is therefore one epilogue per position on COPIES of the accumulators; the running accumulators go
// on untouched, and position g sees nothing behind it: the curve of s[:m] is the first m rows of the curve of s, bit
// for bit.
//
// A block forms the partial tiles of its frequencies for every position and seqpre2o_reduce_kernel adds the blocks in
// index order.  The gates' own shifts are frequency independent: frequency block 0 adds them.  No atomics, no waits
// between wavefronts or blocks, a block width that depends on d and A alone, fresh accumulators of the closing summand
// for every (position, operator, spectrum), and a number of spectra per walk that depends on d, A and whether closing
// gates are given alone (grid z carries the further ones): a position's result is the same bits whatever else is in
// the pass.
//
//   partial[block][position][spectrum][i][N][N]
//
//   seqpre2o_walk2_kernel   d = 2: lane = frequency; Lam, C and Z (4 x 4 per operator and spectrum) per lane, as
//                           seq2o_walk2_kernel; per position the 16 entries of Z (plus the closing summand) are summed
//                           over the wavefront by the halving butterfly of sequence_prefix.hip (wave_sums); lane 0 of
//                           block 0 carries the Lam^T Delta_gate Lam terms
//   seqpre2o_walk4_kernel   d = 4: v_mfma_f64_16x16x4_f64, the operand maps of seq2o_walk4_kernel.  Per position the
//                           lane forms (Z_re + Z_im) + Z_Delta from copies; with a closing gate X_c = R_c Lam (8 matrix
//                           instructions per operator, tile and spectrum), its Gram with weight C into fresh Y_re, Y_im (8
//                           more) and, in block 0, Y_Delta = Lam^T (Delta_gate(c) Lam); the stored tile is
//                           ((Z_re + Z_im) + Z_Delta) + ((Y_re + Y_im) + Y_Delta)
//   seqpre2o_reduce_kernel  out[sp][position][i] = sum over the frequency blocks, in index order
#include <algorithm>
#include <type_traits>

#include "ffk_internal.h"

namespace ffk {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kWaves = 4;                // one wavefront per SIMD: the whole register file of 512 each

// spectra of one walk (accumulator sets); grid z carries the others.  A function of (d, A, closing) alone.
constexpr int spectra_per_walk(int d, int A, bool closing) {
    return (A >= 4 || (d == 4 && closing && A >= 3)) ? 1 : 2;
}

// the row of the weights of selected operator i under spectrum sp: (n_spectra, W) or (n_spectra, n_idx, W)
__device__ __forceinline__ const cplx* weight_row(const cplx* scale, int s_ndim, int n_idx, int sp, int i, int W) {
    return scale + static_cast<size_t>(s_ndim == 1 ? sp : sp*n_idx + i)*W;
}

// The sums over the wavefront of VP values per lane (VP a power of two, at most 64): the halving butterfly of
// sequence_prefix.hip.  Returns the sum of value number lane >> (6 - log2 VP), the same in the 64/VP lanes that share
// it.  The order of the additions depends on the lane numbers alone.
template <int VP, bool OPAQUE>
__device__ __forceinline__ double wave_sums(double (&v)[VP], int lane) {
    int m = 32;
#pragma unroll
    for (int H = VP/2; H >= 1; H >>= 1, m >>= 1) {
        const bool hi = (lane & m) != 0;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            // (OPAQUE: values the compiler cannot trace back to an array -- it would else turn the selects on plain
            // copies of the accumulators into one choice among sixteen registers, whose lane masks spill the scalar
            // registers)
            double lower = v[j], upper = v[j + H];
            if (OPAQUE && H == VP/2) asm("" : "+v"(lower), "+v"(upper));
            const double send = hi ? lower : upper, keep = hi ? upper : lower;
            v[j] = keep + __shfl_xor(send, m);
        }
    }
#pragma unroll
    for (; m >= 1; m >>= 1) v[0] += __shfl_xor(v[0], m);
    return v[0];
}

// ---- d = 2 -------------------------------------------------------------------------------------------------------
constexpr int kN2 = 4;

// acc += Lam^T (D Lam), 4 x 4 (D read through a vector register: see the walk)
__device__ __forceinline__ void add_rotated2(const double* D, const double (&Lam)[16], double (&acc)[16]) {
    constexpr int N = kN2;
    double M[N*N];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int l = 0; l < N; ++l) {
            double a = 0.0;
#pragma unroll
            for (int m = 0; m < N; ++m) a = fma(D[i*N + m], Lam[m*N + l], a);
            M[i*N + l] = a;
        }
#pragma unroll
    for (int kk = 0; kk < N; ++kk)
#pragma unroll
        for (int l = 0; l < N; ++l) {
            double a = 0.0;
#pragma unroll
            for (int m = 0; m < N; ++m) a = fma(Lam[m*N + kk], M[m*N + l], a);
            acc[kk*N + l] += a;
        }
}

template <int A, bool STAGED, bool CLOSING>
__global__ __launch_bounds__(64*kWaves) void seqpre2o_walk2_kernel(
    const cplx* __restrict__ phases, const cplx* const* __restrict__ Rtab, const double* __restrict__ Lpulse,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, const int32_t* __restrict__ closing,
    const int32_t* __restrict__ order, int P, int n_index, int T, int W, int n_groups,
    const cplx* __restrict__ scale, int s_ndim, int n_spectra, const int32_t* __restrict__ idx, int n_idx,
    const double* __restrict__ gate_shifts, double* __restrict__ partial) {
    constexpr int N = kN2;
    constexpr int ROWS = A*N;
    constexpr int LN = N*N;
    constexpr int S = spectra_per_walk(2, A, CLOSING);
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_waves = blockDim.x >> 6;
    const int w = blockIdx.x*64 + lane;
    const int wc = w < W ? w : W - 1;
    const int sp0 = blockIdx.z*S;
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
    double wt[A][S];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        sel[a] = -1;
        for (int i = n_idx - 1; i >= 0; --i)
            if (idx[i] == a) sel[a] = i;
#pragma unroll
        for (int s = 0; s < S; ++s)
            wt[a][s] = (sel[a] >= 0 && sp0 + s < n_spectra && w < W)
                           ? weight_row(scale, s_ndim, n_idx, sp0 + s, sel[a], W)[wc].re : 0.0;
    }
    const bool shifts_here = blockIdx.x == 0 && lane == 0;
    const bool stores = (lane & 3) == 0;                              // value lane >> 2 of the 16 ends here
    const size_t per_position = static_cast<size_t>(n_spectra)*n_idx*LN;
    // (the small matrices are the same for every lane; read through a vector register they stay out of the scalar
    // registers, which the pointers and counters of the walk fill)
    int vzero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
    const int Q = n_groups*n_waves;
    for (int j = wave*n_groups + blockIdx.y; j < P; j += Q) {
        const int p = order[j];
        const int g_begin = offsets[p], g_end = offsets[p + 1];
        cplx C[ROWS];
        double Lam[LN], Z[A][S][LN];
#pragma unroll
        for (int e = 0; e < ROWS; ++e) C[e] = {0.0, 0.0};
#pragma unroll
        for (int e = 0; e < LN; ++e) Lam[e] = e % (N + 1) == 0 ? 1.0 : 0.0;
#pragma unroll
        for (int a = 0; a < A; ++a)
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int e = 0; e < LN; ++e) Z[a][s][e] = 0.0;
        for (int c0 = g_begin; c0 < g_end; c0 += 64) {
            const int c1 = min(g_end, c0 + 64);
            const int my_index = c0 + lane < c1 ? index[c0 + lane] : 0;
            const int my_closing = (CLOSING && c0 + lane < c1) ? closing[c0 + lane] : 0;
            for (int g = c0; g < c1; ++g) {
                const int k = __builtin_amdgcn_readlane(my_index, g - c0);
                const int kc = __builtin_amdgcn_readlane(my_closing, g - c0);
                // (read from L2, the gates' rows are addressed through vector registers as well)
                const int kv = STAGED ? k : k + vzero, kcv = STAGED ? kc : kc + vzero;
                const cplx* Rg = STAGED ? Rs + static_cast<size_t>(k)*ROWS*64 + lane : Rtab[kv] + wc;
                const cplx* Rc = STAGED ? Rs + static_cast<size_t>(kc)*ROWS*64 + lane : Rtab[kcv] + wc;
                const size_t rstride = STAGED ? 64 : static_cast<size_t>(W + vzero);
                const cplx ph = STAGED ? Ps[k*64 + lane] : phases[static_cast<size_t>(kv)*W + wc];
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
                    for (int s = 0; s < S; ++s) {
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
                        for (int s = 0; s < S; ++s) {
                            if (sp0 + s >= n_spectra) continue;
                            add_rotated2(gate_shifts + ((static_cast<size_t>(sp0 + s)*T + k)*n_idx + (sel[a] + vzero))*LN,
                                         Lam, Z[a][s]);
                        }
                    }
                }
                // Lam <- L_k Lam
                {
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
                // the epilogue of this position: copies of Z, plus the closing gate's summand
                double* pos0 = partial + (static_cast<size_t>(blockIdx.x)*n_index + g)*per_position;
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    if (sel[a] < 0) continue;
                    cplx Xc[N];
                    if (CLOSING) {
#pragma unroll
                        for (int jj = 0; jj < N; ++jj) Xc[jj] = {0.0, 0.0};
#pragma unroll
                        for (int kk = 0; kk < N; ++kk) {
                            const cplx v = Rc[(a*N + kk)*rstride];
#pragma unroll
                            for (int jj = 0; jj < N; ++jj) {
                                Xc[jj].re = fma(v.re, Lam[kk*N + jj], Xc[jj].re);
                                Xc[jj].im = fma(v.im, Lam[kk*N + jj], Xc[jj].im);
                            }
                        }
                    }
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        if (sp0 + s >= n_spectra) continue;
                        double v[LN];
                        if (CLOSING) {
                            // the closing gate's summand first, fresh, then the copy of Z in front of it
#pragma unroll
                            for (int kk = 0; kk < N; ++kk) {
                                const double xre = wt[a][s]*Xc[kk].re, xim = wt[a][s]*Xc[kk].im;
#pragma unroll
                                for (int l = 0; l < N; ++l)
                                    v[kk*N + l] = fma(xre, C[a*N + l].re, xim*C[a*N + l].im);
                            }
                            if (shifts_here)
                                add_rotated2(gate_shifts +
                                                 ((static_cast<size_t>(sp0 + s)*T + kc)*n_idx + (sel[a] + vzero))*LN,
                                             Lam, v);
#pragma unroll
                            for (int e = 0; e < LN; ++e) v[e] = Z[a][s][e] + v[e];
                        } else {
#pragma unroll
                            for (int e = 0; e < LN; ++e) v[e] = Z[a][s][e];
                        }
                        const double sum = wave_sums<LN, !CLOSING>(v, lane);
                        if (stores)
                            pos0[(static_cast<size_t>(sp0 + s)*n_idx + (sel[a] + vzero))*LN + (lane >> 2)] = sum;
                    }
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

template <int A, bool STAGED, bool CLOSING>
__global__ __launch_bounds__(64*kWaves) void seqpre2o_walk4_kernel(
    const cplx* __restrict__ phases, const cplx* const* __restrict__ Rtab, const double* __restrict__ Lpulse,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, const int32_t* __restrict__ closing,
    const int32_t* __restrict__ order, int P, int n_index, int T, int W, int n_groups,
    const cplx* __restrict__ scale, int s_ndim, int n_spectra, const int32_t* __restrict__ idx, int n_idx,
    const double* __restrict__ gate_shifts, double* __restrict__ partial) {
    constexpr int N = kN;
    constexpr int ROWS = A*N;
    constexpr int TILES = seq4_tiles(A);
    constexpr int WT = 16*TILES;                                      // frequencies of a block
    constexpr int S = spectra_per_walk(4, A, CLOSING);
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_waves = blockDim.x >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int w0 = blockIdx.x*WT;
    const int sp0 = blockIdx.z*S;
    // the weights of the block's frequencies first ([S][A][WT], 0 beyond W and for what is not selected), the staged
    // tables behind them
    double* Ws = reinterpret_cast<double*>(lds_raw);
    cplx* Rs = reinterpret_cast<cplx*>(lds_raw + S*A*WT*sizeof(double));                  // [T][ROWS][WT]
    cplx* Ps = Rs + static_cast<size_t>(T)*ROWS*WT;                                       // [T][WT]
    int sel[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        sel[a] = -1;
        for (int i = n_idx - 1; i >= 0; --i)
            if (idx[i] == a) sel[a] = i;
    }
    for (int e = threadIdx.x; e < S*A*WT; e += blockDim.x) {
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
    // (32-bit: read from L2 they are live through the whole walk)
    int colA[TILES], colD[TILES][4];
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        colA[t] = STAGED ? 16*t + c : min(w0 + 16*t + c, W - 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) colD[t][r] = STAGED ? 16*t + q + 4*r : min(w0 + 16*t + q + 4*r, W - 1);
    }
    const size_t rstride = STAGED ? WT : static_cast<size_t>(W);
    const bool shifts_here = blockIdx.x == 0;
    const size_t per_position = static_cast<size_t>(n_spectra)*n_idx*N*N;
    // (the tiles' places in a position's partial results are formed in vector registers: the scalar ones are full of
    // the pointers and counters of the walk)
    int vzero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
    const f64x4 zero = {0.0, 0.0, 0.0, 0.0};
    const int Q = n_groups*n_waves;
    for (int j = wave*n_groups + blockIdx.y; j < P; j += Q) {
        const int p = order[j];
        const int g_begin = offsets[p], g_end = offsets[p + 1];
        f64x4 Cre[A][TILES], Cim[A][TILES], Zre[A][S], Zim[A][S], Zd[A][S], Lam;
#pragma unroll
        for (int a = 0; a < A; ++a) {
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                Cre[a][t] = zero;
                Cim[a][t] = zero;
            }
#pragma unroll
            for (int s = 0; s < S; ++s) {
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
            const int my_closing = (CLOSING && c0 + lane < c1) ? closing[c0 + lane] : 0;
            for (int g = c0; g < c1; ++g) {
                const int k = __builtin_amdgcn_readlane(my_index, g - c0);
                const int kc = __builtin_amdgcn_readlane(my_closing, g - c0);
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
                        for (int s = 0; s < S; ++s) {
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
                        for (int s = 0; s < S; ++s) {
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
                {
                    const double* Lsrc = Lpulse + static_cast<size_t>(k)*N*N + c*N + q;
                    f64x4 Ln = zero;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        Ln = __builtin_amdgcn_mfma_f64_16x16x4f64(Lsrc[4*r], Lam[r], Ln, 0, 0, 0);
                    Lam = Ln;
                }
                // the epilogue of this position: copies of the accumulators, plus the closing gate's summand
                double* pos0 = partial + (static_cast<size_t>(blockIdx.x)*n_index + g)*per_position;
                const cplx* Rc = STAGED ? Rs + static_cast<size_t>(kc)*ROWS*WT : Rtab[kc];
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    if (sel[a] < 0) continue;
                    // (one spectrum at a time: X_c is formed again for the second one, eight matrix instructions per
                    // tile, which keeps the epilogue within the registers the walk leaves; the bits are the same)
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        if (sp0 + s >= n_spectra) continue;
                        f64x4 acc = Zre[a][s] + Zim[a][s];
                        if (shifts_here) acc += Zd[a][s];
                        if (CLOSING) {
                            f64x4 Yre = zero, Yim = zero;
#pragma unroll
                            for (int t = 0; t < TILES; ++t) {
                                f64x4 xre = zero, xim = zero;
#pragma unroll
                                for (int m = 0; m < 4; ++m) {
                                    const cplx v = Rc[(a*N + q + 4*m)*rstride + colA[t]];
                                    xre = __builtin_amdgcn_mfma_f64_16x16x4f64(v.re, Lam[m], xre, 0, 0, 0);
                                    xim = __builtin_amdgcn_mfma_f64_16x16x4f64(v.im, Lam[m], xim, 0, 0, 0);
                                }
                                const double* wrow = Ws + (s*A + a)*WT + 16*t + q;
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const double wt = wrow[4*r];
                                    Yre = __builtin_amdgcn_mfma_f64_16x16x4f64(xre[r], wt*Cre[a][t][r], Yre, 0, 0, 0);
                                    Yim = __builtin_amdgcn_mfma_f64_16x16x4f64(xim[r], wt*Cim[a][t][r], Yim, 0, 0, 0);
                                }
                            }
                            f64x4 y = Yre + Yim;
                            if (shifts_here) {
                                const double* Dg = gate_shifts +
                                    ((static_cast<size_t>(sp0 + s)*T + kc)*n_idx + sel[a])*N*N + c*N + q;
                                f64x4 M = zero, Yd = zero;
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    M = __builtin_amdgcn_mfma_f64_16x16x4f64(Dg[4*r], Lam[r], M, 0, 0, 0);
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    Yd = __builtin_amdgcn_mfma_f64_16x16x4f64(Lam[r], M[r], Yd, 0, 0, 0);
                                y += Yd;
                            }
                            acc += y;
                        }
                        double* o = pos0 + (static_cast<size_t>(sp0 + s)*n_idx + (sel[a] + vzero))*N*N;
#pragma unroll
                        for (int r = 0; r < 4; ++r) o[(q + 4*r)*N + c] = acc[r];
                    }
                }
            }
        }
    }
}

size_t weights4_lds_bytes(int A, bool closing) {
    return static_cast<size_t>(spectra_per_walk(4, A, closing))*A*16*seq4_tiles(A)*sizeof(double);
}
size_t staged4_lds_bytes(int T, int A) {
    return static_cast<size_t>(T)*(A*kN + 1)*16*seq4_tiles(A)*sizeof(cplx);
}

// out (n_spectra, n_index, n_idx, N, N): the frequency blocks of partial (blocks, n_index, n_spectra, n_idx, N, N) added
// in index order; tile = N*N doubles
__global__ __launch_bounds__(256) void seqpre2o_reduce_kernel(const double* __restrict__ partial, int blocks,
                                                              size_t n_index, int n_spectra, int n_idx, size_t tile,
                                                              double* __restrict__ out) {
    const size_t members = n_index*n_spectra*n_idx;
    const size_t o = static_cast<size_t>(blockIdx.x)*256 + threadIdx.x;
    if (o >= members*tile) return;
    const size_t e = o % tile, m = o / tile;
    const size_t i = m % n_idx, pos = (m / n_idx) % n_index, sp = m / (n_idx*n_index);
    const size_t src = ((pos*n_spectra + sp)*n_idx + i)*tile + e;
    const size_t stride = members*tile;
    double acc = partial[src];
    for (int b = 1; b < blocks; ++b) acc += partial[static_cast<size_t>(b)*stride + src];
    out[o] = acc;
}

}  // namespace

int sequence_prefix_second_order_block_width(int d, int A) {
    return d == 2 ? 64 : 16*seq4_tiles(A);
}

int sequence_prefix_second_order_spectra_per_walk(int d, int A, bool closing) {
    return spectra_per_walk(d, A, closing);
}

bool sequence_prefix_second_order_staged(int d, int T, int A, bool closing) {
    if (d == 2) return staged2_lds_bytes(T, A) <= 150*1024;
    return staged4_lds_bytes(T, A) + weights4_lds_bytes(A, closing) <= 150*1024;
}

hipError_t launch_sequence_prefix_second_order(int d, const cplx* phases, const cplx* const* Rtab, const double* Lpulse,
                                               const int32_t* offsets, const int32_t* index, const int32_t* closing,
                                               const int32_t* order, int P, size_t n_index, int T, int A, int W,
                                               const cplx* scale, int s_ndim, int n_spectra, const int32_t* idx,
                                               int n_idx, const double* gate_shifts, double* partial, double* out,
                                               hipStream_t stream) {
    if (A < 1 || A > 4 || P < 1 || T < 1 || W < 1 || n_spectra < 1 || n_idx < 1 || n_idx > A ||
        (s_ndim != 1 && s_ndim != 2) || (d != 2 && d != 4) || n_index < size_t(P) || n_index > 0x7fffffffull)
        return hipErrorInvalidValue;
    const bool has_closing = closing != nullptr;
    const bool staged = sequence_prefix_second_order_staged(d, T, A, has_closing);
    const int width = sequence_prefix_second_order_block_width(d, A);
    const int blocks = (W + width - 1)/width;
    const int per_walk = spectra_per_walk(d, A, has_closing);
    const int walks = (n_spectra + per_walk - 1)/per_walk;
    if (walks > 65535) return hipErrorInvalidValue;
    // as launch_sequence_prefix: staged, one block per CU; else a few; never more groups than wavefronts' worth of
    // sequences
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
        hipLaunchKernelGGL(kern, grid, dim3(64*kWaves), lds, stream, phases, Rtab, Lpulse, offsets, index, closing,
                           order, P, static_cast<int>(n_index), T, W, n_groups, scale, s_ndim, n_spectra, idx, n_idx,
                           gate_shifts, partial);
        return hipGetLastError();
    };
    auto walk = [&](auto AA, auto CL) -> hipError_t {
        constexpr int a = decltype(AA)::value;
        constexpr bool cl = decltype(CL)::value;
        if (d == 2)
            return staged ? launch(seqpre2o_walk2_kernel<a, true, cl>, staged2_lds_bytes(T, a))
                          : launch(seqpre2o_walk2_kernel<a, false, cl>, 0);
        return staged ? launch(seqpre2o_walk4_kernel<a, true, cl>, staged4_lds_bytes(T, a) + weights4_lds_bytes(a, cl))
                      : launch(seqpre2o_walk4_kernel<a, false, cl>, weights4_lds_bytes(a, cl));
    };
    hipError_t err = hipErrorInvalidValue;
#define FFK_SEQPRE2O(AA)                                                                                  \
    case AA:                                                                                              \
        err = has_closing ? walk(std::integral_constant<int, AA>{}, std::true_type{})                     \
                          : walk(std::integral_constant<int, AA>{}, std::false_type{});                   \
        break;
    switch (A) {
        FFK_SEQPRE2O(1) FFK_SEQPRE2O(2) FFK_SEQPRE2O(3) FFK_SEQPRE2O(4)
        default: break;
    }
#undef FFK_SEQPRE2O
    if (err != hipSuccess) return err;
    const size_t tile = static_cast<size_t>(d)*d*d*d;
    const size_t n = n_index*n_spectra*n_idx*tile;
    if ((n + 255)/256 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(seqpre2o_reduce_kernel, dim3(static_cast<unsigned>((n + 255)/256)), dim3(256), 0, stream,
                       partial, blocks, n_index, n_spectra, n_idx, tile, out);
    return hipGetLastError();
}

}  // namespace ffk

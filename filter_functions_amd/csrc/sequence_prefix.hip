// sequence_prefix.hip -- infidelities and decay amplitudes of every PREFIX of many gate sequences drawn from one table
// of distinct gates, optionally with a closing gate behind each prefix, in one forward walk of each sequence
// (ff.sequence_prefix_infidelities, ff.sequence_prefix_decay_amplitudes; ffk_sequence_prefix_processes).
//
// The concatenation rule is a sum over the positions, R = sum_g phi_{g-1} R_{k_g} Lam_g, so the control matrix of the
// prefix of m gates is the partial sum Cum_m.  The forward walk of sequence_second_order.hip carries exactly that:
//     X_g       = R_{k_g} Lam_g
//     C_g       = conj(p_{k_g}) (C_{g-1} + X_g)       (= conj(phi_g) Cum_g)
//     Lam_{g+1} = L_{k_g} Lam_g
// and with a closing gate c_g behind the prefix the control matrix is Cum_g + phi_g R_{c_g} Lam_{g+1}, i.e.
//     E_g       = C_g + R_{c_g} Lam_{g+1}             (C_g itself is not changed)
// up to the common phase phi_g, which cancels in
//     Gamma_g[k, l] = sum_w c_w S(w) (Re E_g[k, w] Re E_g[l, w] + Im E_g[k, w] Im E_g[l, w]).
// A prefix quantity is therefore one epilogue per position.  Position g sees nothing behind it: the curve of s[:m] is
// the first m rows of the curve of s, bit for bit.
//
// A block forms the partial sums of its frequencies for every position and seqpre_reduce_kernel adds the blocks in
// index order.  No atomics, no waits between wavefronts or blocks, a block width that depends on d and A alone, fresh
// accumulators for every (position, operator, spectrum), at most kSpectra spectra per walk (grid z carries the
// further ones): a position's result is the same bits whatever else is in the pass.
//
//   mode 0, 1   partial[block][position][spectrum][i][N]      sum_w c_w S(w) |E[k, w]|^2   (the diagonal of Gamma)
//   mode 2      partial[block][position][spectrum][i][N][N]   Gamma; only k <= l is read back
//
//   seqpre_walk2_kernel   d = 2: lane = frequency; Lam and C per lane.  The lane-local products of a position (ten
//                         k <= l, or four squares) are summed over the wavefront by a butterfly that halves the values
//                         a lane carries at every step (wave_sums): about one shuffle per value, a fixed order
//   seqpre_walk4_kernel   d = 4: v_mfma_f64_16x16x4_f64, the operand maps of seq2o_walk4_kernel.  E is C + Y with the
//                         eight matrix instructions of Y accumulating onto C's registers; mode 2 is the Gram matrix of
//                         E over the block's frequencies (real and imaginary chains, added at the end), modes 0 and 1
//                         the lane's own 4 TILES frequencies in a fixed order, then the four row groups by two shuffles
//   seqpre_reduce_kernel  the frequency blocks in index order; mode 2 reads (min(k, l), max(k, l)): symmetric bit for
//                         bit; mode 0 adds the N diagonal sums in index order and divides by d
#include <algorithm>

#include "ffk_internal.h"

namespace ffk {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kSpectra = 2;              // spectra of one walk; grid z carries the others
constexpr int kWaves = 4;                // one wavefront per SIMD

// the row of the weights of selected operator i under spectrum sp: (n_spectra, W) or (n_spectra, n_idx, W)
__device__ __forceinline__ const cplx* weight_row(const cplx* scale, int s_ndim, int n_idx, int sp, int i, int W) {
    return scale + static_cast<size_t>(s_ndim == 1 ? sp : sp*n_idx + i)*W;
}

// The sums over the wavefront of VP values per lane (VP a power of two, at most 64).  At every step a lane keeps one
// half of its values and hands the other half to its partner, so the values a lane carries halve; once one is left
// the remaining steps are a plain butterfly.  Returns the sum of value number lane >> (6 - log2 VP), the same in the
// 64/VP lanes that share it.  The order of the additions depends on the lane numbers alone.
template <int VP>
__device__ __forceinline__ double wave_sums(double (&v)[VP], int lane) {
    int m = 32;
#pragma unroll
    for (int H = VP/2; H >= 1; H >>= 1, m >>= 1) {
        const bool hi = (lane & m) != 0;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const double send = hi ? v[j] : v[j + H], keep = hi ? v[j + H] : v[j];
            v[j] = keep + __shfl_xor(send, m);
        }
    }
#pragma unroll
    for (; m >= 1; m >>= 1) v[0] += __shfl_xor(v[0], m);
    return v[0];
}

// ---- d = 2 -------------------------------------------------------------------------------------------------------
constexpr int kN2 = 4;

template <int A, bool STAGED>
__global__ __launch_bounds__(64*kWaves) void seqpre_walk2_kernel(
    const cplx* __restrict__ phases, const cplx* const* __restrict__ Rtab, const double* __restrict__ Lpulse,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, const int32_t* __restrict__ closing,
    const int32_t* __restrict__ order, int P, int n_index, int T, int W, int n_groups,
    const cplx* __restrict__ scale, int s_ndim, int n_spectra, const int32_t* __restrict__ idx, int n_idx, int mode,
    double* __restrict__ partial) {
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
    // where this lane's value of a reduced set goes: value e = lane >> 2 of the ten products k <= l (mode 2), lane >> 4
    // of the four squares
    const int e10 = lane >> 2;
    const int tk = (e10 >= 4) + (e10 >= 7) + (e10 >= 9);
    const int tl = e10 - (tk == 0 ? 0 : tk == 1 ? 3 : tk == 2 ? 5 : 6);
    const bool stores2 = (lane & 3) == 0 && e10 < 10, stores1 = (lane & 15) == 0;
    const size_t tile = mode == 2 ? LN : N;
    const size_t per_position = static_cast<size_t>(n_spectra)*n_idx*tile;
    // (the small matrices are the same for every lane; read through a vector register they stay out of the scalar
    // registers, which the pointers and counters of the walk fill)
    int vzero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
    const int Q = n_groups*n_waves;
    for (int j = wave*n_groups + blockIdx.y; j < P; j += Q) {
        const int p = order[j];
        const int g_begin = offsets[p], g_end = offsets[p + 1];
        cplx C[ROWS];
        double Lam[LN];
#pragma unroll
        for (int e = 0; e < ROWS; ++e) C[e] = {0.0, 0.0};
#pragma unroll
        for (int e = 0; e < LN; ++e) Lam[e] = e % (N + 1) == 0 ? 1.0 : 0.0;
        for (int c0 = g_begin; c0 < g_end; c0 += 64) {
            const int c1 = min(g_end, c0 + 64);
            const int my_index = c0 + lane < c1 ? index[c0 + lane] : 0;
            const int my_closing = (closing != nullptr && c0 + lane < c1) ? closing[c0 + lane] : 0;
            for (int g = c0; g < c1; ++g) {
                const int k = __builtin_amdgcn_readlane(my_index, g - c0);
                const int kc = __builtin_amdgcn_readlane(my_closing, g - c0);
                // (read from L2, the gates' rows are addressed through vector registers as well)
                const int kv = STAGED ? k : k + vzero, kcv = STAGED ? kc : kc + vzero;
                const cplx* Rg = STAGED ? Rs + static_cast<size_t>(k)*ROWS*64 + lane : Rtab[kv] + wc;
                const cplx* Rc = STAGED ? Rs + static_cast<size_t>(kc)*ROWS*64 + lane : Rtab[kcv] + wc;
                const size_t rstride = STAGED ? 64 : static_cast<size_t>(W + vzero);
                const cplx ph = STAGED ? Ps[k*64 + lane] : phases[static_cast<size_t>(kv)*W + wc];
                // C <- conj(p) (C + R_k Lam)
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
                    for (int jj = 0; jj < N; ++jj) {
                        const double sre = C[a*N + jj].re + X[jj].re, sim = C[a*N + jj].im + X[jj].im;
                        C[a*N + jj] = {fma(ph.re, sre, ph.im*sim), fma(ph.re, sim, -(ph.im*sre))};
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
                // the epilogue of this position
                double* pos0 = partial + (static_cast<size_t>(blockIdx.x)*n_index + g)*per_position;
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    if (sel[a] < 0) continue;
                    cplx E[N];
#pragma unroll
                    for (int jj = 0; jj < N; ++jj) E[jj] = C[a*N + jj];
                    if (closing != nullptr) {
#pragma unroll
                        for (int kk = 0; kk < N; ++kk) {
                            const cplx v = Rc[(a*N + kk)*rstride];
#pragma unroll
                            for (int jj = 0; jj < N; ++jj) {
                                E[jj].re = fma(v.re, Lam[kk*N + jj], E[jj].re);
                                E[jj].im = fma(v.im, Lam[kk*N + jj], E[jj].im);
                            }
                        }
                    }
#pragma unroll
                    for (int s = 0; s < kSpectra; ++s) {
                        if (sp0 + s >= n_spectra) continue;
                        double* o = pos0 + (static_cast<size_t>(sp0 + s)*n_idx + (sel[a] + vzero))*tile;
                        if (mode == 2) {
                            double v[16];
                            int e = 0;
#pragma unroll
                            for (int kk = 0; kk < N; ++kk) {
                                const double bre = wt[a][s]*E[kk].re, bim = wt[a][s]*E[kk].im;
#pragma unroll
                                for (int l = kk; l < N; ++l, ++e) v[e] = fma(E[l].re, bre, E[l].im*bim);
                            }
#pragma unroll
                            for (; e < 16; ++e) v[e] = 0.0;
                            const double sum = wave_sums<16>(v, lane);
                            if (stores2) o[tk*N + tl] = sum;
                        } else {
                            double v[N];
#pragma unroll
                            for (int kk = 0; kk < N; ++kk)
                                v[kk] = wt[a][s]*fma(E[kk].re, E[kk].re, E[kk].im*E[kk].im);
                            const double sum = wave_sums<N>(v, lane);
                            if (stores1) o[lane >> 4] = sum;
                        }
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

template <int A, bool STAGED>
__global__ __launch_bounds__(64*kWaves) void seqpre_walk4_kernel(
    const cplx* __restrict__ phases, const cplx* const* __restrict__ Rtab, const double* __restrict__ Lpulse,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ index, const int32_t* __restrict__ closing,
    const int32_t* __restrict__ order, int P, int n_index, int T, int W, int n_groups,
    const cplx* __restrict__ scale, int s_ndim, int n_spectra, const int32_t* __restrict__ idx, int n_idx, int mode,
    double* __restrict__ partial) {
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
    const size_t tile = mode == 2 ? N*N : N;
    const size_t per_position = static_cast<size_t>(n_spectra)*n_idx*tile;
    const f64x4 zero = {0.0, 0.0, 0.0, 0.0};
    const int Q = n_groups*n_waves;
    for (int j = wave*n_groups + blockIdx.y; j < P; j += Q) {
        const int p = order[j];
        const int g_begin = offsets[p], g_end = offsets[p + 1];
        f64x4 Cre[A][TILES], Cim[A][TILES], Lam;
#pragma unroll
        for (int a = 0; a < A; ++a)
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                Cre[a][t] = zero;
                Cim[a][t] = zero;
            }
#pragma unroll
        for (int r = 0; r < 4; ++r) Lam[r] = q + 4*r == c ? 1.0 : 0.0;
        for (int c0 = g_begin; c0 < g_end; c0 += 64) {
            const int c1 = min(g_end, c0 + 64);
            const int my_index = c0 + lane < c1 ? index[c0 + lane] : 0;
            const int my_closing = (closing != nullptr && c0 + lane < c1) ? closing[c0 + lane] : 0;
            for (int g = c0; g < c1; ++g) {
                const int k = __builtin_amdgcn_readlane(my_index, g - c0);
                const int kc = __builtin_amdgcn_readlane(my_closing, g - c0);
                const cplx* Rg = STAGED ? Rs + static_cast<size_t>(k)*ROWS*WT : Rtab[k];
                const cplx* Rc = STAGED ? Rs + static_cast<size_t>(kc)*ROWS*WT : Rtab[kc];
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
                        // C <- conj(p) (C + X)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double sre = Cre[a][t][r] + xre[r], sim = Cim[a][t][r] + xim[r];
                            Cre[a][t][r] = fma(ph[r].re, sre, ph[r].im*sim);
                            Cim[a][t][r] = fma(ph[r].re, sim, -(ph[r].im*sre));
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
                // the epilogue of this position: E = C (+ R_c Lam), then its weighted Gram matrix or squares
                double* pos0 = partial + (static_cast<size_t>(blockIdx.x)*n_index + g)*per_position;
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    if (sel[a] < 0) continue;
                    f64x4 Gre[kSpectra], Gim[kSpectra];
                    double dsum[kSpectra];
#pragma unroll
                    for (int s = 0; s < kSpectra; ++s) {
                        Gre[s] = zero;
                        Gim[s] = zero;
                        dsum[s] = 0.0;
                    }
#pragma unroll
                    for (int t = 0; t < TILES; ++t) {
                        f64x4 ere = Cre[a][t], eim = Cim[a][t];
                        if (closing != nullptr) {
#pragma unroll
                            for (int s = 0; s < 4; ++s) {
                                const cplx v = Rc[(a*N + q + 4*s)*rstride + colA[t]];
                                ere = __builtin_amdgcn_mfma_f64_16x16x4f64(v.re, Lam[s], ere, 0, 0, 0);
                                eim = __builtin_amdgcn_mfma_f64_16x16x4f64(v.im, Lam[s], eim, 0, 0, 0);
                            }
                        }
#pragma unroll
                        for (int s = 0; s < kSpectra; ++s) {
                            if (sp0 + s >= n_spectra) continue;
                            const double* wrow = Ws + (s*A + a)*WT + 16*t + q;
                            if (mode == 2) {
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const double wgt = wrow[4*r];
                                    Gre[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(ere[r], wgt*ere[r], Gre[s], 0, 0, 0);
                                    Gim[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(eim[r], wgt*eim[r], Gim[s], 0, 0, 0);
                                }
                            } else {
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    dsum[s] = fma(wrow[4*r], fma(ere[r], ere[r], eim[r]*eim[r]), dsum[s]);
                            }
                        }
                    }
#pragma unroll
                    for (int s = 0; s < kSpectra; ++s) {
                        if (sp0 + s >= n_spectra) continue;
                        double* o = pos0 + (static_cast<size_t>(sp0 + s)*n_idx + sel[a])*tile;
                        if (mode == 2) {
                            const f64x4 acc = Gre[s] + Gim[s];
#pragma unroll
                            for (int r = 0; r < 4; ++r) o[(q + 4*r)*N + c] = acc[r];
                        } else {
                            double sum = dsum[s];
                            sum += __shfl_xor(sum, 16);
                            sum += __shfl_xor(sum, 32);
                            if (lane < 16) o[c] = sum;
                        }
                    }
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

// out (n_spectra, n_index, n_idx[, N[, N]]): the frequency blocks of partial (blocks, n_index, n_spectra, n_idx, N[, N])
// added in index order.  Mode 2 reads entry (min(k, l), max(k, l)) for (k, l); mode 0 adds the N sums in index order
// and divides by d.
__global__ __launch_bounds__(256) void seqpre_reduce_kernel(const double* __restrict__ partial, int blocks,
                                                            size_t n_index, int n_spectra, int n_idx, int N, int d,
                                                            int mode, double* __restrict__ out) {
    const size_t out_tile = mode == 2 ? size_t(N)*N : mode == 1 ? size_t(N) : 1;
    const size_t in_tile = mode == 2 ? size_t(N)*N : size_t(N);
    const size_t members = n_index*n_spectra*n_idx;
    const size_t o = static_cast<size_t>(blockIdx.x)*256 + threadIdx.x;
    if (o >= members*out_tile) return;
    const size_t e = o % out_tile, m = o / out_tile;
    const size_t i = m % n_idx, pos = (m / n_idx) % n_index, sp = m / (n_idx*n_index);
    const double* src = partial + ((pos*n_spectra + sp)*n_idx + i)*in_tile;
    const size_t stride = members*in_tile;
    auto blocks_sum = [&](size_t at) {
        double acc = src[at];
        for (int b = 1; b < blocks; ++b) acc += src[static_cast<size_t>(b)*stride + at];
        return acc;
    };
    if (mode == 2) {
        const size_t k = e / N, l = e % N;
        out[o] = blocks_sum(k <= l ? k*N + l : l*N + k);
    } else if (mode == 1) {
        out[o] = blocks_sum(e);
    } else {
        double acc = blocks_sum(0);
        for (int n = 1; n < N; ++n) acc += blocks_sum(n);
        out[o] = acc/d;
    }
}

}  // namespace

int sequence_prefix_block_width(int d, int A) {
    return d == 2 ? 64 : 16*seq4_tiles(A);
}

int sequence_prefix_spectra_per_walk() {
    return kSpectra;
}

bool sequence_prefix_staged(int d, int T, int A) {
    if (d == 2) return staged2_lds_bytes(T, A) <= 150*1024;
    return staged4_lds_bytes(T, A) + weights4_lds_bytes(A) <= 150*1024;
}

hipError_t launch_sequence_prefix(int d, const cplx* phases, const cplx* const* Rtab, const double* Lpulse,
                                  const int32_t* offsets, const int32_t* index, const int32_t* closing,
                                  const int32_t* order, int P, size_t n_index, int T, int A, int W, const cplx* scale,
                                  int s_ndim, int n_spectra, const int32_t* idx, int n_idx, int mode, double* partial,
                                  double* out, hipStream_t stream) {
    if (A < 1 || A > 4 || P < 1 || T < 1 || W < 1 || n_spectra < 1 || n_idx < 1 || n_idx > A || mode < 0 || mode > 2 ||
        (s_ndim != 1 && s_ndim != 2) || (d != 2 && d != 4) || n_index < size_t(P) || n_index > 0x7fffffffull)
        return hipErrorInvalidValue;
    const bool staged = sequence_prefix_staged(d, T, A);
    const int width = sequence_prefix_block_width(d, A);
    const int blocks = (W + width - 1)/width;
    const int walks = (n_spectra + kSpectra - 1)/kSpectra;
    if (walks > 65535) return hipErrorInvalidValue;
    // as launch_sequence_second_order: staged, one block per CU; else a few; never more groups than wavefronts' worth
    // of sequences
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
                           mode, partial);
        return hipGetLastError();
    };
    hipError_t err = hipErrorInvalidValue;
#define FFK_SEQPRE(AA)                                                                                              \
    case AA:                                                                                                        \
        if (d == 2)                                                                                                 \
            err = staged ? launch(seqpre_walk2_kernel<AA, true>, staged2_lds_bytes(T, AA))                          \
                         : launch(seqpre_walk2_kernel<AA, false>, 0);                                               \
        else                                                                                                        \
            err = staged ? launch(seqpre_walk4_kernel<AA, true>, staged4_lds_bytes(T, AA) + weights4_lds_bytes(AA)) \
                         : launch(seqpre_walk4_kernel<AA, false>, weights4_lds_bytes(AA));                          \
        break;
    switch (A) {
        FFK_SEQPRE(1) FFK_SEQPRE(2) FFK_SEQPRE(3) FFK_SEQPRE(4)
        default: break;
    }
#undef FFK_SEQPRE
    if (err != hipSuccess) return err;
    const int N = d*d;
    const size_t out_tile = mode == 2 ? size_t(N)*N : mode == 1 ? size_t(N) : 1;
    const size_t n = n_index*n_spectra*n_idx*out_tile;
    if ((n + 255)/256 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(seqpre_reduce_kernel, dim3(static_cast<unsigned>((n + 255)/256)), dim3(256), 0, stream, partial,
                       blocks, n_index, n_spectra, n_idx, N, d, mode, out);
    return hipGetLastError();
}

}  // namespace ffk

// sequence_prefix.hip -- infidelities and decay amplitudes of every PREFIX of many gate sequences drawn from one table
// of distinct gates, optionally with a closing gate behind each prefix, in one forward walk of each sequence
// (ff.sequence_prefix_infidelities, ff.sequence_prefix_decay_amplitudes; ffk_sequence_prefix_processes).
//
// The concatenation rule is a sum over the positions, R = sum_g phi_{g-1} R_{k_g} Lam_g, so the control matrix of the
// prefix of m gates is the partial sum Cum_m, which the forward walk carries as C_m (sequence_walk.h: recurrences,
// operand maps, determinism).  With a closing gate c_g behind the prefix the control matrix is
// Cum_g + phi_g R_{c_g} Lam_{g+1}, i.e.
//     E_g       = C_g + R_{c_g} Lam_{g+1}             (C_g itself is not changed)
// up to the common phase phi_g, which cancels in
//     Gamma_g[k, l] = sum_w c_w S(w) (Re E_g[k, w] Re E_g[l, w] + Im E_g[k, w] Im E_g[l, w]).
// A prefix quantity is therefore one epilogue per position, from the state.  Position g sees nothing behind it: the
// curve of s[:m] is the first m rows of the curve of s, bit for bit.  Fresh accumulators for every (position,
// operator, spectrum), at most kSpectra spectra per walk; closing gates are a runtime pointer.
//
//   mode 0, 1   partial[block][position][spectrum][i][N]      sum_w c_w S(w) |E[k, w]|^2   (the diagonal of Gamma)
//   mode 2      partial[block][position][spectrum][i][N][N]   Gamma; only k <= l is read back
//
//   seqpre_walk2_kernel   d = 2: the lane-local products of a position (ten k <= l, or four squares) are summed over
//                         the wavefront by a butterfly that halves the values a lane carries at every step
//                         (wave_sums): about one shuffle per value, a fixed order
//   seqpre_walk4_kernel   d = 4: E is C + Y with the eight matrix instructions of Y accumulating onto C's registers;
//                         mode 2 is the Gram matrix of E over the block's frequencies (real and imaginary chains, added
//                         at the end), modes 0 and 1 the lane's own 4 TILES frequencies in a fixed order, then the four
//                         row groups by two shuffles
//   seqpre_reduce_kernel  the frequency blocks in index order; mode 2 reads (min(k, l), max(k, l)): symmetric bit for
//                         bit; mode 0 adds the N diagonal sums in index order and divides by d
#include "sequence_walk.h"

namespace ffk {
namespace {

using namespace seqwalk;

constexpr int kSpectra = 2;              // spectra of one walk; grid z carries the others

// ---- d = 2 -------------------------------------------------------------------------------------------------------
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
        stage_tables2<ROWS>(Rs, Ps, phases, Rtab, T, W, wc, lane, wave, n_waves);
        __syncthreads();
    }
    int sel[A];
    double wt[A][kSpectra];
    select_weights2(scale, s_ndim, n_spectra, idx, n_idx, sp0, w, wc, W, sel, wt);
    // where this lane's value of a reduced set goes: value e = lane >> 2 of the ten products k <= l (mode 2), lane >> 4
    // of the four squares
    const int e10 = lane >> 2;
    const int tk = (e10 >= 4) + (e10 >= 7) + (e10 >= 9);
    const int tl = e10 - (tk == 0 ? 0 : tk == 1 ? 3 : tk == 2 ? 5 : 6);
    const bool stores2 = (lane & 3) == 0 && e10 < 10, stores1 = (lane & 15) == 0;
    const size_t tile = mode == 2 ? LN : N;
    const size_t per_position = static_cast<size_t>(n_spectra)*n_idx*tile;
    int vzero;                               // (the small matrices and, read from L2, the gates' rows: sequence_walk.h)
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
            const int my_index = chunk_gates(index, true, c0, c1, lane);
            const int my_closing = chunk_gates(closing, closing != nullptr, c0, c1, lane);
            for (int g = c0; g < c1; ++g) {
                const int k = gate_at(my_index, g - c0), kc = gate_at(my_closing, g - c0);
                const cplx* Rg = gate_rows2<ROWS, STAGED>(Rs, Rtab, k, vzero, lane, wc);
                const cplx* Rc = gate_rows2<ROWS, STAGED>(Rs, Rtab, kc, vzero, lane, wc);
                const size_t rstride = row_stride2<STAGED>(W, vzero);
                const cplx ph = gate_phase2<STAGED>(Ps, phases, k, vzero, W, lane, wc);
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    if (sel[a] < 0) continue;
                    cplx X[N];
                    summand2(Rg, a, rstride, Lam, X);
                    fold2(ph, X, C, a);
                }
                advance2(Lpulse + static_cast<size_t>(k)*LN + vzero, Lam);
                // the epilogue of this position
                double* pos0 = partial + (static_cast<size_t>(blockIdx.x)*n_index + g)*per_position;
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    if (sel[a] < 0) continue;
                    cplx E[N];
#pragma unroll
                    for (int jj = 0; jj < N; ++jj) E[jj] = C[a*N + jj];
                    if (closing != nullptr) add_summand2(Rc, a, rstride, Lam, E);
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
                            const double sum = wave_sums<16, false>(v, lane);
                            if (stores2) o[tk*N + tl] = sum;
                        } else {
                            double v[N];
#pragma unroll
                            for (int kk = 0; kk < N; ++kk)
                                v[kk] = wt[a][s]*fma(E[kk].re, E[kk].re, E[kk].im*E[kk].im);
                            const double sum = wave_sums<N, false>(v, lane);
                            if (stores1) o[lane >> 4] = sum;
                        }
                    }
                }
            }
        }
    }
}

// ---- d = 4 -------------------------------------------------------------------------------------------------------
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
    double* Ws = reinterpret_cast<double*>(lds_raw);                                      // [kSpectra][A][WT]
    cplx* Rs = reinterpret_cast<cplx*>(lds_raw + kSpectra*A*WT*sizeof(double));           // [T][ROWS][WT]
    cplx* Ps = Rs + static_cast<size_t>(T)*ROWS*WT;                                       // [T][WT]
    int sel[A];
#pragma unroll
    for (int a = 0; a < A; ++a) sel[a] = selected(idx, n_idx, a);
    stage_weights4<A, kSpectra, WT>(Ws, scale, s_ndim, n_spectra, idx, n_idx, sp0, w0, W);
    if (STAGED) stage_tables4<ROWS, WT>(Rs, Ps, phases, Rtab, T, W, w0, lane, wave, n_waves);
    __syncthreads();
    size_t colA[TILES], colD[TILES][4];
    columns4<STAGED>(colA, colD, w0, W, c, q);
    const size_t rstride = row_stride4<WT, STAGED>(W);
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
            const int my_index = chunk_gates(index, true, c0, c1, lane);
            const int my_closing = chunk_gates(closing, closing != nullptr, c0, c1, lane);
            for (int g = c0; g < c1; ++g) {
                const int k = gate_at(my_index, g - c0), kc = gate_at(my_closing, g - c0);
                const cplx* Rg = gate_rows4<ROWS, WT, STAGED>(Rs, Rtab, k);
                const cplx* Rc = gate_rows4<ROWS, WT, STAGED>(Rs, Rtab, kc);
                const cplx* Pg = gate_phases4<WT, STAGED>(Ps, phases, k, W);
#pragma unroll
                for (int t = 0; t < TILES; ++t) {
                    cplx ph[4];
                    load_phases4(Pg, colD[t], ph);
#pragma unroll
                    for (int a = 0; a < A; ++a) {
                        if (sel[a] < 0) continue;
                        fold4(ph, add_summand4(Rg + (a*N + q)*rstride + colA[t], rstride, Lam, {zero, zero}), Cre[a][t],
                              Cim[a][t]);
                    }
                }
                advance4(Lpulse + static_cast<size_t>(k)*N*N + c*N + q, Lam);
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
                        tile4 E = {Cre[a][t], Cim[a][t]};
                        if (closing != nullptr) E = add_summand4(Rc + (a*N + q)*rstride + colA[t], rstride, Lam, E);
#pragma unroll
                        for (int s = 0; s < kSpectra; ++s) {
                            if (sp0 + s >= n_spectra) continue;
                            const double* wrow = Ws + (s*A + a)*WT + 16*t + q;
                            if (mode == 2) {
                                gram4(wrow, E, E.re, E.im, Gre[s], Gim[s]);
                            } else {
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    dsum[s] = fma(wrow[4*r], fma(E.re[r], E.re[r], E.im[r]*E.im[r]), dsum[s]);
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
    return block_width(d, A);
}

int sequence_prefix_spectra_per_walk() {
    return kSpectra;
}

bool sequence_prefix_staged(int d, int T, int A) {
    return tables_staged(d, T, A, kSpectra);
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
    const int blocks = (W + block_width(d, A) - 1)/block_width(d, A);
    const int walks = (n_spectra + kSpectra - 1)/kSpectra;
    if (walks > 65535) return hipErrorInvalidValue;
    const int n_groups = walk_groups(staged, blocks, walks, P);
    const dim3 grid(blocks, n_groups, walks);
    const size_t lds = walk_lds_bytes(d, staged, T, A, kSpectra);
    auto launch = [&](auto kern) {
        return launch_walk(kern, grid, lds, stream, phases, Rtab, Lpulse, offsets, index, closing, order, P,
                           static_cast<int>(n_index), T, W, n_groups, scale, s_ndim, n_spectra, idx, n_idx, mode,
                           partial);
    };
    const hipError_t err = for_operators(A, [&](auto AA) {
        constexpr int a = decltype(AA)::value;
        if (d == 2) return staged ? launch(seqpre_walk2_kernel<a, true>) : launch(seqpre_walk2_kernel<a, false>);
        return staged ? launch(seqpre_walk4_kernel<a, true>) : launch(seqpre_walk4_kernel<a, false>);
    });
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

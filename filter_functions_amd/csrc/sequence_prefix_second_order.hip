// sequence_prefix_second_order.hip -- frequency shifts (second order) of every PREFIX of many gate sequences drawn from
// one table of distinct gates, optionally with a closing gate behind each prefix, in one forward walk of each sequence
// (ff.sequence_prefix_frequency_shifts; ffk_sequence_prefix_frequency_shifts).
//
// The forward walk (sequence_walk.h: recurrences, operand maps, determinism) holds, after position m, the running sum
//     Z_m = sum_{g <= m} [ Lam_g^T Delta_gate(k_g) Lam_g + sum_w c_w S(w) Re( conj(Rs_g[k, w]) Cum_{g-1}[l, w] ) ]
// which is the frequency shift of the first m gates.  A closing gate c behind them adds one more summand of the same
// form, with the state the walk holds after the position (Lam_{m+1}, C_m = conj(phi_m) Cum_m; the common phase cancels):
//     X_c     = R_c Lam_{m+1}
//     Delta_m = Z_m + Lam_{m+1}^T Delta_gate(c) Lam_{m+1} + sum_w c_w S(w) (Re X_c[w, k] Re C_m[w, l] + Im X_c[w, k] Im C_m[w, l])
// A prefix quantity is therefore one epilogue per position on COPIES of the accumulators; the running accumulators go
// on untouched, and position g sees nothing behind it: the curve of s[:m] is the first m rows of the curve of s, bit
// for bit.  The gates' own shifts are frequency independent: frequency block 0 adds them.  Fresh accumulators of the
// closing summand for every (position, operator, spectrum); the spectra per walk depend on d, A and whether closing
// gates are given (a template parameter here) alone.
//
//   partial[block][position][spectrum][i][N][N]
//
//   seqpre2o_walk2_kernel   d = 2: per position the 16 entries of Z (plus the closing summand) are summed over the
//                           wavefront by the halving butterfly (wave_sums); lane 0 of block 0 carries the
//                           Lam^T Delta_gate Lam terms
//   seqpre2o_walk4_kernel   d = 4: per position the lane forms (Z_re + Z_im) + Z_Delta from copies; with a closing gate
//                           X_c = R_c Lam (8 matrix instructions per operator, tile and spectrum), its Gram with weight
//                           C into fresh Y_re, Y_im (8 more) and, in block 0, Y_Delta = Lam^T (Delta_gate(c) Lam); the
//                           stored tile is ((Z_re + Z_im) + Z_Delta) + ((Y_re + Y_im) + Y_Delta).  32-bit columns.
//   seqpre2o_reduce_kernel  out[sp][position][i] = sum over the frequency blocks, in index order
#include "sequence_walk.h"

namespace ffk {
namespace {

using namespace seqwalk;

// spectra of one walk (accumulator sets); grid z carries the others.  A function of (d, A, closing) alone.
constexpr int spectra_per_walk(int d, int A, bool closing) {
    return (A >= 4 || (d == 4 && closing && A >= 3)) ? 1 : 2;
}

// ---- d = 2 -------------------------------------------------------------------------------------------------------
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
        stage_tables2<ROWS>(Rs, Ps, phases, Rtab, T, W, wc, lane, wave, n_waves);
        __syncthreads();
    }
    int sel[A];
    double wt[A][S];
    select_weights2(scale, s_ndim, n_spectra, idx, n_idx, sp0, w, wc, W, sel, wt);
    const bool shifts_here = blockIdx.x == 0 && lane == 0;
    const bool stores = (lane & 3) == 0;                              // value lane >> 2 of the 16 ends here
    const size_t per_position = static_cast<size_t>(n_spectra)*n_idx*LN;
    int vzero;                               // (the small matrices and, read from L2, the gates' rows: sequence_walk.h)
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
            const int my_index = chunk_gates(index, true, c0, c1, lane);
            const int my_closing = chunk_gates(closing, CLOSING, c0, c1, lane);
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
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        if (sp0 + s >= n_spectra) continue;
                        gram2<false>(wt[a][s], X, C, a, Z[a][s]);
                    }
                    fold2(ph, X, C, a);
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
                advance2(Lpulse + static_cast<size_t>(k)*LN + vzero, Lam);
                // the epilogue of this position: copies of Z, plus the closing gate's summand
                double* pos0 = partial + (static_cast<size_t>(blockIdx.x)*n_index + g)*per_position;
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    if (sel[a] < 0) continue;
                    cplx Xc[N];
                    if (CLOSING) summand2(Rc, a, rstride, Lam, Xc);
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        if (sp0 + s >= n_spectra) continue;
                        double v[LN];
                        if (CLOSING) {
                            // the closing gate's summand first, fresh, then the copy of Z in front of it
                            gram2<true>(wt[a][s], Xc, C, a, v);
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

// ---- d = 4 -------------------------------------------------------------------------------------------------------
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
    double* Ws = reinterpret_cast<double*>(lds_raw);                                      // [S][A][WT]
    cplx* Rs = reinterpret_cast<cplx*>(lds_raw + S*A*WT*sizeof(double));                  // [T][ROWS][WT]
    cplx* Ps = Rs + static_cast<size_t>(T)*ROWS*WT;                                       // [T][WT]
    int sel[A];
#pragma unroll
    for (int a = 0; a < A; ++a) sel[a] = selected(idx, n_idx, a);
    stage_weights4<A, S, WT>(Ws, scale, s_ndim, n_spectra, idx, n_idx, sp0, w0, W);
    if (STAGED) stage_tables4<ROWS, WT>(Rs, Ps, phases, Rtab, T, W, w0, lane, wave, n_waves);
    __syncthreads();
    int colA[TILES], colD[TILES][4];                                  // (32-bit: sequence_walk.h, columns4)
    columns4<STAGED>(colA, colD, w0, W, c, q);
    const size_t rstride = row_stride4<WT, STAGED>(W);
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
            const int my_index = chunk_gates(index, true, c0, c1, lane);
            const int my_closing = chunk_gates(closing, CLOSING, c0, c1, lane);
            for (int g = c0; g < c1; ++g) {
                const int k = gate_at(my_index, g - c0), kc = gate_at(my_closing, g - c0);
                const cplx* Rg = gate_rows4<ROWS, WT, STAGED>(Rs, Rtab, k);
                const cplx* Pg = gate_phases4<WT, STAGED>(Ps, phases, k, W);
#pragma unroll
                for (int t = 0; t < TILES; ++t) {
                    cplx ph[4];
                    load_phases4(Pg, colD[t], ph);
#pragma unroll
                    for (int a = 0; a < A; ++a) {
                        if (sel[a] < 0) continue;
                        const tile4 X = add_summand4(Rg + (a*N + q)*rstride + colA[t], rstride, Lam, {zero, zero});
#pragma unroll
                        for (int s = 0; s < S; ++s) {
                            if (sp0 + s >= n_spectra) continue;
                            // (gram4 of sequence_walk.h, written out: as a call on the running accumulators the
                            // A = 1 walks hold fewer of them in accumulator registers, 208 registers in all, below the
                            // range the host test asserts; the closing summand below takes the call)
                            const double* wrow = Ws + (s*A + a)*WT + 16*t + q;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const double wt = wrow[4*r];
                                Zre[a][s] = __builtin_amdgcn_mfma_f64_16x16x4f64(X.re[r], wt*Cre[a][t][r], Zre[a][s],
                                                                                 0, 0, 0);
                                Zim[a][s] = __builtin_amdgcn_mfma_f64_16x16x4f64(X.im[r], wt*Cim[a][t][r], Zim[a][s],
                                                                                 0, 0, 0);
                            }
                        }
                        fold4(ph, X, Cre[a][t], Cim[a][t]);
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
                            add_rotated4(gate_shifts + ((static_cast<size_t>(sp0 + s)*T + k)*n_idx + sel[a])*N*N + c*N + q,
                                         Lam, Zd[a][s]);
                        }
                    }
                }
                advance4(Lpulse + static_cast<size_t>(k)*N*N + c*N + q, Lam);
                // the epilogue of this position: copies of the accumulators, plus the closing gate's summand
                double* pos0 = partial + (static_cast<size_t>(blockIdx.x)*n_index + g)*per_position;
                const cplx* Rc = gate_rows4<ROWS, WT, STAGED>(Rs, Rtab, kc);
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
                                const tile4 X =
                                    add_summand4(Rc + (a*N + q)*rstride + colA[t], rstride, Lam, {zero, zero});
                                gram4(Ws + (s*A + a)*WT + 16*t + q, X, Cre[a][t], Cim[a][t], Yre, Yim);
                            }
                            f64x4 y = Yre + Yim;
                            if (shifts_here) {
                                f64x4 Yd = zero;
                                add_rotated4(gate_shifts +
                                                 ((static_cast<size_t>(sp0 + s)*T + kc)*n_idx + sel[a])*N*N + c*N + q,
                                             Lam, Yd);
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
    return block_width(d, A);
}

int sequence_prefix_second_order_spectra_per_walk(int d, int A, bool closing) {
    return spectra_per_walk(d, A, closing);
}

bool sequence_prefix_second_order_staged(int d, int T, int A, bool closing) {
    return tables_staged(d, T, A, spectra_per_walk(d, A, closing));
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
    const int blocks = (W + block_width(d, A) - 1)/block_width(d, A);
    const int per_walk = spectra_per_walk(d, A, has_closing);
    const int walks = (n_spectra + per_walk - 1)/per_walk;
    if (walks > 65535) return hipErrorInvalidValue;
    const int n_groups = walk_groups(staged, blocks, walks, P);
    const dim3 grid(blocks, n_groups, walks);
    const size_t lds = walk_lds_bytes(d, staged, T, A, per_walk);
    auto launch = [&](auto kern) {
        return launch_walk(kern, grid, lds, stream, phases, Rtab, Lpulse, offsets, index, closing, order, P,
                           static_cast<int>(n_index), T, W, n_groups, scale, s_ndim, n_spectra, idx, n_idx,
                           gate_shifts, partial);
    };
    auto walk = [&](auto AA, auto CL) {
        constexpr int a = decltype(AA)::value;
        constexpr bool cl = decltype(CL)::value;
        if (d == 2)
            return staged ? launch(seqpre2o_walk2_kernel<a, true, cl>) : launch(seqpre2o_walk2_kernel<a, false, cl>);
        return staged ? launch(seqpre2o_walk4_kernel<a, true, cl>) : launch(seqpre2o_walk4_kernel<a, false, cl>);
    };
    const hipError_t err = for_operators(A, [&](auto AA) {
        return has_closing ? walk(AA, std::true_type{}) : walk(AA, std::false_type{});
    });
    if (err != hipSuccess) return err;
    const size_t tile = static_cast<size_t>(d)*d*d*d;
    const size_t n = n_index*n_spectra*n_idx*tile;
    if ((n + 255)/256 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(seqpre2o_reduce_kernel, dim3(static_cast<unsigned>((n + 255)/256)), dim3(256), 0, stream,
                       partial, blocks, n_index, n_spectra, n_idx, tile, out);
    return hipGetLastError();
}

}  // namespace ffk

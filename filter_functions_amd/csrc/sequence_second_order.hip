// sequence_second_order.hip -- frequency shifts (second order) of many gate sequences drawn from one table of distinct
// gates, in one walk of each sequence (ff.sequence_frequency_shifts; ffk_sequence_frequency_shifts).
//
// The rotated concatenation rule of the second-order filter function (numeric.
// calculate_second_order_filter_function_from_atomic), integrated against the spectrum, is
//     Delta = sum_g [ Lam_g^T Delta_gate(k_g) Lam_g  +  sum_w c_w S_a(w) Re( conj(Rs_g[k, w]) Cum_{g-1}[l, w] ) ]
// with Rs_g = phi_{g-1} (R_{k_g} Lam_g) the rule's summand and Cum_{g-1} the sum of the summands before it: the sum Z
// of the forward walk (sequence_walk.h: recurrences, operand maps, determinism).  The epilogue is one tile per
// sequence, operator and spectrum.  Z is linear in the weights: a block forms the partial Z of its frequencies and
// seq2o_reduce_kernel adds the blocks.  The gates' own shifts are frequency independent: frequency block 0 adds them.
// At most kSpectra spectra per walk.
//
//   seq2o_walk2_kernel   d = 2: Z (4 x 4 per operator and spectrum) per lane; one butterfly per sequence; lane 0 of
//                        block 0 carries the gates' own shifts.  The gates' rows are addressed through scalars.
//   seq2o_walk4_kernel   d = 4: Z_re, Z_im and Z_Delta tiles per operator and spectrum, added at the end
//   seq2o_reduce_kernel  out[sp][p][i] = sum over the frequency blocks, in index order
#include "sequence_walk.h"

namespace ffk {
namespace {

using namespace seqwalk;

constexpr int kSpectra = 2;              // spectra of one walk (accumulator sets); grid z carries the others

// ---- d = 2 -------------------------------------------------------------------------------------------------------
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
        stage_tables2<ROWS>(Rs, Ps, phases, Rtab, T, W, wc, lane, wave, n_waves);
        __syncthreads();
    }
    int sel[A];
    double wt[A][kSpectra];
    select_weights2(scale, s_ndim, n_spectra, idx, n_idx, sp0, w, wc, W, sel, wt);
    const bool shifts_here = blockIdx.x == 0 && lane == 0;
    int vzero;                                                        // (the small matrices: sequence_walk.h)
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
            const int my_index = chunk_gates(index, true, c0, c1, lane);
            for (int g = c0; g < c1; ++g) {
                const int k = gate_at(my_index, g - c0);
                const cplx* Rg = gate_rows2<ROWS, STAGED>(Rs, Rtab, k, 0, lane, wc);
                const size_t rstride = row_stride2<STAGED>(W, 0);
                const cplx ph = gate_phase2<STAGED>(Ps, phases, k, 0, W, lane, wc);
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    if (sel[a] < 0) continue;
                    cplx X[N];
                    summand2(Rg, a, rstride, Lam, X);
#pragma unroll
                    for (int s = 0; s < kSpectra; ++s) {
                        if (sp0 + s >= n_spectra) continue;
                        gram2<false>(wt[a][s], X, C, a, Z[a][s]);
                    }
                    fold2(ph, X, C, a);
                    if (shifts_here) {
                        // Lam^T Delta_gate Lam of this position, for every spectrum of the walk
#pragma unroll
                        for (int s = 0; s < kSpectra; ++s) {
                            if (sp0 + s >= n_spectra) continue;
                            add_rotated2(gate_shifts + ((static_cast<size_t>(sp0 + s)*T + k)*n_idx + sel[a])*LN + vzero,
                                         Lam, Z[a][s]);
                        }
                    }
                }
                advance2(Lpulse + static_cast<size_t>(k)*LN + vzero, Lam);
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

// ---- d = 4 -------------------------------------------------------------------------------------------------------
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
            const int my_index = chunk_gates(index, true, c0, c1, lane);
            for (int g = c0; g < c1; ++g) {
                const int k = gate_at(my_index, g - c0);
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
                        for (int s = 0; s < kSpectra; ++s) {
                            if (sp0 + s >= n_spectra) continue;
                            gram4(Ws + (s*A + a)*WT + 16*t + q, X, Cre[a][t], Cim[a][t], Zre[a][s], Zim[a][s]);
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
                        for (int s = 0; s < kSpectra; ++s) {
                            if (sp0 + s >= n_spectra) continue;
                            add_rotated4(gate_shifts + ((static_cast<size_t>(sp0 + s)*T + k)*n_idx + sel[a])*N*N + c*N + q,
                                         Lam, Zd[a][s]);
                        }
                    }
                }
                advance4(Lpulse + static_cast<size_t>(k)*N*N + c*N + q, Lam);
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
    return block_width(d, A);
}

int sequence_second_order_spectra_per_walk() {
    return kSpectra;
}

bool sequence_second_order_staged(int d, int T, int A) {
    return tables_staged(d, T, A, kSpectra);
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
    const int blocks = (W + block_width(d, A) - 1)/block_width(d, A);
    const int walks = (n_spectra + kSpectra - 1)/kSpectra;
    if (walks > 65535) return hipErrorInvalidValue;
    const int n_groups = walk_groups(staged, blocks, walks, P);
    const dim3 grid(blocks, n_groups, walks);
    const size_t lds = walk_lds_bytes(d, staged, T, A, kSpectra);
    auto launch = [&](auto kern) {
        return launch_walk(kern, grid, lds, stream, phases, Rtab, Lpulse, offsets, index, order, P, T, W, n_groups,
                           scale, s_ndim, n_spectra, idx, n_idx, gate_shifts, partial);
    };
    const hipError_t err = for_operators(A, [&](auto AA) {
        constexpr int a = decltype(AA)::value;
        if (d == 2) return staged ? launch(seq2o_walk2_kernel<a, true>) : launch(seq2o_walk2_kernel<a, false>);
        return staged ? launch(seq2o_walk4_kernel<a, true>) : launch(seq2o_walk4_kernel<a, false>);
    });
    if (err != hipSuccess) return err;
    const size_t row = static_cast<size_t>(n_idx)*d*d*d*d;
    const size_t n = static_cast<size_t>(P)*n_spectra*row;
    if ((n + 255)/256 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(seq2o_reduce_kernel, dim3(static_cast<unsigned>((n + 255)/256)), dim3(256), 0, stream, partial,
                       blocks, P, n_spectra, row, out);
    return hipGetLastError();
}

}  // namespace ffk

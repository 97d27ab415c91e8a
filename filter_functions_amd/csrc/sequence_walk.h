// sequence_walk.h -- the FORWARD walk of the concatenation rule along a gate sequence, once, for the kernels of
// sequence_second_order.hip, sequence_prefix.hip and sequence_prefix_second_order.hip.  Those files keep their kernels,
// their epilogues and their entry points; every step of the walk, and the host code that sizes it, is here.
//
// The walk goes forward through the positions g of a sequence (gate k_g of the table) and carries
//     X_g       = R_{k_g} Lam_g                       (the rule's summand without its phase)
//     C_g       = conj(p_{k_g}) (C_{g-1} + X_g)       (= conj(phi_g) Cum_g: only the gate's own phase is needed)
//     Lam_{g+1} = L_{k_g} Lam_g                       (16 x 16 or 4 x 4 real, the same for every frequency)
// with Lam_g the Liouville matrix of the propagator before position g and Cum_g the sum of the rule's summands
// phi_{g-1} X_g up to position g, i.e. the control matrix of the first g gates.  The second-order kernels add
//     Z        += sum_w c_w S_a(w) (Re X_g[k] Re C_{g-1}[l] + Im X_g[k] Im C_{g-1}[l])  [+ Lam_g^T Delta_gate Lam_g]
// in which the common phase phi_{g-1} cancels.  The forward form is chosen because the frequency-dependent operand of
// its product, the gate's control matrix, comes from the table at every position and can be read in either operand
// layout, while the other operand, Lam, lies in the accumulator layout of the matrix instruction, which is an operand
// layout for a contraction over its rows.  X_g then comes out with the frequency along the rows -- the layout of both
// operands of a Gram matrix over the frequencies -- and nothing is ever transposed (the backward recurrence of
// sequences_d4.hip holds its state with the frequency along the columns and would need an LDS round trip per position
// and operator).
//
//   d = 2   lane = frequency; Lam (4 x 4), C (4 per operator) and the accumulators per lane; the gates' tables staged
//           as [T][ROWS][64] control matrices and [T][64] phases, or read from L2
//   d = 4   v_mfma_f64_16x16x4_f64 (operand maps: header comment of sequences_d4.hip).  Lam is held as
//           D[row = q + 4 r][col = c] (c = lane & 15, q = lane >> 4, register r).  K-step s of X = R Lam has the A
//           operand R[a, q + 4 s] at frequency 16 t + c and the B operand register s of Lam; X and C are D tiles with
//           row = frequency 16 t + q + 4 r, col = basis element c.  K-step r of the Gram has the A operand register r
//           of X and the B operand register r of C times the weight; real and imaginary products go to accumulators
//           of their own and are added at the end.  Lam^T (Delta Lam) and L Lam are products of the same kind with
//           Lam's registers as B (and A) operands.  Tables staged as [T][ROWS][WT] and [T][WT] behind the weights
//           [S][A][WT], WT = 16 seq4_tiles(A) frequencies a block.
//
// Determinism: a block forms the partial results of its frequencies and a reduce kernel adds the blocks in index
// order.  No atomics, no waits between wavefronts or blocks, a block width that depends on d and A alone, and a number
// of spectra per walk fixed by the kernel (grid z carries the further ones): a result is the same bits whatever else
// is in the pass.
//
// Register pressure: every function is inlined into its kernel and takes arrays by reference; the d = 4 summand goes
// in and out by value (tile4).  What a kernel needs to stay within its registers is a parameter here -- vz (0, or a
// zero held in a vector register, which keeps addresses that are the same for every lane out of the scalar
// registers), OPAQUE of wave_sums, the type of the d = 4 columns.  The kernels keep their accumulators in arrays of
// f64x4, real and imaginary parts apart: held as arrays of tile4 the closing-gate kernels need 30 registers more.
#pragma once

#include <algorithm>
#include <type_traits>

#include "ffk_internal.h"

namespace ffk {
namespace seqwalk {

using f64x4 = __attribute__((ext_vector_type(4))) double;
struct tile4 { f64x4 re, im; };          // real and imaginary parts of a summand's D tile (d = 4)

constexpr int kWaves = 4;                // one wavefront per SIMD: the whole register file of 512 each
constexpr int kN2 = 4;                   // Liouville dimension at d = 2
constexpr int kN = 16;                   // ... and at d = 4

// tiles of sixteen frequencies a wavefront walks at once: 64 A accumulator registers at four tiles, which A <= 2
// affords; A = 3 and 4 take two tiles (32 frequencies), 96 and 128 accumulator registers
constexpr int seq4_tiles(int A) { return A <= 2 ? 4 : 2; }

// ---- common ------------------------------------------------------------------------------------------------------
// the row of the weights of selected operator i under spectrum sp: (n_spectra, W) or (n_spectra, n_idx, W)
__device__ __forceinline__ const cplx* weight_row(const cplx* scale, int s_ndim, int n_idx, int sp, int i, int W) {
    return scale + static_cast<size_t>(s_ndim == 1 ? sp : sp*n_idx + i)*W;
}

// which selected operator operator a is (-1: none; the first of idx that names it)
__device__ __forceinline__ int selected(const int32_t* idx, int n_idx, int a) {
    int i = -1;
    for (int m = n_idx - 1; m >= 0; --m)
        if (idx[m] == a) i = m;
    return i;
}

// The gate numbers of positions [c0, c1) of a chunk of at most 64, one per lane (0 beyond c1, or if the list is not
// present), and the gate of position c0 + at of the chunk, the same in every lane.
__device__ __forceinline__ int chunk_gates(const int32_t* list, bool present, int c0, int c1, int lane) {
    return (present && c0 + lane < c1) ? list[c0 + lane] : 0;
}
__device__ __forceinline__ int gate_at(int chunk, int at) { return __builtin_amdgcn_readlane(chunk, at); }

// The sums over the wavefront of VP values per lane (VP a power of two, at most 64).  At every step a lane keeps one
// half of its values and hands the other half to its partner, so the values a lane carries halve; once one is left
// the remaining steps are a plain butterfly.  Returns the sum of value number lane >> (6 - log2 VP), the same in the
// 64/VP lanes that share it.  The order of the additions depends on the lane numbers alone.
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
// the tables of the block's frequencies to LDS: Rs [T][ROWS][64], Ps [T][64] (wc: the lane's frequency, clamped)
template <int ROWS>
__device__ __forceinline__ void stage_tables2(cplx* Rs, cplx* Ps, const cplx* phases, const cplx* const* Rtab, int T,
                                              int W, int wc, int lane, int wave, int n_waves) {
    for (int e = wave; e < T*ROWS; e += n_waves) {
        const int k = e / ROWS, r = e % ROWS;
        Rs[static_cast<size_t>(e)*64 + lane] = Rtab[k][static_cast<size_t>(r)*W + wc];
    }
    for (int k = wave; k < T; k += n_waves) Ps[k*64 + lane] = phases[static_cast<size_t>(k)*W + wc];
}

// which selected operator an operator is (-1: none), and its weights at this lane's frequency w (0 beyond W)
template <int A, int S>
__device__ __forceinline__ void select_weights2(const cplx* scale, int s_ndim, int n_spectra, const int32_t* idx,
                                                int n_idx, int sp0, int w, int wc, int W, int (&sel)[A],
                                                double (&wt)[A][S]) {
#pragma unroll
    for (int a = 0; a < A; ++a) {
        sel[a] = selected(idx, n_idx, a);
#pragma unroll
        for (int s = 0; s < S; ++s)
            wt[a][s] = (sel[a] >= 0 && sp0 + s < n_spectra && w < W)
                           ? weight_row(scale, s_ndim, n_idx, sp0 + s, sel[a], W)[wc].re : 0.0;
    }
}

// gate k's rows, their stride and its phase at this lane's frequency: staged, or from L2 (then through vz)
template <int ROWS, bool STAGED>
__device__ __forceinline__ const cplx* gate_rows2(const cplx* Rs, const cplx* const* Rtab, int k, int vz, int lane,
                                                  int wc) {
    return STAGED ? Rs + static_cast<size_t>(k)*ROWS*64 + lane : Rtab[k + vz] + wc;
}
template <bool STAGED>
__device__ __forceinline__ size_t row_stride2(int W, int vz) {
    return STAGED ? 64 : static_cast<size_t>(W + vz);
}
template <bool STAGED>
__device__ __forceinline__ cplx gate_phase2(const cplx* Ps, const cplx* phases, int k, int vz, int W, int lane,
                                            int wc) {
    return STAGED ? Ps[k*64 + lane] : phases[static_cast<size_t>(k + vz)*W + wc];
}

// X += R Lam for operator a's four rows of the gate at Rg, and X = R Lam
__device__ __forceinline__ void add_summand2(const cplx* Rg, int a, size_t rstride, const double (&Lam)[16],
                                             cplx (&X)[4]) {
    constexpr int N = kN2;
#pragma unroll
    for (int kk = 0; kk < N; ++kk) {
        const cplx v = Rg[(a*N + kk)*rstride];
#pragma unroll
        for (int jj = 0; jj < N; ++jj) {
            X[jj].re = fma(v.re, Lam[kk*N + jj], X[jj].re);
            X[jj].im = fma(v.im, Lam[kk*N + jj], X[jj].im);
        }
    }
}
__device__ __forceinline__ void summand2(const cplx* Rg, int a, size_t rstride, const double (&Lam)[16],
                                         cplx (&X)[4]) {
#pragma unroll
    for (int jj = 0; jj < kN2; ++jj) X[jj] = {0.0, 0.0};
    add_summand2(Rg, a, rstride, Lam, X);
}

// Z[k, l] (+)= weight (Re X[k] Re C[l] + Im X[k] Im C[l]) with operator a's C; FRESH: Z is set, not added to
template <bool FRESH, int ROWS>
__device__ __forceinline__ void gram2(double wt, const cplx (&X)[4], const cplx (&C)[ROWS], int a, double (&Z)[16]) {
    constexpr int N = kN2;
#pragma unroll
    for (int kk = 0; kk < N; ++kk) {
        const double xre = wt*X[kk].re, xim = wt*X[kk].im;
#pragma unroll
        for (int l = 0; l < N; ++l) {
            if (FRESH)
                Z[kk*N + l] = fma(xre, C[a*N + l].re, xim*C[a*N + l].im);
            else
                Z[kk*N + l] += fma(xre, C[a*N + l].re, xim*C[a*N + l].im);
        }
    }
}

// C <- conj(p) (C + X) for operator a
template <int ROWS>
__device__ __forceinline__ void fold2(const cplx& ph, const cplx (&X)[4], cplx (&C)[ROWS], int a) {
    constexpr int N = kN2;
#pragma unroll
    for (int jj = 0; jj < N; ++jj) {
        const double sre = C[a*N + jj].re + X[jj].re, sim = C[a*N + jj].im + X[jj].im;
        C[a*N + jj] = {fma(ph.re, sre, ph.im*sim), fma(ph.re, sim, -(ph.im*sre))};
    }
}

// Lam <- L Lam (L the same for every lane: read through a vector register it stays out of the scalar registers,
// which the pointers and counters of the walk fill)
__device__ __forceinline__ void advance2(const double* Lsrc, double (&Lam)[16]) {
    constexpr int N = kN2;
    double Ln[N*N];
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
    for (int e = 0; e < N*N; ++e) Lam[e] = Ln[e];
}

// acc += Lam^T (D Lam), 4 x 4 (D read through a vector register, as L)
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

// ---- d = 4 -------------------------------------------------------------------------------------------------------
// the weights of the block's frequencies [S][A][WT] to LDS (0 beyond W and for what is not selected)
template <int A, int S, int WT>
__device__ __forceinline__ void stage_weights4(double* Ws, const cplx* scale, int s_ndim, int n_spectra,
                                               const int32_t* idx, int n_idx, int sp0, int w0, int W) {
    for (int e = threadIdx.x; e < S*A*WT; e += blockDim.x) {
        const int x = e % WT, a = (e / WT) % A, s = e / (WT*A);
        const int i = selected(idx, n_idx, a);
        Ws[e] = (i >= 0 && sp0 + s < n_spectra && w0 + x < W)
                    ? weight_row(scale, s_ndim, n_idx, sp0 + s, i, W)[w0 + x].re : 0.0;
    }
}

// the tables of the block's frequencies to LDS: Rs [T][ROWS][WT], Ps [T][WT]
template <int ROWS, int WT>
__device__ __forceinline__ void stage_tables4(cplx* Rs, cplx* Ps, const cplx* phases, const cplx* const* Rtab, int T,
                                              int W, int w0, int lane, int wave, int n_waves) {
    const int x = lane % WT, wl = min(w0 + x, W - 1);
    for (int e = wave*(64/WT) + lane/WT; e < T*ROWS; e += n_waves*(64/WT)) {
        const int k = e / ROWS, r = e % ROWS;
        Rs[static_cast<size_t>(e)*WT + x] = Rtab[k][static_cast<size_t>(r)*W + wl];
    }
    for (int k = wave*(64/WT) + lane/WT; k < T; k += n_waves*(64/WT))
        Ps[k*WT + x] = phases[static_cast<size_t>(k)*W + wl];
}

// columns of the table reads: as A operand the frequency is 16 t + c, in a D tile 16 t + q + 4 r (COL: size_t, or
// int where, read from L2, they are live through the whole walk and the epilogue needs the registers)
template <bool STAGED, typename COL, int TILES>
__device__ __forceinline__ void columns4(COL (&colA)[TILES], COL (&colD)[TILES][4], int w0, int W, int c, int q) {
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        colA[t] = COL(STAGED ? 16*t + c : min(w0 + 16*t + c, W - 1));
#pragma unroll
        for (int r = 0; r < 4; ++r) colD[t][r] = COL(STAGED ? 16*t + q + 4*r : min(w0 + 16*t + q + 4*r, W - 1));
    }
}

// gate k's rows, their stride and its phases: staged, or where they lie
template <int ROWS, int WT, bool STAGED>
__device__ __forceinline__ const cplx* gate_rows4(const cplx* Rs, const cplx* const* Rtab, int k) {
    return STAGED ? Rs + static_cast<size_t>(k)*ROWS*WT : Rtab[k];
}
template <int WT, bool STAGED>
__device__ __forceinline__ size_t row_stride4(int W) {
    return STAGED ? WT : static_cast<size_t>(W);
}
template <int WT, bool STAGED>
__device__ __forceinline__ const cplx* gate_phases4(const cplx* Ps, const cplx* phases, int k, int W) {
    return STAGED ? Ps + k*WT : phases + static_cast<size_t>(k)*W;
}
template <typename COL>
__device__ __forceinline__ void load_phases4(const cplx* Pg, const COL (&col)[4], cplx (&ph)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) ph[r] = Pg[col[r]];
}

// X + R Lam for one operator and tile: row = frequency 16 t + q + 4 r, col = basis element c.  Ra: the lane's entry of
// the operator's row q in the tile's A operand column, Rg + (a*N + q)*rstride + colA[t].  (By value: a tile written
// through a reference is promoted to registers only after the loops around it have been transformed, and is then
// carried around them.)
__device__ __forceinline__ tile4 add_summand4(const cplx* Ra, size_t rstride, f64x4 Lam, tile4 X) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const cplx v = Ra[4*s*rstride];
        X.re = __builtin_amdgcn_mfma_f64_16x16x4f64(v.re, Lam[s], X.re, 0, 0, 0);
        X.im = __builtin_amdgcn_mfma_f64_16x16x4f64(v.im, Lam[s], X.im, 0, 0, 0);
    }
    return X;
}

// Z[k, l] += sum_w X[w, k] (weight_w C[w, l]) over the tile's frequencies (wrow: the weights of rows q + 4 r)
__device__ __forceinline__ void gram4(const double* wrow, tile4 X, f64x4 cre, f64x4 cim, f64x4& Zre, f64x4& Zim) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double wt = wrow[4*r];
        Zre = __builtin_amdgcn_mfma_f64_16x16x4f64(X.re[r], wt*cre[r], Zre, 0, 0, 0);
        Zim = __builtin_amdgcn_mfma_f64_16x16x4f64(X.im[r], wt*cim[r], Zim, 0, 0, 0);
    }
}

// C <- conj(p) (C + X), one tile
__device__ __forceinline__ void fold4(const cplx (&ph)[4], tile4 X, f64x4& Cre, f64x4& Cim) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double sre = Cre[r] + X.re[r], sim = Cim[r] + X.im[r];
        Cre[r] = fma(ph[r].re, sre, ph[r].im*sim);
        Cim[r] = fma(ph[r].re, sim, -(ph[r].im*sre));
    }
}

// Zd += Lam^T (D Lam); Dg: the lane's entries of D, D + c*N + q
__device__ __forceinline__ void add_rotated4(const double* Dg, const f64x4& Lam, f64x4& Zd) {
    f64x4 M = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) M = __builtin_amdgcn_mfma_f64_16x16x4f64(Dg[4*r], Lam[r], M, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) Zd = __builtin_amdgcn_mfma_f64_16x16x4f64(Lam[r], M[r], Zd, 0, 0, 0);
}

// Lam <- L Lam; Lsrc: the lane's entries of L, L + c*N + q
__device__ __forceinline__ void advance4(const double* Lsrc, f64x4& Lam) {
    f64x4 Ln = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) Ln = __builtin_amdgcn_mfma_f64_16x16x4f64(Lsrc[4*r], Lam[r], Ln, 0, 0, 0);
    Lam = Ln;
}

// ---- host --------------------------------------------------------------------------------------------------------
inline int block_width(int d, int A) { return d == 2 ? 64 : 16*seq4_tiles(A); }

inline size_t staged2_lds_bytes(int T, int A) { return static_cast<size_t>(T)*(A*kN2 + 1)*64*sizeof(cplx); }
inline size_t staged4_lds_bytes(int T, int A) {
    return static_cast<size_t>(T)*(A*kN + 1)*16*seq4_tiles(A)*sizeof(cplx);
}
inline size_t weights4_lds_bytes(int A, int spectra) {
    return static_cast<size_t>(spectra)*A*16*seq4_tiles(A)*sizeof(double);
}
// the dynamic LDS of a walk, and whether the gates' tables are staged in it (spectra: per walk)
inline size_t walk_lds_bytes(int d, bool staged, int T, int A, int spectra) {
    if (d == 2) return staged ? staged2_lds_bytes(T, A) : 0;
    return (staged ? staged4_lds_bytes(T, A) : 0) + weights4_lds_bytes(A, spectra);
}
inline bool tables_staged(int d, int T, int A, int spectra) {
    return walk_lds_bytes(d, true, T, A, spectra) <= 150*1024;
}

// groups of sequences (grid y): staged, one block per CU; else a few; never more groups than wavefronts' worth of
// sequences
inline int walk_groups(bool staged, int blocks, int walks, int P) {
    long groups = ((staged ? 256L : 1024L) + static_cast<long>(blocks)*walks - 1)/(static_cast<long>(blocks)*walks);
    groups = std::min(groups, (static_cast<long>(P) + kWaves - 1)/kWaves);
    return static_cast<int>(std::max(1L, std::min(groups, 65535L)));
}

// launches a walk kernel with lds bytes of dynamic LDS (above 48 KiB the limit is raised first)
template <typename K, typename... Args>
inline hipError_t launch_walk(K kern, dim3 grid, size_t lds, hipStream_t stream, Args... args) {
    if (lds > 48*1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, grid, dim3(64*kWaves), lds, stream, args...);
    return hipGetLastError();
}

// f(std::integral_constant<int, A>) for A = 1..4: the instantiations of a walk
template <typename F>
inline hipError_t for_operators(int A, F&& f) {
    switch (A) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        default: return hipErrorInvalidValue;
    }
}

}  // namespace seqwalk
}  // namespace ffk

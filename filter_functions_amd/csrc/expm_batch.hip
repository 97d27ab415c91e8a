// expm_batch.hip -- the exponential of MANY independent real N x N matrices, 1 <= N <= 16, each the sum of `rows`
// consecutive input tiles (ffk_expm_real_batch*; ff.exponentiate_cumulant_functions): the error transfer matrices
// exp K after every gate of many sequences in one launch.
//
// The arithmetic plan is launch_expm_real's (decay.hip): the 1-norm, s = expm_squarings(norm), B = A / 2^s (exact),
// the Taylor polynomial of degree 18 the Paterson-Stockmeyer way -- B^2, B^3, B^4 once, then Horner in B^4 over five
// blocks --, then s squarings.  The order of the sums inside a product is this file's own, so the results are not the
// bits of ffk_expm_real; a matrix's result is the same bits at every count, at every place in the batch and in every
// split of it: no value of a matrix meets another matrix's anywhere.
//
// Two kernels, chosen by N alone.
//   N = 4 (one qubit): one LANE per matrix, everything in registers, no LDS, no matrix instruction; every lane has
//     its own norm and its own number of squarings (a divergent trip count).
//   every other N: one WAVEFRONT per matrix on v_mfma_f64_16x16x4_f64, four wavefronts per block, each with its own
//     matrix; the zero-padded tile stays in registers in the instruction's C/D layout
//         col = lane & 15, row = (lane >> 4) + 4 reg.
//     Register r of a tile X in that layout is a legal A fragment (A[i = lane & 15][k = lane >> 4] = X[k + 4 r][i])
//     and register r of Y a legal B fragment (B[k][j] = Y[k + 4 r][j]): the four instructions r = 0..3 on (X, Y)
//     accumulate X^T Y.  Every matrix of the scheme is a polynomial in B, so each is kept as the pair (X, X^T):
//         X Y     = the four instructions on (X^T, Y),
//         (X Y)^T = the four instructions on (Y, X^T),
//     eight matrix instructions per product, no LDS tile, no barrier, nothing transposed; B^T comes from how the
//     input is indexed on load.
#include <cmath>

#include "ffk_internal.h"

namespace ffk {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

struct TaylorCoefficients {
    double c[19];          // 1/k!
};
// c0 I + c1 B + c2 B^2 + c3 B^3
struct Block {
    double c0, c1, c2, c3;
};
__device__ __forceinline__ Block taylor_block(const TaylorCoefficients& co, int j) {      // (j = 4: three terms)
    return Block{co.c[4*j], co.c[4*j + 1], co.c[4*j + 2], 4*j + 3 <= 18 ? co.c[4*j + 3] : 0.0};
}

// ---- N = 4: one lane per matrix --------------------------------------------------------------------------------------
struct M4 {
    double a[16];
};
// z = x y, every entry one chain over k = 0..3
__device__ __forceinline__ M4 mul4(const M4& x, const M4& y) {
    M4 z;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double v = x.a[4*i]*y.a[j];
            v = fma(x.a[4*i + 1], y.a[4 + j], v);
            v = fma(x.a[4*i + 2], y.a[8 + j], v);
            v = fma(x.a[4*i + 3], y.a[12 + j], v);
            z.a[4*i + j] = v;
        }
    return z;
}
// z + c0 I + c1 x1 + c2 x2 + c3 x3
__device__ __forceinline__ M4 add_block4(M4 z, Block p, const M4& x1, const M4& x2, const M4& x3) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        double v = z.a[e];
        if (e % 5 == 0) v += p.c0;
        v = fma(p.c1, x1.a[e], v);
        v = fma(p.c2, x2.a[e], v);
        v = fma(p.c3, x3.a[e], v);
        z.a[e] = v;
    }
    return z;
}

__global__ __launch_bounds__(256) void expm_batch_lane4_kernel(const double* __restrict__ K, long count, int rows,
                                                               TaylorCoefficients co, double* __restrict__ out,
                                                               int32_t* __restrict__ not_finite) {
    const long m = static_cast<long>(blockIdx.x)*256 + threadIdx.x;
    if (m >= count) return;
    const double* Kp = K + static_cast<size_t>(m)*rows*16;
    M4 A;
#pragma unroll
    for (int e = 0; e < 16; ++e) A.a[e] = Kp[e];
    for (int q = 1; q < rows; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) A.a[e] += Kp[static_cast<size_t>(q)*16 + e];
    bool bad = false;
#pragma unroll
    for (int e = 0; e < 16; ++e) bad |= !(A.a[e] - A.a[e] == 0.0);
    not_finite[m] = bad ? 1 : 0;
    if (bad) return;
    // |A|_1: the largest column sum of absolute values, every column added down its rows
    double norm = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double column = ((fabs(A.a[j]) + fabs(A.a[4 + j])) + fabs(A.a[8 + j])) + fabs(A.a[12 + j]);
        norm = column > norm ? column : norm;
    }
    const int squarings = expm_squarings(norm);
    const double scale = ldexp(1.0, -squarings);
    M4 B;
#pragma unroll
    for (int e = 0; e < 16; ++e) B.a[e] = scale*A.a[e];
    const M4 X2 = mul4(B, B);
    const M4 X3 = mul4(X2, B);
    const M4 X4 = mul4(X2, X2);
    // S = P_4;  S <- S X4 + P_j, j = 3 .. 0, then the squarings
    M4 S;
#pragma unroll
    for (int e = 0; e < 16; ++e) S.a[e] = 0.0;
    S = add_block4(S, taylor_block(co, 4), B, X2, X3);
#pragma unroll
    for (int j = 3; j >= 0; --j) S = add_block4(mul4(S, X4), taylor_block(co, j), B, X2, X3);
    for (int q = 0; q < squarings; ++q) S = mul4(S, S);
    double* o = out + static_cast<size_t>(m)*16;
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = S.a[e];
}

// ---- every other N <= 16: one wavefront per matrix -------------------------------------------------------------------
// X and X^T, both in the C/D layout
struct Pair {
    f64x4 m, t;
};
// P^T Q of two tiles in the C/D layout: register r of P as the A operand, register r of Q as the B operand
__device__ __forceinline__ f64x4 mfma_tn(f64x4 P, f64x4 Q) {
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(P[r], Q[r], acc, 0, 0, 0);
    return acc;
}
// X Y and its transpose
__device__ __forceinline__ Pair product(const Pair& X, const Pair& Y) {
    return Pair{mfma_tn(X.t, Y.m), mfma_tn(Y.m, X.t)};
}
// Z + c0 I + c1 X1 + c2 X2 + c3 X3 on both halves; the padding stays zero
__device__ __forceinline__ Pair add_block(Pair Z, Block p, const Pair& X1, const Pair& X2, const Pair& X3, int N,
                                          int lane) {
    const int l15 = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lk + 4*r;
        const bool inside = i < N && l15 < N;
        double v = Z.m[r], w = Z.t[r];
        if (i == l15) {
            v += p.c0;
            w += p.c0;
        }
        v = fma(p.c1, X1.m[r], v);
        w = fma(p.c1, X1.t[r], w);
        v = fma(p.c2, X2.m[r], v);
        w = fma(p.c2, X2.t[r], w);
        v = fma(p.c3, X3.m[r], v);
        w = fma(p.c3, X3.t[r], w);
        Z.m[r] = inside ? v : 0.0;
        Z.t[r] = inside ? w : 0.0;
    }
    return Z;
}

__global__ __launch_bounds__(256) void expm_batch_wave_kernel(const double* __restrict__ K, long count, int rows,
                                                              int N, TaylorCoefficients co, double* __restrict__ out,
                                                              int32_t* __restrict__ not_finite) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const long m = static_cast<long>(blockIdx.x)*4 + wave;
    if (m >= count) return;          // (a whole wavefront: the block has no barrier)
    const int l15 = lane & 15, lk = lane >> 4;
    const size_t nn = static_cast<size_t>(N)*N;
    const double* Kp = K + static_cast<size_t>(m)*rows*nn;
    // the sum over the rows in order, as A (row = lk + 4 r, column = l15) and, indexed the other way, as A^T
    Pair A;
    bool bad = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lk + 4*r;
        double v = 0.0, w = 0.0;
        if (i < N && l15 < N) {
            const double* a = Kp + i*N + l15;
            const double* at = Kp + l15*N + i;
            v = a[0];
            w = at[0];
            for (int q = 1; q < rows; ++q) {
                v += a[q*nn];
                w += at[q*nn];
            }
        }
        bad |= !(v - v == 0.0);
        A.m[r] = v;
        A.t[r] = w;
    }
    const bool any_bad = __builtin_amdgcn_ballot_w64(bad) != 0ull;
    if (lane == 0) not_finite[m] = any_bad ? 1 : 0;
    if (any_bad) return;
    // |A|_1: a column is a lane's four registers and the lanes 16, 32 and 48 above it; then the largest of sixteen
    double column = ((fabs(A.m[0]) + fabs(A.m[1])) + fabs(A.m[2])) + fabs(A.m[3]);
    column += __shfl_xor(column, 16);
    column += __shfl_xor(column, 32);
    double norm = column;
#pragma unroll
    for (int step = 1; step < 16; step <<= 1) {
        const double other = __shfl_xor(norm, step);
        norm = other > norm ? other : norm;
    }
    // (every lane holds the same norm; as a scalar the trip count of the squarings is the wavefront's)
    const int squarings = __builtin_amdgcn_readfirstlane(expm_squarings(norm));
    const double scale = ldexp(1.0, -squarings);
    Pair B;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        B.m[r] = scale*A.m[r];
        B.t[r] = scale*A.t[r];
    }
    const Pair X2 = product(B, B);
    const Pair X3 = product(X2, B);
    const Pair X4 = product(X2, X2);
    // S = P_4;  S <- S X4 + P_j, j = 3 .. 0, then the squarings
    const f64x4 zero = {0.0, 0.0, 0.0, 0.0};
    Pair S = add_block(Pair{zero, zero}, taylor_block(co, 4), B, X2, X3, N, lane);
#pragma unroll
    for (int j = 3; j >= 0; --j) S = add_block(product(S, X4), taylor_block(co, j), B, X2, X3, N, lane);
    for (int q = 0; q < squarings; ++q) S = product(S, S);
    if (l15 >= N) return;
    double* o = out + static_cast<size_t>(m)*nn;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lk + 4*r;
        if (i < N) o[i*N + l15] = S.m[r];
    }
}

}  // namespace

hipError_t launch_expm_batch(const double* tiles, long count, int rows, int N, double* out, int32_t* not_finite,
                             hipStream_t stream) {
    if (count < 0 || rows < 1 || N < 1 || N > 16) return hipErrorInvalidValue;
    TaylorCoefficients co;
    co.c[0] = 1.0;
    for (int k = 1; k <= 18; ++k) co.c[k] = co.c[k - 1]/k;
    const size_t nn = static_cast<size_t>(N)*N;
    // (a launch takes 2^28 matrices: the grid stays far below its limit at both block shapes)
    const long slab = 1L << 28;
    for (long at = 0; at < count; at += slab) {
        const long n = count - at < slab ? count - at : slab;
        const double* in = tiles + static_cast<size_t>(at)*rows*nn;
        if (N == 4)
            hipLaunchKernelGGL(expm_batch_lane4_kernel, dim3(static_cast<unsigned>((n + 255)/256)), dim3(256), 0,
                               stream, in, n, rows, co, out + static_cast<size_t>(at)*nn, not_finite + at);
        else
            hipLaunchKernelGGL(expm_batch_wave_kernel, dim3(static_cast<unsigned>((n + 3)/4)), dim3(256), 0, stream,
                               in, n, rows, N, co, out + static_cast<size_t>(at)*nn, not_finite + at);
    }
    return hipGetLastError();
}

}  // namespace ffk

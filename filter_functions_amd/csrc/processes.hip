// processes.hip -- decay amplitudes, cumulant functions and error transfer matrices of MANY independent pulses
// whose control matrices already lie in HBM (ffk_resident_batch_processes; SURVEY 8f.2 over a pulse axis).
//
//   Gamma[p,a(,b),k,l] = sum_w c_w Re( conj R[p,a,k,w] S_ab(w) R[p,b,l,w] ),   N <= 16 basis elements,
// c_w the trapezoid weights / 2 pi (launch_spectral_weights).  R comes through a table of P device pointers: the
// members of batched and sequence passes, single resident results and uploaded host rows are read where they lie.
// As in decay.hip the integral is a real matrix product over the 2 W interleaved reals of a row on
// v_mfma_f64_16x16x4_f64, and a 16 x 16 output is exactly one tile: ONE wavefront per (pulse, operator pair,
// frequency chunk) reads its 16 rows once -- for a spectrum of one or two dimensions both operands are the same
// rows, so every byte of R is fetched once -- and nothing else of size.  The frequency axis is cut into chunks
// whose length depends on W alone (never on P: a pulse's result must not depend on its batch); the partial tiles
// are added in chunk order by a second launch.
//
// The cumulant function is launch_cumulant_function (decay.hip) with batch = P rows.  The sum over the noise
// operators, the 1-norm, the choice of the squarings and exp(K) run in one wavefront per pulse, with the
// arithmetic of launch_expm_real (same Taylor polynomial, same products, same order) on one zero-padded tile.
#include <cmath>
#include <type_traits>

#include "ffk_internal.h"

namespace ffk {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kStep = 32;          // frequencies per step of a wavefront: 8 consecutive ones per lane group

// One wavefront: the 16 x 16 tile of Gamma[p, pair] over the chunk blockIdx.z.  MFMA operand maps as in
// decay_gemm_kernel: A[i = lane & 15][k = lane >> 4], B[k][j = lane & 15], D[row = (lane >> 4) + 4 r][col].
// REAL_W: the weights are real (two products per entry instead of a complex one); PAIR: the right operand is
// another operator's rows (a spectrum of three dimensions).
template <bool REAL_W, bool PAIR>
__global__ __launch_bounds__(64) void processes_decay_kernel(
    const cplx* const* __restrict__ Rtab, int N, int W, const cplx* __restrict__ scale, int s_ndim,
    const int32_t* __restrict__ idx, int n_idx, int chunk, int symmetric, double* __restrict__ out,
    size_t split_stride) {
    __shared__ double tile[16][17];
    const int lane = threadIdx.x;
    const int l15 = lane & 15, lk = lane >> 4;
    const int pair = blockIdx.x, p = blockIdx.y, split = blockIdx.z;
    const int ia = s_ndim == 3 ? pair / n_idx : pair;
    const int ib = s_ndim == 3 ? pair % n_idx : pair;
    const cplx* sp = scale + static_cast<size_t>(s_ndim == 1 ? 0 : pair)*W;
    const cplx* Rp = Rtab[p];
    const int row = min(N - 1, l15);          // (lanes beyond N repeat the last row; their results are not stored)
    const cplx* La = Rp + (static_cast<size_t>(idx[ia])*N + row)*W;
    const cplx* Lb = PAIR ? Rp + (static_cast<size_t>(idx[ib])*N + row)*W : La;
    const int wbeg = split*chunk;
    const int wend = min(W, wbeg + chunk);

    struct Weight {          // (real weights: the real part alone is fetched and kept)
        double re, im;
    };
    struct RealWeight {
        double re;
    };
    using weight_t = typename std::conditional<REAL_W, RealWeight, Weight>::type;
    auto weight = [&](int w) {
        weight_t s;
        s.re = sp[w].re;
        if constexpr (!REAL_W) s.im = sp[w].im;
        return s;
    };
    struct Frag {
        cplx a[8], b[PAIR ? 8 : 1];
        weight_t s[8];
    };
    auto load = [&](Frag& f, int w0) {
        const int w = w0 + 8*lk;
        if (w0 + kStep <= wend) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                f.a[c] = La[w + c];
                if (PAIR) f.b[c] = Lb[w + c];
                f.s[c] = weight(w + c);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const bool ok = w + c < wend;
                const int wc = ok ? w + c : wend - 1;
                f.a[c] = La[wc];
                if (PAIR) f.b[c] = Lb[wc];
                f.s[c] = weight(wc);
                if (!ok) f.s[c] = weight_t{};
            }
        }
    };
    // real and imaginary parts go to accumulators of their own: consecutive matrix instructions never share one
    f64x4 acc_re = {0.0, 0.0, 0.0, 0.0}, acc_im = {0.0, 0.0, 0.0, 0.0};
    Frag cur, nxt;
    load(cur, wbeg);
    for (int w0 = wbeg; w0 < wend; w0 += kStep) {
        // the next step's rows are requested before this step's products
        const bool more = w0 + kStep < wend;
        if (more) load(nxt, w0 + kStep);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const cplx a = cur.a[c];
            const cplx y = PAIR ? cur.b[PAIR ? c : 0] : a;
            cplx b;
            if constexpr (REAL_W) b = {cur.s[c].re*y.re, cur.s[c].re*y.im};
            else b = cmul(cplx{cur.s[c].re, cur.s[c].im}, y);
            acc_re = __builtin_amdgcn_mfma_f64_16x16x4f64(a.re, b.re, acc_re, 0, 0, 0);
            acc_im = __builtin_amdgcn_mfma_f64_16x16x4f64(a.im, b.im, acc_im, 0, 0, 0);
        }
        if (more) cur = nxt;
    }
    f64x4 acc = acc_re + acc_im;
    if (symmetric) {
        // real weights, one operator with itself: Gamma is symmetric in (k, l); the entries below the diagonal are
        // those above it (the sums of a chunk's partial tiles are then symmetric bit for bit as well)
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[lk + 4*r][l15] = acc[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (lk + 4*r > l15) acc[r] = tile[l15][lk + 4*r];
    }
    if (l15 >= N) return;
    double* o = out + static_cast<size_t>(split)*split_stride +
                (static_cast<size_t>(p)*gridDim.x + pair)*N*N;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lk + 4*r;
        if (i < N) o[i*N + l15] = acc[r];
    }
}

// out[i] = sum_s part[s][i], the chunks in order
__global__ __launch_bounds__(256) void processes_reduce_kernel(const double* __restrict__ part, int nsplit, size_t n,
                                                               double* __restrict__ out) {
    const size_t i = static_cast<size_t>(blockIdx.x)*256 + threadIdx.x;
    if (i >= n) return;
    double acc = part[i];
    for (int s = 1; s < nsplit; ++s) acc += part[static_cast<size_t>(s)*n + i];
    out[i] = acc;
}

struct TaylorCoefficients {
    double c[19];          // 1/k!
};
struct PolyTerms16 {
    double c0, c1, c2, c3;
};
using Tile = double[16][17];

// C = alpha A B + c0 I + c1 X1 + c2 X2 + c3 X3 on zero-padded 16 x 16 tiles in LDS: the arithmetic of
// dgemm_poly_kernel (decay.hip) for N <= 16, where one step of the k loop holds the whole product -- four matrix
// instructions with k = 4 (lane >> 4) + j, j = 0..3 -- and the other three wavefronts of its block add zeros.
__device__ __forceinline__ void poly_product16(const Tile& A, const Tile& B, int N, double alpha, PolyTerms16 p,
                                               const Tile& X1, const Tile& X2, const Tile& X3, Tile& C, int lane) {
    const int l15 = lane & 15, lk = lane >> 4;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    if (alpha != 0.0) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[l15][4*lk + j], B[4*lk + j][l15], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = acc[r] + 0.0;      // (the partial tiles of the idle wavefronts)
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lk + 4*r;
        double v = alpha*acc[r];
        if (i == l15) v += p.c0;
        if (p.c1 != 0.0) v = fma(p.c1, X1[i][l15], v);
        if (p.c2 != 0.0) v = fma(p.c2, X2[i][l15], v);
        if (p.c3 != 0.0) v = fma(p.c3, X3[i][l15], v);
        C[i][l15] = (i < N && l15 < N) ? v : 0.0;
    }
    __syncthreads();
}

// One wavefront per pulse: K summed over its rows (in order, as NumPy's sum over the leading axes), the 1-norm,
// the squarings of expm_squarings, the degree-18 Taylor polynomial of launch_expm_real and the squarings.  A sum
// with a NaN or Inf sets not_finite[p] and writes nothing else.
__global__ __launch_bounds__(64) void processes_expm_kernel(const double* __restrict__ K, int rows, int N,
                                                            TaylorCoefficients co, double* __restrict__ out,
                                                            int32_t* __restrict__ not_finite) {
    __shared__ Tile M[7];
    __shared__ double colsum[16];
    const int lane = threadIdx.x;
    const int l15 = lane & 15, lk = lane >> 4;
    const size_t nn = static_cast<size_t>(N)*N;
    const double* Kp = K + static_cast<size_t>(blockIdx.x)*rows*nn;
    bool bad = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lk + 4*r;
        double v = 0.0;
        if (i < N && l15 < N) {
            v = Kp[i*N + l15];
            for (int q = 1; q < rows; ++q) v += Kp[q*nn + i*N + l15];
        }
        bad |= !(v - v == 0.0);
        M[0][i][l15] = v;
    }
    const bool any_bad = __builtin_amdgcn_ballot_w64(bad) != 0ull;
    if (lane == 0) not_finite[blockIdx.x] = any_bad ? 1 : 0;
    if (any_bad) return;
    __syncthreads();
    // |A|_1: the largest column sum of absolute values, every column added down its rows
    if (lane < 16) {
        double column = 0.0;
        for (int i = 0; i < N; ++i) column += fabs(M[0][i][lane]);
        colsum[lane] = column;
    }
    __syncthreads();
    double norm = 0.0;
    for (int j = 0; j < N; ++j) norm = colsum[j] > norm ? colsum[j] : norm;
    const int squarings = expm_squarings(norm);
    const double scale = ldexp(1.0, -squarings);

    Tile &A = M[0], &X1 = M[1], &X2 = M[2], &X3 = M[3], &X4 = M[4];
    const PolyTerms16 none = {0.0, 0.0, 0.0, 0.0};
    // X1 = B = scale A (as a linear combination: no product), X2 = B B, X3 = X2 B, X4 = X2 X2
    poly_product16(A, A, N, 0.0, PolyTerms16{0.0, scale, 0.0, 0.0}, A, A, A, X1, lane);
    poly_product16(X1, X1, N, 1.0, none, X1, X2, X3, X2, lane);
    poly_product16(X2, X1, N, 1.0, none, X1, X2, X3, X3, lane);
    poly_product16(X2, X2, N, 1.0, none, X1, X2, X3, X4, lane);
    auto block = [&](int j) {             // P_j = sum_{i<4} c[4j+i] B^i  (j = 4: three terms)
        return PolyTerms16{co.c[4*j], co.c[4*j + 1], co.c[4*j + 2], 4*j + 3 <= 18 ? co.c[4*j + 3] : 0.0};
    };
    // S = P_4;  S <- S X4 + P_j, j = 3 .. 0, then the squarings (ping-pong between two tiles)
    int cur = 5, nxt = 6;
    poly_product16(X1, X1, N, 0.0, block(4), X1, X2, X3, M[cur], lane);
    for (int j = 3; j >= 0; --j) {
        poly_product16(M[cur], X4, N, 1.0, block(j), X1, X2, X3, M[nxt], lane);
        const int t = cur; cur = nxt; nxt = t;
    }
    for (int q = 0; q < squarings; ++q) {
        poly_product16(M[cur], M[cur], N, 1.0, none, X1, X2, X3, M[nxt], lane);
        const int t = cur; cur = nxt; nxt = t;
    }
    if (l15 >= N) return;
    double* o = out + static_cast<size_t>(blockIdx.x)*nn;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lk + 4*r;
        if (i < N) o[i*N + l15] = M[cur][i][l15];
    }
}

}  // namespace

int processes_decay_chunks(int W, int* chunk) {
    // chunks of about 256 frequencies (a wavefront then reads 64 KiB at N = 16), whole steps, 64 at most
    int n = (W + 255)/256;
    n = n < 1 ? 1 : (n > 64 ? 64 : n);
    const int len = ((W + n - 1)/n + kStep - 1)/kStep*kStep;
    if (chunk) *chunk = len;
    return W < 1 ? 1 : (W + len - 1)/len;
}

hipError_t launch_processes_decay(const cplx* const* Rtab, int P, int N, int W, const cplx* scale, int s_ndim,
                                  int complex_weights, const int32_t* idx, int n_idx, double* gamma,
                                  double* partials, hipStream_t stream) {
    if (P < 1 || P > 65535 || N < 1 || N > 16 || W < 1 || n_idx < 1 || s_ndim < 1 || s_ndim > 3)
        return hipErrorInvalidValue;
    int chunk = 0;
    const int nsplit = processes_decay_chunks(W, &chunk);
    const int pairs = s_ndim == 3 ? n_idx*n_idx : n_idx;
    const size_t n = static_cast<size_t>(P)*pairs*N*N;
    if (nsplit > 1 && !partials) return hipErrorInvalidValue;
    double* dst = nsplit > 1 ? partials : gamma;
    const dim3 grid(pairs, P, nsplit);
    const int symmetric = s_ndim != 3 && !complex_weights;
#define FFK_PROC_LAUNCH(REAL_W, PAIR) \
    hipLaunchKernelGGL((processes_decay_kernel<REAL_W, PAIR>), grid, dim3(64), 0, stream, Rtab, N, W, scale, \
                       s_ndim, idx, n_idx, chunk, symmetric, dst, n)
    if (s_ndim == 3)
        FFK_PROC_LAUNCH(false, true);
    else if (complex_weights)
        FFK_PROC_LAUNCH(false, false);
    else
        FFK_PROC_LAUNCH(true, false);
#undef FFK_PROC_LAUNCH
    if (nsplit > 1)
        hipLaunchKernelGGL(processes_reduce_kernel, dim3(static_cast<unsigned>((n + 255)/256)), dim3(256), 0, stream,
                           partials, nsplit, n, gamma);
    return hipGetLastError();
}

hipError_t launch_processes_expm(const double* K, int P, int rows, int N, double* out, int32_t* not_finite,
                                 hipStream_t stream) {
    if (P < 1 || rows < 1 || N < 1 || N > 16) return hipErrorInvalidValue;
    TaylorCoefficients co;
    co.c[0] = 1.0;
    for (int k = 1; k <= 18; ++k) co.c[k] = co.c[k - 1]/k;
    hipLaunchKernelGGL(processes_expm_kernel, dim3(P), dim3(64), 0, stream, K, rows, N, co, out, not_finite);
    return hipGetLastError();
}

}  // namespace ffk

// periodic_batch.hip -- periodic driving of MANY pulses at MANY repeat counts in one pass (ff.periodic_*,
// ffk_periodic_dev / ffk_resident_periodic).
//
// One period of pulse p: control matrix R1 (A, N = d^2, W), total propagator U = V diag(e^{i phi_j}) V^dag (V unitary,
// found on the host), duration T.  With X(w) = sum_l R1[a,l,w] C_l and X' = V^dag X V the control matrix of n periods
// is element-wise in U's eigenbasis,
//     X'_n[j,k] = X'[j,k] s_jk(w, n),   s = sum_{g<n} e^{i g theta} = e^{i (n-1) theta/2} sin(n theta/2)/sin(theta/2),
//     theta_jk = fl(w T) - (phi_j - phi_k), reduced to [-pi, pi],
// so the repeat count is the argument of a sine, not a number of passes:
//     F_n[a](w) = sum_jk |X'[j,k]|^2 sin^2(n theta_jk/2)/sin^2(theta_jk/2)                    (periodic_fejer_kernel)
//     Gamma_n[a,k,l] = Re sum_{e,f} conj(E[e,k]) G'[e,f] E[f,l],  G'[e,f] = sum_w c_w conj(Y_e) Y_f,  Y = X' s,
//     E[(j,m), l] = (V^dag C_l V)[m, j]                                                       (periodic_decay_kernel)
// The rotation is folded into the basis once per block: C'_l = V^dag C_l V, X'[j,k] = sum_l R1[a,l] C'_l[j,k].
// Pulse, selected operator and repeat count are grid axes: two launches at most per pass whatever P and K.  Every sum
// over the frequencies has an order that depends on W alone, so a result does not depend on what else is in the pass.
#include "ffk_internal.h"

namespace ffk {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kThreads = 256;
constexpr int kRepeatChunk = 8;      // repeat counts of one block of the Fejer kernel
constexpr int kChunk = 64;           // frequencies of one step of the decay kernel
constexpr int kPad = kChunk + 1;

// an unevaluated sum hi + lo of two doubles
struct HalfAngle {
    double hi, lo;
};

// x - 2 pi round(x / 2 pi) as hi + lo: the product k 2 pi_head with its rounding error (fma), whose subtraction from
// x is exact (Sterbenz: x lies within a factor of two of it), then the middle and low parts of 2 pi -- the
// three-term constants of sincos_pi (pi/2 = P1 + P2 + P3), times four
__device__ __forceinline__ HalfAngle reduce_two_pi(double x) {
    const double k = rint(x*1.59154943091895345554e-01);
    const double p = k*(4.0*1.57079632679489655800e+00);
    const double pe = fma(k, 4.0*1.57079632679489655800e+00, -p);
    const double s = x - p;
    double lo = fma(-k, 4.0*6.12323399573676603587e-17, -pe);
    lo = fma(-k, 4.0*(-1.49738490485916983294e-33), lo);
    const double hi = s + lo;
    return {hi, lo - (hi - s)};
}

// r in [-pi, pi] (the reduced fl(w T)), delta = phi_j - phi_k in (-2 pi, 2 pi), both as hi + lo: theta/2 with
// theta = r - delta brought back to [-pi, pi], the rounding error of the difference kept (two-sum; the subtraction
// of 2 pi's head is exact)
__device__ __forceinline__ HalfAngle half_angle(HalfAngle r, double delta_hi, double delta_lo) {
    const double s = r.hi - delta_hi;
    const double bb = s - r.hi;
    double e = (r.hi - (s - bb)) + (-delta_hi - bb);
    e += r.lo - delta_lo;
    const double m = rint(s*1.59154943091895345554e-01);
    const double t = fma(-m, 6.28318530717958623200e+00, s);
    e = fma(-m, 2.44929359829470641435e-16, e);
    const double hi = t + e;
    const double lo = e - (hi - t);
    return {0.5*hi, 0.5*lo};
}

// sin and cos of n (hi + lo): the product n hi with its rounding error (fma), the head through sincos_pi's
// reduction (good to ~2^50), the tail to first order
template <bool PIN>
__device__ __forceinline__ void sincos_multiple(double n, HalfAngle h, double* s, double* c) {
    const double p = n*h.hi;
    const double pe = fma(n, h.hi, -p) + n*h.lo;
    double s0, c0;
    sincos_pi<PIN>(p, &s0, &c0);
    *s = fma(pe, c0, s0);
    *c = fma(-pe, s0, c0);
}

// s_jk(w, n) of one entry: (cos + i sin)((n - 1) theta/2) sin(n theta/2)/sin(theta/2); n where the sine vanishes
__device__ __forceinline__ cplx dirichlet_factor(HalfAngle h, double n) {
    double s1, c1, sn, cn;
    sincos_multiple<true>(1.0, h, &s1, &c1);
    sincos_multiple<true>(n, h, &sn, &cn);
    const double ratio = s1 == 0.0 ? n : sn/s1;
    // e^{i (n-1) h} = e^{i n h} e^{-i h}
    return {ratio*fma(cn, c1, sn*s1), ratio*fma(sn, c1, -(cn*s1))};
}

// C'[l][j d + k] = (V^dag C_l V)[j, k] of the block's pulse into LDS, and dphi[j d + k] = phi_j - phi_k (hi, lo)
template <int D, int THREADS>
__device__ __forceinline__ void rotate_basis(const cplx* __restrict__ basis, const cplx* __restrict__ V,
                                             const double* __restrict__ dphase, cplx* Cp, double* dphi) {
    constexpr int DD = D*D;
    for (int item = threadIdx.x; item < DD*DD; item += THREADS) {
        const int l = item / DD, j = (item % DD) / D, k = item % D;
        cplx acc = {0.0, 0.0};
#pragma unroll
        for (int a = 0; a < D; ++a) {
            cplx row = {0.0, 0.0};
#pragma unroll
            for (int b = 0; b < D; ++b) cmac(row, basis[l*DD + a*D + b], V[b*D + k]);
            cmac_conj(acc, V[a*D + j], row);
        }
        Cp[item] = acc;
    }
    if (threadIdx.x < 2*DD) dphi[threadIdx.x] = dphase[threadIdx.x];
}

// ---- filter functions and infidelities --------------------------------------------------------------------------
// Block = one wavefront: (selected operator i, chunk of kRepeatChunk repeat counts, pulse p), lane = frequency
// (strides of 64).  Per frequency once: X' (d^2 complex in registers), then per term -- term 0 the diagonal, which
// shares theta = w T and has one weight, terms 1 .. d (d - 1) the pairs j != k -- the weight |X'_jk|^2, the half
// angle and 1/sin(theta/2), parked in LDS (a lane's column), so that the loop over the repeat counts walks the terms
// with one sine each and a handful of registers.  F (P, K, n_ops, W) is written only if asked for; the integral
// against the weighted spectrum is summed over the wavefront with a fixed butterfly and over the strides in stride
// order: an order that depends on W alone.
template <int D>
__global__ __launch_bounds__(64) void periodic_fejer_kernel(
    const cplx* const* __restrict__ Rtab, const cplx* __restrict__ basis, const cplx* __restrict__ Vall,
    const double* __restrict__ phiall, const double* __restrict__ period, const double* __restrict__ omega, int W,
    const int32_t* __restrict__ repeats, int K, const int32_t* __restrict__ ops, int n_ops,
    const cplx* __restrict__ scale, int s_ndim, double inv_d, double* __restrict__ F, double* __restrict__ infid) {
    constexpr int DD = D*D, TERMS = D*(D - 1) + 1;
    __shared__ cplx Cp[DD*DD];
    __shared__ double dphi[2*DD];
    __shared__ double term[TERMS][4][64];      // weight, half angle (hi, lo), 1/sin(half angle) or 0
    __shared__ double sums[kRepeatChunk];
    const int i = blockIdx.x, p = blockIdx.z;
    const int k0 = blockIdx.y*kRepeatChunk, kc = min(kRepeatChunk, K - k0);
    const int lane = threadIdx.x;
    rotate_basis<D, 64>(basis, Vall + static_cast<size_t>(p)*DD, phiall + static_cast<size_t>(p)*2*DD, Cp, dphi);
    if (lane < kRepeatChunk) sums[lane] = 0.0;
    __syncthreads();
    const double T = period[p];
    const cplx* R = Rtab[p] + static_cast<size_t>(ops[i])*DD*W;
    const cplx* sc = scale ? scale + static_cast<size_t>(s_ndim == 1 ? 0 : i)*W : nullptr;
#pragma unroll 1
    for (int w0 = 0; w0 < W; w0 += 64) {
        const int w = w0 + lane;
        const bool valid = w < W;
        const int wc = valid ? w : W - 1;
        {
            cplx X[DD];
#pragma unroll
            for (int e = 0; e < DD; ++e) X[e] = {0.0, 0.0};
#pragma unroll 1
            for (int l = 0; l < DD; ++l) {
                const cplx r = R[static_cast<size_t>(l)*W + wc];
#pragma unroll
                for (int e = 0; e < DD; ++e) cmac(X[e], r, Cp[l*DD + e]);
            }
            const HalfAngle x = reduce_two_pi(omega[wc]*T);      // fl(w T), as every route forms it
            double diagonal = 0.0;
            int o = 1;
#pragma unroll
            for (int j = 0; j < D; ++j)
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const cplx v = X[j*D + k];
                    const double a2 = fma(v.re, v.re, v.im*v.im);
                    if (j == k) {
                        diagonal += a2;
                    } else {
                        const HalfAngle h = half_angle(x, dphi[2*(j*D + k)], dphi[2*(j*D + k) + 1]);
                        term[o][0][lane] = a2;
                        term[o][1][lane] = h.hi;
                        term[o][2][lane] = h.lo;
                        ++o;
                    }
                }
            const HalfAngle h = half_angle(x, 0.0, 0.0);
            term[0][0][lane] = diagonal;
            term[0][1][lane] = h.hi;
            term[0][2][lane] = h.lo;
        }
#pragma unroll 1
        for (int o = 0; o < TERMS; ++o) {
            double s1, c1;
            sincos_multiple<false>(1.0, HalfAngle{term[o][1][lane], term[o][2][lane]}, &s1, &c1);
            term[o][3][lane] = s1 == 0.0 ? 0.0 : 1.0/s1;
        }
        const double weight = (sc && valid) ? sc[wc].re : 0.0;
#pragma unroll 1
        for (int q = 0; q < kc; ++q) {
            const double n = static_cast<double>(repeats[k0 + q]);
            double f = 0.0;
#pragma unroll 1
            for (int o = 0; o < TERMS; ++o) {
                double sn, cn;
                sincos_multiple<false>(n, HalfAngle{term[o][1][lane], term[o][2][lane]}, &sn, &cn);
                const double rs = term[o][3][lane];
                const double ratio = rs == 0.0 ? n : sn*rs;
                f = fma(term[o][0][lane], ratio*ratio, f);
            }
            if (F && valid) F[((static_cast<size_t>(p)*K + k0 + q)*n_ops + i)*W + w] = f;
            if (infid) {
                double v = weight*f;
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
                if (lane == 0) sums[q] += v;      // (the strides in order)
            }
        }
    }
    if (!infid) return;
    __syncthreads();
    if (lane < kc) infid[(static_cast<size_t>(p)*K + k0 + lane)*n_ops + i] = sums[lane]*inv_d;
}

// ---- decay amplitudes -------------------------------------------------------------------------------------------
// Block (selected operator i, repeat count, pulse p), four wavefronts.  Steps of 64 frequencies: wavefront g fills
// Y[e][w] = X'_e(w) s_e(w, n) for the entries e = g, g + 4, ... (lane = frequency) into LDS; then the Gram matrix
// G'[e][f] += sum_w c_w conj(Y_e) Y_f of the step --
//   d = 4: on v_mfma_f64_16x16x4_f64 (A[i = lane & 15][k = lane >> 4], B[k][j = lane & 15], D[row = (lane >> 4) + 4 r]
//          [col] in register r), wavefront g the frequencies 16 g .. 16 g + 15 of the step in four K-steps, real and
//          imaginary parts as real products: Re = Yr^T c Yr + Yi^T c Yi, Im = M - M^T with M = Yr^T c Yi; the four
//          wavefronts' tiles are added in index order after the last step;
//   d = 2, 3: thread (e, f), e <= f, vector FMAs over the 64 frequencies in order.
// G' is completed Hermitian from e <= f; then T = G' E and Gamma[k,l] = Re sum_e conj(E[e,k]) T[e,l] for k <= l,
// mirrored: symmetric bit for bit.
template <int D>
__global__ __launch_bounds__(kThreads) void periodic_decay_kernel(
    const cplx* const* __restrict__ Rtab, const cplx* __restrict__ basis, const cplx* __restrict__ Vall,
    const double* __restrict__ phiall, const double* __restrict__ period, const double* __restrict__ omega, int W,
    const int32_t* __restrict__ repeats, int K, const int32_t* __restrict__ ops, int n_ops,
    const cplx* __restrict__ scale, int s_ndim, double* __restrict__ gamma) {
    constexpr int DD = D*D, PER = (DD + 3)/4;
    __shared__ cplx Cp[DD*DD];
    __shared__ double dphi[2*DD];
    __shared__ double Yr[DD*kPad], Yi[DD*kPad], cw[kChunk];
    __shared__ cplx G[DD*DD], Tm[DD*DD];
    __shared__ double part[D == 4 ? 4*3*16*17 : 1];
    const int i = blockIdx.x, q = blockIdx.y, p = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    rotate_basis<D, kThreads>(basis, Vall + static_cast<size_t>(p)*DD, phiall + static_cast<size_t>(p)*2*DD, Cp, dphi);
    __syncthreads();
    const double T = period[p], n = static_cast<double>(repeats[q]);
    const cplx* R = Rtab[p] + static_cast<size_t>(ops[i])*DD*W;
    const cplx* sc = scale + static_cast<size_t>(s_ndim == 1 ? 0 : i)*W;
    // the thread's Gram entry (d = 2, 3) or the wavefront's tiles (d = 4)
    const int ge = threadIdx.x / DD, gf = threadIdx.x % DD;
    cplx acc = {0.0, 0.0};
    f64x4 acc_rr = {0.0, 0.0, 0.0, 0.0}, acc_ii = {0.0, 0.0, 0.0, 0.0}, acc_ri = {0.0, 0.0, 0.0, 0.0};
    for (int w0 = 0; w0 < W; w0 += kChunk) {
        const int w = w0 + lane;
        const bool valid = w < W;
        const int wc = valid ? w : W - 1;
        cplx X[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) X[u] = {0.0, 0.0};
        for (int l = 0; l < DD; ++l) {
            const cplx r = R[static_cast<size_t>(l)*W + wc];
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const int e = min(wave + 4*u, DD - 1);
                cmac(X[u], r, Cp[l*DD + e]);
            }
        }
        const HalfAngle x = reduce_two_pi(omega[wc]*T);
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = wave + 4*u;
            if (e < DD) {
                const cplx s = dirichlet_factor(half_angle(x, dphi[2*e], dphi[2*e + 1]), n);
                const cplx y = cmul(X[u], s);
                Yr[e*kPad + lane] = valid ? y.re : 0.0;
                Yi[e*kPad + lane] = valid ? y.im : 0.0;
            }
        }
        if (wave == 0) cw[lane] = valid ? sc[wc].re : 0.0;
        __syncthreads();
        if constexpr (D == 4) {
            const int c = lane & 15, r4 = lane >> 4;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int wl = 16*wave + 4*s + r4;
                const double yr = Yr[c*kPad + wl], yi = Yi[c*kPad + wl], cc = cw[wl];
                acc_rr = __builtin_amdgcn_mfma_f64_16x16x4f64(yr, cc*yr, acc_rr, 0, 0, 0);
                acc_ii = __builtin_amdgcn_mfma_f64_16x16x4f64(yi, cc*yi, acc_ii, 0, 0, 0);
                acc_ri = __builtin_amdgcn_mfma_f64_16x16x4f64(yr, cc*yi, acc_ri, 0, 0, 0);
            }
        } else {
            if (threadIdx.x < DD*DD && ge <= gf) {
                for (int wl = 0; wl < kChunk; ++wl) {
                    const double cc = cw[wl];
                    const cplx a = {Yr[ge*kPad + wl], Yi[ge*kPad + wl]};
                    const cplx b = {cc*Yr[gf*kPad + wl], cc*Yi[gf*kPad + wl]};
                    cmac_conj(acc, a, b);
                }
            }
        }
        __syncthreads();
    }
    if constexpr (D == 4) {
        const int c = lane & 15, r4 = lane >> 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            part[((wave*3 + 0)*16 + r4 + 4*r)*17 + c] = acc_rr[r];
            part[((wave*3 + 1)*16 + r4 + 4*r)*17 + c] = acc_ii[r];
            part[((wave*3 + 2)*16 + r4 + 4*r)*17 + c] = acc_ri[r];
        }
        __syncthreads();
        // thread (e, f): the tiles of the four wavefronts in index order
        double re = 0.0, m_ef = 0.0, m_fe = 0.0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            re += part[((g*3 + 0)*16 + ge)*17 + gf] + part[((g*3 + 1)*16 + ge)*17 + gf];
            m_ef += part[((g*3 + 2)*16 + ge)*17 + gf];
            m_fe += part[((g*3 + 2)*16 + gf)*17 + ge];
        }
        acc = {re, m_ef - m_fe};
    }
    if (threadIdx.x < DD*DD && ge <= gf) {
        G[ge*DD + gf] = acc;
        if (ge != gf) G[gf*DD + ge] = {acc.re, -acc.im};
        else G[ge*DD + gf].im = 0.0;
    }
    __syncthreads();
    // E[f][l] = C'_l[m, j] with f = (j, m):  Cp[l DD + m D + j]
    if (threadIdx.x < DD*DD) {
        const int e = ge, l = gf;
        cplx t = {0.0, 0.0};
#pragma unroll
        for (int f = 0; f < DD; ++f) cmac(t, G[e*DD + f], Cp[l*DD + (f % D)*D + f / D]);
        Tm[e*DD + l] = t;
    }
    __syncthreads();
    if (threadIdx.x < DD*DD && ge <= gf) {
        const int k = ge, l = gf;
        double re = 0.0;
#pragma unroll
        for (int e = 0; e < DD; ++e) {
            const cplx a = Cp[k*DD + (e % D)*D + e / D];
            const cplx t = Tm[e*DD + l];
            re = fma(a.re, t.re, re);
            re = fma(a.im, t.im, re);
        }
        double* o = gamma + ((static_cast<size_t>(p)*K + q)*n_ops + i)*DD*DD;
        o[k*DD + l] = re;
        o[l*DD + k] = re;
    }
}

}  // namespace

bool periodic_supported(int P, int K, int d, int W, int n_ops) {
    return P >= 1 && P <= 65535 && K >= 1 && K <= 65535 && d >= 2 && d <= 4 && W >= 1 && n_ops >= 1 && n_ops <= 65535;
}

hipError_t launch_periodic_fejer(const cplx* const* Rtab, int P, int d, int W, const cplx* basis, const cplx* V,
                                 const double* phi, const double* period, const double* omega,
                                 const int32_t* repeats, int K, const int32_t* ops, int n_ops, const cplx* scale,
                                 int s_ndim, int d_infidelity, double* F, double* infid, hipStream_t stream) {
    if (!periodic_supported(P, K, d, W, n_ops) || (infid && !scale)) return hipErrorInvalidValue;
    const dim3 grid(n_ops, (K + kRepeatChunk - 1)/kRepeatChunk, P);
    const double inv_d = infid ? 1.0/d_infidelity : 0.0;
#define FFK_LAUNCH(D)                                                                                                \
    periodic_fejer_kernel<D><<<grid, 64, 0, stream>>>(Rtab, basis, V, phi, period, omega, W, repeats, K, ops,  \
                                                            n_ops, scale, s_ndim, inv_d, F, infid)
    if (d == 2) FFK_LAUNCH(2);
    else if (d == 3) FFK_LAUNCH(3);
    else FFK_LAUNCH(4);
#undef FFK_LAUNCH
    return hipGetLastError();
}

hipError_t launch_periodic_decay(const cplx* const* Rtab, int P, int d, int W, const cplx* basis, const cplx* V,
                                 const double* phi, const double* period, const double* omega,
                                 const int32_t* repeats, int K, const int32_t* ops, int n_ops, const cplx* scale,
                                 int s_ndim, double* gamma, hipStream_t stream) {
    if (!periodic_supported(P, K, d, W, n_ops) || !scale || !gamma) return hipErrorInvalidValue;
    const dim3 grid(n_ops, K, P);
#define FFK_LAUNCH(D)                                                                                                \
    periodic_decay_kernel<D><<<grid, kThreads, 0, stream>>>(Rtab, basis, V, phi, period, omega, W, repeats, K, ops,  \
                                                            n_ops, scale, s_ndim, gamma)
    if (d == 2) FFK_LAUNCH(2);
    else if (d == 3) FFK_LAUNCH(3);
    else FFK_LAUNCH(4);
#undef FFK_LAUNCH
    return hipGetLastError();
}

// ---- second order: frequency shifts by period doubling -----------------------------------
// The concatenation rule of the second-order filter function, integrated, for an atom of m periods followed by one
// of m' periods of the same pulse:
//     Delta_{m+m'} = Delta_m + Q_m^T Delta_{m'} Q_m + X(m, m'),
//     X(m, m')[k,l] = sum_w c_w Re( conj( e^{i w m T} (R_{m'} Q_m)[k,w] ) R_m[l,w] ),
// Q_m the Liouville matrix of U^m.  In U's eigenbasis both operands are element-wise in what periodic_decay_kernel
// forms: R_m <-> B_e = X'_e s_e(m), and e^{i w m T} R_{m'} Q_m <-> A_e = X'_e s_e(m') e^{i m theta_e} (the terms
// g = m .. m + m' - 1 of the sum), so that
//     M[e,f] = sum_w c_w conj(A_e) B_f   (d^2 x d^2 complex, not Hermitian),
//     X[k,l] = Re sum_ef conj(E[e,k]) M[e,f] E[f,l],
//     Q_m[i,j] = Re sum_ab e^{-i m (phi_a - phi_b)} C'_i[a,b] C'_j[b,a].
// A host-made plan of steps (m, m', slot of Delta_m, slot of Delta_m') reaches every count in O(log n) steps; the
// result of step s lies in slot s + 1, slot 0 is Delta_1.
namespace {

// Block (selected operator i, step s, pulse p), four wavefronts, as periodic_decay_kernel: steps of 64 frequencies,
// wavefront g fills the two operands of the entries e = g, g + 4, ... into LDS; then M of the step --
//   d = 4: four real chains on v_mfma_f64_16x16x4_f64, Re = Ar^T c Br + Ai^T c Bi, Im = Ar^T c Bi - Ai^T c Br, the four
//          wavefronts' tiles added in index order after the last step (their LDS is that of the operands, reused);
//   d = 2, 3: thread (e, f), vector FMAs over the 64 frequencies in order.
// Then T = M E and X[k,l] = Re sum_e conj(E[e,k]) T[e,l] for all (k, l) into tiles (P, n_ops, S, N, N).
template <int D>
__global__ __launch_bounds__(kThreads) void periodic_shift_gram_kernel(
    const cplx* const* __restrict__ Rtab, const cplx* __restrict__ basis, const cplx* __restrict__ Vall,
    const double* __restrict__ phiall, const double* __restrict__ period, const double* __restrict__ omega, int W,
    const int32_t* __restrict__ steps, int S, const int32_t* __restrict__ ops, int n_ops,
    const cplx* __restrict__ scale, int s_ndim, double* __restrict__ tiles) {
    constexpr int DD = D*D, PER = (DD + 3)/4, PLANE = DD*kPad;
    constexpr int PART = D == 4 ? 4*4*16*17 : 0;
    constexpr int BUF = PART > 4*PLANE ? PART : 4*PLANE;
    __shared__ cplx Cp[DD*DD];
    __shared__ double dphi[2*DD];
    __shared__ double buf[BUF], cw[kChunk];
    __shared__ cplx M[DD*DD], Tm[DD*DD];
    double* const Ar = buf;
    double* const Ai = buf + PLANE;
    double* const Br = buf + 2*PLANE;
    double* const Bi = buf + 3*PLANE;
    const int i = blockIdx.x, s = blockIdx.y, p = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    rotate_basis<D, kThreads>(basis, Vall + static_cast<size_t>(p)*DD, phiall + static_cast<size_t>(p)*2*DD, Cp, dphi);
    __syncthreads();
    const double T = period[p];
    const double m = static_cast<double>(steps[4*s]), mp = static_cast<double>(steps[4*s + 1]);
    const cplx* R = Rtab[p] + static_cast<size_t>(ops[i])*DD*W;
    const cplx* sc = scale + static_cast<size_t>(s_ndim == 1 ? 0 : i)*W;
    const int ge = threadIdx.x / DD, gf = threadIdx.x % DD;
    cplx acc = {0.0, 0.0};
    f64x4 acc_rr = {0.0, 0.0, 0.0, 0.0}, acc_ii = {0.0, 0.0, 0.0, 0.0}, acc_ri = {0.0, 0.0, 0.0, 0.0},
          acc_ir = {0.0, 0.0, 0.0, 0.0};
    for (int w0 = 0; w0 < W; w0 += kChunk) {
        const int w = w0 + lane;
        const bool valid = w < W;
        const int wc = valid ? w : W - 1;
        cplx X[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) X[u] = {0.0, 0.0};
        for (int l = 0; l < DD; ++l) {
            const cplx r = R[static_cast<size_t>(l)*W + wc];
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const int e = min(wave + 4*u, DD - 1);
                cmac(X[u], r, Cp[l*DD + e]);
            }
        }
        const HalfAngle x = reduce_two_pi(omega[wc]*T);
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = wave + 4*u;
            if (e < DD) {
                const HalfAngle h = half_angle(x, dphi[2*e], dphi[2*e + 1]);
                const cplx sm = dirichlet_factor(h, m);
                const cplx smp = mp == m ? sm : dirichlet_factor(h, mp);
                // e^{i m theta} = e^{i (2 m) h}: the multiplier is exact as a double
                cplx ph;
                sincos_multiple<true>(2.0*m, h, &ph.im, &ph.re);
                const cplx a = cmul(cmul(X[u], smp), ph);
                const cplx b = cmul(X[u], sm);
                Ar[e*kPad + lane] = valid ? a.re : 0.0;
                Ai[e*kPad + lane] = valid ? a.im : 0.0;
                Br[e*kPad + lane] = valid ? b.re : 0.0;
                Bi[e*kPad + lane] = valid ? b.im : 0.0;
            }
        }
        if (wave == 0) cw[lane] = valid ? sc[wc].re : 0.0;
        __syncthreads();
        if constexpr (D == 4) {
            const int c = lane & 15, r4 = lane >> 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int wl = 16*wave + 4*q + r4;
                const double cc = cw[wl];
                const double ar = Ar[c*kPad + wl], ai = Ai[c*kPad + wl];
                const double br = cc*Br[c*kPad + wl], bi = cc*Bi[c*kPad + wl];
                acc_rr = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, acc_rr, 0, 0, 0);
                acc_ii = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bi, acc_ii, 0, 0, 0);
                acc_ri = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, acc_ri, 0, 0, 0);
                acc_ir = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, acc_ir, 0, 0, 0);
            }
        } else {
            if (threadIdx.x < DD*DD) {
                for (int wl = 0; wl < kChunk; ++wl) {
                    const double cc = cw[wl];
                    const cplx a = {Ar[ge*kPad + wl], Ai[ge*kPad + wl]};
                    const cplx b = {cc*Br[gf*kPad + wl], cc*Bi[gf*kPad + wl]};
                    cmac_conj(acc, a, b);
                }
            }
        }
        __syncthreads();
    }
    if constexpr (D == 4) {
        // (the operands' LDS is free after the last step's barrier)
        double* const part = buf;
        const int c = lane & 15, r4 = lane >> 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            part[((wave*4 + 0)*16 + r4 + 4*r)*17 + c] = acc_rr[r];
            part[((wave*4 + 1)*16 + r4 + 4*r)*17 + c] = acc_ii[r];
            part[((wave*4 + 2)*16 + r4 + 4*r)*17 + c] = acc_ri[r];
            part[((wave*4 + 3)*16 + r4 + 4*r)*17 + c] = acc_ir[r];
        }
        __syncthreads();
        // thread (e, f): the tiles of the four wavefronts in index order
        double re = 0.0, im = 0.0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            re += part[((g*4 + 0)*16 + ge)*17 + gf] + part[((g*4 + 1)*16 + ge)*17 + gf];
            im += part[((g*4 + 2)*16 + ge)*17 + gf] - part[((g*4 + 3)*16 + ge)*17 + gf];
        }
        acc = {re, im};
    }
    if (threadIdx.x < DD*DD) M[ge*DD + gf] = acc;
    __syncthreads();
    // E[f][l] = C'_l[m, j] with f = (j, m):  Cp[l DD + m D + j]
    if (threadIdx.x < DD*DD) {
        const int e = ge, l = gf;
        cplx t = {0.0, 0.0};
#pragma unroll
        for (int f = 0; f < DD; ++f) cmac(t, M[e*DD + f], Cp[l*DD + (f % D)*D + f / D]);
        Tm[e*DD + l] = t;
    }
    __syncthreads();
    if (threadIdx.x < DD*DD) {
        const int k = ge, l = gf;
        double re = 0.0;
#pragma unroll
        for (int e = 0; e < DD; ++e) {
            const cplx a = Cp[k*DD + (e % D)*D + e / D];
            const cplx t = Tm[e*DD + l];
            re = fma(a.re, t.re, re);
            re = fma(a.im, t.im, re);
        }
        tiles[((static_cast<size_t>(p)*n_ops + i)*S + s)*DD*DD + k*DD + l] = re;
    }
}

// Block (selected operator i, pulse p) walks the plan serially.  Per step: the phases e^{-i m (phi_a - phi_b)} from
// the hi + lo differences (reduced as every other angle, the multiplier 2 m on the half angle), Q_m in LDS, then
// table[s + 1] = table[slot_m] + Q_m^T table[slot_m'] Q_m + X[s], in that order.  The table (P, n_ops, S + 1, N, N)
// lies in device memory: a block reads back only what it wrote itself, behind a barrier.  Last, the K rows of `out`
// (P, K, n_ops, N, N) are copied from the slots of the counts: with no step at all, Delta_1 bit for bit.
template <int D>
__global__ __launch_bounds__(kThreads) void periodic_shift_combine_kernel(
    const cplx* __restrict__ basis, const cplx* __restrict__ Vall, const double* __restrict__ phiall,
    const int32_t* __restrict__ steps, int S, const int32_t* __restrict__ count_slots, int K, int n_ops,
    const double* __restrict__ delta1, const double* __restrict__ tiles, double* table, double* __restrict__ out) {
    constexpr int DD = D*D, NN = DD*DD;
    __shared__ cplx Cp[NN];
    __shared__ double dphi[2*DD];
    __shared__ cplx ph[DD];
    __shared__ double Q[NN], Tm[NN];
    const int i = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
    const int k = t / DD, l = t % DD;
    const size_t member = static_cast<size_t>(p)*n_ops + i;
    rotate_basis<D, kThreads>(basis, Vall + static_cast<size_t>(p)*DD, phiall + static_cast<size_t>(p)*2*DD, Cp, dphi);
    double* tab = table + member*(static_cast<size_t>(S) + 1)*NN;
    const double* X = tiles + member*static_cast<size_t>(S)*NN;
    if (t < NN) tab[t] = delta1[member*NN + t];
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
        const double m = static_cast<double>(steps[4*s]);
        const size_t at_m = static_cast<size_t>(steps[4*s + 2])*NN, at_mp = static_cast<size_t>(steps[4*s + 3])*NN;
        if (t < DD) {
            const HalfAngle h = half_angle(HalfAngle{0.0, 0.0}, dphi[2*t], dphi[2*t + 1]);
            cplx e;
            sincos_multiple<true>(2.0*m, h, &e.im, &e.re);
            ph[t] = e;
        }
        __syncthreads();
        if (t < NN) {
            double q = 0.0;
#pragma unroll
            for (int ab = 0; ab < DD; ++ab) {
                const cplx c = cmul(Cp[k*DD + ab], Cp[l*DD + (ab % D)*D + ab / D]);
                q = fma(ph[ab].re, c.re, q);
                q = fma(-ph[ab].im, c.im, q);
            }
            Q[t] = q;
        }
        __syncthreads();
        if (t < NN) {
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < DD; ++q) v = fma(tab[at_mp + k*DD + q], Q[q*DD + l], v);
            Tm[t] = v;
        }
        __syncthreads();
        if (t < NN) {
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < DD; ++q) v = fma(Q[q*DD + k], Tm[q*DD + l], v);
            tab[(static_cast<size_t>(s) + 1)*NN + t] = (tab[at_m + t] + v) + X[static_cast<size_t>(s)*NN + t];
        }
        __syncthreads();
    }
    for (int item = t; item < K*NN; item += kThreads) {
        const int q = item / NN, x = item % NN;
        out[((static_cast<size_t>(p)*K + q)*n_ops + i)*NN + x] = tab[static_cast<size_t>(count_slots[q])*NN + x];
    }
}

}  // namespace

bool periodic_shifts_supported(int P, int K, int S, int d, int W, int n_ops) {
    return periodic_supported(P, K, d, W, n_ops) && S >= 0 && S <= 65535 && W >= 2;
}

hipError_t launch_periodic_shift_gram(const cplx* const* Rtab, int P, int d, int W, const cplx* basis, const cplx* V,
                                      const double* phi, const double* period, const double* omega,
                                      const int32_t* steps, int S, const int32_t* ops, int n_ops, const cplx* scale,
                                      int s_ndim, double* tiles, hipStream_t stream) {
    if (!periodic_shifts_supported(P, 1, S, d, W, n_ops) || S < 1 || !steps || !scale || !tiles)
        return hipErrorInvalidValue;
    const dim3 grid(n_ops, S, P);
#define FFK_LAUNCH(D)                                                                                                \
    periodic_shift_gram_kernel<D><<<grid, kThreads, 0, stream>>>(Rtab, basis, V, phi, period, omega, W, steps, S,    \
                                                                 ops, n_ops, scale, s_ndim, tiles)
    if (d == 2) FFK_LAUNCH(2);
    else if (d == 3) FFK_LAUNCH(3);
    else FFK_LAUNCH(4);
#undef FFK_LAUNCH
    return hipGetLastError();
}

hipError_t launch_periodic_shift_combine(int P, int d, const cplx* basis, const cplx* V, const double* phi,
                                         const int32_t* steps, int S, const int32_t* count_slots, int K, int n_ops,
                                         const double* delta1, const double* tiles, double* table, double* out,
                                         hipStream_t stream) {
    if (!periodic_shifts_supported(P, K, S, d, 2, n_ops) || !count_slots || !delta1 || !table || !out ||
        (S > 0 && (!steps || !tiles)))
        return hipErrorInvalidValue;
    const dim3 grid(n_ops, P);
#define FFK_LAUNCH(D)                                                                                                \
    periodic_shift_combine_kernel<D><<<grid, kThreads, 0, stream>>>(basis, V, phi, steps, S, count_slots, K, n_ops,  \
                                                                    delta1, tiles, table, out)
    if (d == 2) FFK_LAUNCH(2);
    else if (d == 3) FFK_LAUNCH(3);
    else FFK_LAUNCH(4);
#undef FFK_LAUNCH
    return hipGetLastError();
}

}  // namespace ffk

// grad_walk.h -- what the kernels that walk the segments of a gradient share (grad_batch.hip: P pulses of one shape;
// sequence_gradient.hip: gate sequences given as index arrays): the record of one segment, the step of the
// interaction-picture noise operator, and the body that evaluates the gradient's terms at one segment from
// Ytot^dag and the running sum Ycum held in registers.  The mathematics is grad.hip's (read its header first).
//
// Every function is inlined into its kernel; the arithmetic of a kernel that uses them is the arithmetic written
// here, statement by statement, so two kernels that call the same function round alike.
#pragma once

#include "ffk_internal.h"

namespace ffk {
namespace gradwalk {

// ---- record of one segment, in complex numbers: a header of 1 + d2 [as doubles: dt_s, t_s, W_mn (d2),
//      derivative_integral_rcp(W_mn, dt_s) (d2)], then [T (d2)] [Bbar (A d2)] [Abar (H d2)] [E (H d2)] ------------------------------------
__host__ __device__ inline size_t record_header(int d) { return static_cast<size_t>(1 + d*d); }
__host__ __device__ inline size_t record_elems(int d, int A, int H) {
    return record_header(d) + static_cast<size_t>(1 + A + 2*H)*d*d;
}

// dynamic LDS of a kernel that runs segment_terms: the record's header, T, Bbar_a, Abar and E of all H, the per-lane
// second terms, and two per-lane columns of d2
inline size_t segment_lds_bytes(int d, int H) {
    return size_t(1 + d*d)*sizeof(cplx) + size_t(2 + 2*H)*d*d*sizeof(cplx) + size_t(H)*64*sizeof(double) +
           2*size_t(d*d)*64*sizeof(cplx);
}

// I1[e] = I1(w + W_e) into the lane's LDS column, then Z = (Bbar o I1) T into the lane's second column
template <int D>
__device__ __forceinline__ void integrals_and_half_step(double om, double dts, const double* __restrict__ dE,
                                                        const cplx* __restrict__ Ts, const cplx* __restrict__ Bs,
                                                        cplx* __restrict__ I1, cplx* __restrict__ Z) {
    constexpr int D2 = D*D;
#pragma unroll 1
    for (int e = 0; e < D2; ++e) I1[e*64] = first_order_integral(om, dE[e], dts);
#pragma unroll 1
    for (int m = 0; m < D; ++m) {
        cplx X[D];
#pragma unroll
        for (int n = 0; n < D; ++n) X[n] = cmul(Bs[m*D + n], I1[(m*D + n)*64]);
#pragma unroll
        for (int j = 0; j < D; ++j) {
            cplx acc = {0.0, 0.0};
#pragma unroll
            for (int n = 0; n < D; ++n) cmac(acc, X[n], Ts[n*D + j]);
            Z[(m*D + j)*64] = acc;
        }
    }
}
// entry [i][j] of the step e^{i w t_s} T^dag Z
template <int D>
__device__ __forceinline__ cplx step_entry(const cplx* __restrict__ Ts, const cplx* __restrict__ Z, cplx ph, int i,
                                           int j) {
    cplx acc = {0.0, 0.0};
#pragma unroll
    for (int m = 0; m < D; ++m) cmac_conj(acc, Ts[m*D + i], Z[(m*D + j)*64]);
    return cmul(ph, acc);
}

// The block's view of its dynamic LDS (segment_lds_bytes): one record at a time, and the lane's columns.
template <int D>
struct SegmentLds {
    static constexpr int D2 = D*D;
    cplx* head;            // the record's header: dt_s, t_s,
    const double* hdr;
    const double* dE;      // [D2]  W_mn
    const double* inv;     // [D2]  derivative_integral_rcp(W_mn, dt)
    cplx* Ts;              // [D2]
    cplx* Bs;              // [D2]   (this block's operator)
    cplx* As;              // [H][D2]
    cplx* Es;              // [H][D2]
    double* sec;           // [H][64]  per-lane Re tr(E_h comm)
    cplx* I1;              // [D2][64] per-lane columns
    cplx* Wa;              // [D2][64] Z = (Bbar o I1) T first, then W_a
    __device__ __forceinline__ SegmentLds(unsigned char* smem, int H, int lane) {
        head = reinterpret_cast<cplx*>(smem);
        hdr = reinterpret_cast<const double*>(smem);
        dE = hdr + 2;
        inv = dE + D2;
        Ts = head + 1 + D2;
        Bs = Ts + D2;
        As = Bs + D2;
        Es = As + H*D2;
        sec = reinterpret_cast<double*>(Es + H*D2);
        I1 = reinterpret_cast<cplx*>(sec + H*64) + lane;
        Wa = I1 + D2*64;
    }
    // the record r of one segment: header and T, Bbar of operator a (b_off), Abar and E of all H (ae_off)
    __device__ __forceinline__ void load(const cplx* __restrict__ r, int b_off, int ae_off, int H, int lane) const {
        __syncthreads();
        if (lane < 1 + 2*D2) head[lane] = r[lane];
        if (lane < D2) Bs[lane] = r[b_off + lane];
        for (int e = lane; e < 2*H*D2; e += 64) As[e] = r[ae_off + e];   // Abar, E
        __syncthreads();
    }
};

// One segment, whose record is in LDS: adds the segment's step to Ycum (Yq) and hands emit(h, val, tr_step), for
// every control operator h, val = 2 Im(ph first_h) - 2 Re tr(E_h [Yd, Ycum]) -- the derivative of the filter function
// without the explicit sensitivity term -- and tr_step = 2 Re tr(Ytot^dag step) for that term.
template <int D, typename Emit>
__device__ __forceinline__ void segment_terms(const SegmentLds<D>& L, double om, int H, int lane, cplx (&Yd)[D*D],
                                              cplx (&Yq)[D*D], Emit&& emit) {
    constexpr int D2 = D*D;
    const double* dE = L.dE;
    const double* inv = L.inv;
    const cplx *Ts = L.Ts, *Bs = L.Bs, *As = L.As, *Es = L.Es;
    double* sec = L.sec;
    cplx *I1 = L.I1, *Wa = L.Wa;
    const double dts = L.hdr[0];
    const cplx ph = cexp(om*L.hdr[1]);
    integrals_and_half_step<D>(om, dts, dE, Ts, Bs, I1, Wa);
    // Ycum += step; explicit sensitivity term 2 Re tr(Ytot^dag step)
    double tr_step = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const cplx st = step_entry<D>(Ts, Wa, ph, i, j);
            Yq[i*D + j].re += st.re;
            Yq[i*D + j].im += st.im;
            tr_step += Yd[j*D + i].re*st.re - Yd[j*D + i].im*st.im;
        }
    tr_step *= 2.0;
    // (II): sec[h] = Re tr(E_h [Yd, Ycum])
    for (int h = 0; h < H; ++h) sec[h*64 + lane] = 0.0;
#pragma unroll
    for (int x = 0; x < D; ++x)
#pragma unroll
        for (int y = 0; y < D; ++y) {
            cplx cm = {0.0, 0.0};                      // comm[y][x]
#pragma unroll
            for (int k = 0; k < D; ++k) {
                cmac(cm, Yd[y*D + k], Yq[k*D + x]);
                const cplx q = cmul(Yq[y*D + k], Yd[k*D + x]);
                cm.re -= q.re;
                cm.im -= q.im;
            }
            for (int h = 0; h < H; ++h) {
                const cplx e = Es[h*D2 + x*D + y];
                sec[h*64 + lane] += e.re*cm.re - e.im*cm.im;
            }
        }
    // Wa = T Yd T^dag, row by row (Z is used up)
#pragma unroll
    for (int x = 0; x < D; ++x) {
        cplx row[D];                                   // (T Yd)[x][:]
#pragma unroll
        for (int k = 0; k < D; ++k) {
            cplx acc = {0.0, 0.0};
#pragma unroll
            for (int j = 0; j < D; ++j) cmac(acc, Ts[x*D + j], Yd[j*D + k]);
            row[k] = acc;
        }
#pragma unroll
        for (int y = 0; y < D; ++y) {
            cplx acc = {0.0, 0.0};
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const cplx ty = Ts[y*D + k];
                cmac(acc, row[k], cplx{ty.re, -ty.im});
            }
            Wa[(x*D + y)*64] = acc;
        }
    }
#pragma unroll 1
    for (int h = 0; h < H; ++h) {
        const cplx* Ab = As + h*D2;
        cplx first = {0.0, 0.0};
#pragma unroll 1
        for (int x = 0; x < D; ++x)
#pragma unroll 1
            for (int y = 0; y < D; ++y) {
                cplx g = {0.0, 0.0};                   // G_xy (grad.hip)
                const cplx iyx = I1[(y*D + x)*64];
#pragma unroll
                for (int n = 0; n < D; ++n) {
                    const cplx iyn = I1[(y*D + n)*64];
                    const cplx j1 = derivative_integral(om + dE[y*D + n], dE[n*D + x],
                                                        inv[n*D + x], dts, iyn, iyx);
                    cmac(g, cmul(Bs[y*D + n], Ab[n*D + x]), j1);
                    const cplx inx = I1[(n*D + x)*64];
                    const cplx j2 = derivative_integral(om + dE[n*D + x], dE[y*D + n],
                                                        inv[y*D + n], dts, inx, iyx);
                    const cplx ab = cmul(Ab[y*D + n], Bs[n*D + x]);
                    cmac(g, cplx{-ab.re, -ab.im}, j2);
                }
                cmac(first, Wa[(x*D + y)*64], g);
            }
        const cplx pf = cmul(ph, first);               // 2 Re(-i ph first) = 2 Im(ph first)
        emit(h, 2.0*pf.im - 2.0*sec[h*64 + lane], tr_step);
    }
}

// the sum of a value over the 64 lanes, in the order of the butterfly (the same in every lane)
__device__ __forceinline__ double lane_sum(double sum) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    return sum;
}

}  // namespace gradwalk
}  // namespace ffk

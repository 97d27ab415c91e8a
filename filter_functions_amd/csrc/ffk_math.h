// ffk_math.h -- scalar FP64 building blocks shared by every kernel of the filter-function path.
//
// All functions are __host__ __device__ so that tests/ can compile them for the host (a
// test-only harness, tests/csrc/) and check them against NumPy without a GPU; the product
// library only ever runs them on the device.
//
// Rounding contract (DESIGN.md "Numerics"): the reference evaluates sin/cos at the *rounded*
// arguments fl(omega*t_g) (numeric.py:865) and fl(fl(omega + dE)*dt) (numeric.py:155-163).
// For omega*t up to ~1e6 the rounding of the argument itself is worth ~1e-10 relative in the
// result, so the kernels form exactly the same double-precision arguments and only the
// sin/cos implementation (<= ~1 ulp) differs from NumPy's.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#define FFK_HD __host__ __device__ __forceinline__

namespace ffk {

struct cplx {
    double re, im;
};

FFK_HD cplx cmul(cplx a, cplx b) {
    return {fma(a.re, b.re, -(a.im*b.im)), fma(a.re, b.im, a.im*b.re)};
}
// acc += a*b
FFK_HD void cmac(cplx& acc, cplx a, cplx b) {
    acc.re = fma(a.re, b.re, acc.re);
    acc.re = fma(-a.im, b.im, acc.re);
    acc.im = fma(a.re, b.im, acc.im);
    acc.im = fma(a.im, b.re, acc.im);
}
// acc += conj(a)*b
FFK_HD void cmac_conj(cplx& acc, cplx a, cplx b) {
    acc.re = fma(a.re, b.re, acc.re);
    acc.re = fma(a.im, b.im, acc.re);
    acc.im = fma(a.re, b.im, acc.im);
    acc.im = fma(-a.im, b.re, acc.im);
}

// ---------------------------------------------------------------------------------------
// sincos for |x| < ~2^50: 3-term Cody-Waite reduction with FMA (pi/2 = P1 + P2 + P3 carries
// ~160 bits, so the reduction error stays ~1e-16 absolute for every k that is an exact
// double), then the classic minimax kernels on [-pi/4, pi/4] (13th/14th degree; the
// coefficients are the widely published fdlibm k_sin/k_cos constants).  Max error observed
// against NumPy on random arguments up to 1e8: 1 ulp (tests/test_math_host.py).
// round-to-nearest and the quadrant come from the 1.5*2^52 "magic number" addition: the low
// mantissa bits of t hold the integer k.  NaN/Inf give NaN.
// ---------------------------------------------------------------------------------------
// FFK_PIN(c): the constant is materialised (two v_mov_b32) where it is used.  Inside a loop the
// compiler otherwise hoists every polynomial coefficient into a register that stays live across
// the whole loop body; the accumulate kernel (ctrl.hip) cannot afford those ~34 VGPRs across its
// contraction phase.
template <unsigned long long BITS>
FFK_HD double pinned_bits() {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned lo, hi;
    asm volatile("v_mov_b32 %0, %1" : "=v"(lo) : "n"(static_cast<unsigned>(BITS & 0xffffffffull)));
    asm volatile("v_mov_b32 %0, %1" : "=v"(hi) : "n"(static_cast<unsigned>(BITS >> 32)));
    return __hiloint2double(static_cast<int>(hi), static_cast<int>(lo));
#else
    return __builtin_bit_cast(double, BITS);
#endif
}
#define FFK_PIN(c) (PIN ? pinned_bits<__builtin_bit_cast(unsigned long long, static_cast<double>(c))>() : (c))

template <bool PIN = false>
FFK_HD void sincos_reduced(double r, double* s, double* c) {
    const double z = r*r;
    // sin
    double ps = fma(z, FFK_PIN(1.58969099521155010221e-10), FFK_PIN(-2.50507602534068634195e-08));
    ps = fma(z, ps, FFK_PIN(2.75573137070700676789e-06));
    ps = fma(z, ps, FFK_PIN(-1.98412698298579493134e-04));
    ps = fma(z, ps, FFK_PIN(8.33333333332248946124e-03));
    ps = fma(z, ps, FFK_PIN(-1.66666666666666324348e-01));
    *s = fma(r*z, ps, r);
    // cos
    double pc = fma(z, FFK_PIN(-1.13596475577881948265e-11), FFK_PIN(2.08757232129817482790e-09));
    pc = fma(z, pc, FFK_PIN(-2.75573143513906633035e-07));
    pc = fma(z, pc, FFK_PIN(2.48015872894767294178e-05));
    pc = fma(z, pc, FFK_PIN(-1.38888888888741095749e-03));
    pc = fma(z, pc, FFK_PIN(4.16666666666666019037e-02));
    const double hz = 0.5*z;
    const double w = 1.0 - hz;
    *c = w + (((1.0 - w) - hz) + z*z*pc);
}

// the same kernels cut to the terms that matter for |r| < 2^-5 (z < 2^-10: the dropped terms are
// below 2^-60 relative)
template <bool PIN = false>
FFK_HD void sincos_small(double r, double* s, double* c) {
    const double z = r*r;
    double ps = fma(z, FFK_PIN(2.75573137070700676789e-06), FFK_PIN(-1.98412698298579493134e-04));
    ps = fma(z, ps, FFK_PIN(8.33333333332248946124e-03));
    ps = fma(z, ps, FFK_PIN(-1.66666666666666324348e-01));
    *s = fma(r*z, ps, r);
    double pc = fma(z, FFK_PIN(2.48015872894767294178e-05), FFK_PIN(-1.38888888888741095749e-03));
    pc = fma(z, pc, FFK_PIN(4.16666666666666019037e-02));
    const double hz = 0.5*z;
    const double w = 1.0 - hz;
    *c = w + (((1.0 - w) - hz) + z*z*pc);
}

// sincos_small's sine alone: the same operations in the same order, bit for bit (tests/test_sin_small_host.py).
// With PIN only its four constants are materialised; through sincos_small<true> a caller that drops the cosine
// still pays the cosine's six v_mov_b32 (pinned_bits is asm volatile: dead constants are not removed).
template <bool PIN = false>
FFK_HD double sin_small(double r) {
    const double z = r*r;
    double ps = fma(z, FFK_PIN(2.75573137070700676789e-06), FFK_PIN(-1.98412698298579493134e-04));
    ps = fma(z, ps, FFK_PIN(8.33333333332248946124e-03));
    ps = fma(z, ps, FFK_PIN(-1.66666666666666324348e-01));
    return fma(r*z, ps, r);
}

FFK_HD unsigned low_word(double t) {
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<unsigned>(__double2loint(t));
#else
    unsigned long long bits;
    __builtin_memcpy(&bits, &t, sizeof bits);
    return static_cast<unsigned>(bits);
#endif
}

template <bool PIN = false>
FFK_HD void sincos_pi(double x, double* s, double* c) {
    const double kMagic = FFK_PIN(6755399441055744.0);                     // 1.5 * 2^52
    const double t = fma(x, FFK_PIN(6.36619772367581382433e-01), kMagic);  // x * 2/pi, rounded to integer
    const unsigned q = low_word(t);
    const double k = t - kMagic;
    double r = fma(-k, FFK_PIN(1.57079632679489655800e+00), x);            // pi/2 high
    r = fma(-k, FFK_PIN(6.12323399573676603587e-17), r);                   // pi/2 mid
    r = fma(-k, FFK_PIN(-1.49738490485916983294e-33), r);                  // pi/2 low
    double sr, cr;
    sincos_reduced<PIN>(r, &sr, &cr);
    const double s0 = (q & 1u) ? cr : sr;
    const double c0 = (q & 1u) ? sr : cr;
    *s = (q & 2u) ? -s0 : s0;
    *c = ((q + 1u) & 2u) ? -c0 : c0;
}

#undef FFK_PIN

// Reciprocal to ~1 ulp.  Device: v_rcp_f64 seed + two Newton steps; host: plain division.
FFK_HD double rcp(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    double y = __builtin_amdgcn_rcp(x);
    double e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    return y;
#else
    return 1.0/x;
#endif
}

// Reciprocal to ~1e-15 relative (10 ulp): v_rcp_f64 (4.6e-8 on gfx950, measured over 2^20 random
// arguments of either sign and 40 binades) + ONE Newton step.  For the integral entries of the
// accumulate kernels, where the factor 1/x multiplies a sine that is itself good to ~1 ulp and
// 256 segments are summed: two instructions less per entry and frequency.
FFK_HD double rcp_fast(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    double y = __builtin_amdgcn_rcp(x);
    const double e = fma(-x, y, 1.0);
    return fma(y, e, y);
#else
    return 1.0/x;
#endif
}

// 1/sqrt(x) to ~1 ulp for normal x > 0.  Device: v_rsq_f64 seed + two Newton steps.
FFK_HD double rsqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    double y = __builtin_amdgcn_rsq(x);
    double e = fma(-x*y, y, 1.0);
    y = fma(y, 0.5*e, y);
    e = fma(-x*y, y, 1.0);
    y = fma(y, 0.5*e, y);
    return y;
#else
    return 1.0/sqrt(x);
#endif
}

// First-order Magnus integral of one (m, n) entry, numeric.py:144-167 with util.cexpm1
// (util.py:165-182):
//     I = (exp(i x dt) - 1)/(i x),  x = omega + dE,  I = dt where x == 0 exactly.
// exp(iy) - 1 = -2 sin^2(y/2) + i sin(y) and sin(y) = 2 sin(y/2) cos(y/2), so with
// s = sin(y/2), c = cos(y/2):  I = (2 s / x) (c + i s).  Cancellation free like the
// reference's form; one sincos instead of two sin.
FFK_HD cplx first_order_integral(double omega, double dE, double dt) {
    const double x = omega + dE;              // same rounding as np.add.outer(E, dE)
    const double y = x*dt;                    // same rounding as int_buf.imag*dt
    double s, c;
    sincos_pi(0.5*y, &s, &c);
    const double q = 2.0*s*rcp(x);
    cplx out = {q*c, q*s};
    if (x == 0.0) {
        out.re = dt;
        out.im = 0.0;
    }
    return out;
}

// The same integral for an off-diagonal entry, given sin/cos of the two half-angles
//     a = fl(omega*dt)/2     (per frequency: the diagonal entry's own argument) and
//     b = fl(dE*dt)/2        (per segment and entry: frequency independent, precomputed),
// through the addition theorems  sin(a+b) = sa cb + ca sb,  cos(a+b) = ca cb - sa sb:
// 4 flops instead of a sincos.  x = fl(omega + dE) (for 1/x and the exact-zero test) is still
// formed exactly like the reference; only the half-angle a+b differs from the reference's
// fl(fl(omega+dE)*dt)/2 by a few ulp of (|omega|+|dE|) dt, worth ~1e-16*dt absolute in I.
// Near a resonance (omega ~ -dE) the sum sa cb + ca sb cancels; below |h| < 2^-5 the direct
// evaluation is used instead (a divergent branch; for an OFF-diagonal entry the band is a few
// percent of a logarithmic grid, for the half of the entries with dE < 0 -- a caller that passes
// dE = 0 is inside it for every frequency below 2^-4/dt).
FFK_HD cplx first_order_integral_aa(double omega, double dE, double dt, double sa, double ca,
                                    double sb, double cb) {
    const double x = omega + dE;
    const double h = 0.5*(x*dt);
    double s = fma(sa, cb, ca*sb);
    double c = fma(ca, cb, -(sa*sb));
    if (fabs(h) < 0.03125) sincos_small<true>(h, &s, &c);   // no range reduction needed here
    const double q = 2.0*s*rcp_fast(x);
    cplx out = {q*c, q*s};
    if (x == 0.0) {
        out.re = dt;
        out.im = 0.0;
    }
    return out;
}

// The accumulate kernels need E = e^{i omega t_g} I, not I: with h = (omega + dE) dt / 2,
//     I = e^{ih} 2 sin(h)/x      =>      E = e^{i(omega t_g + a)} e^{ib} (2 sin(a + b)/x),
// a = fl(omega dt)/2 per (segment, frequency), b = fl(dE dt)/2 per (segment, entry).  Per frequency
// and segment (PhasedFrequency): psi = e^{i omega t_g} e^{ia} and 2 sin a, 2 cos a; per entry one
// rotation of psi by b (4 flops), 2 sin(a + b) by the addition theorem (2), a reciprocal, 3 products:
// 13 instructions and no select, against 25 for "I, then multiply by the phase" (cos(a + b) is never
// formed, the phase costs nothing extra, the x == 0 limit lives in the near branch).  Near a
// resonance (|x dt| < 2^-4, which includes x == 0 and zero-length segments) the sine comes from the
// short polynomial -- the sum would cancel -- as in first_order_integral_aa.  The near branch is NOT
// rare for the diagonal entries: dE = 0 there, so every frequency below 2^-4/dt takes it for every
// segment -- the lower decades of any logarithmic grid (tools/count_near_resonance.py; the d = 4
// kernel gives the diagonal a path of its own, ctrl_pq.hip, DESIGN.md section 6.1 "Round 8").
// E = psi e^{ib} q with q = 2 sin(a + b)/x REAL: the d = 4 kernel (ctrl_pq.hip) never forms E; it
// folds e^{ib} into the frequency-independent operands and contracts with q (phased_q) alone.
struct PhasedFrequency {
    double om, dt, thr;        // frequency, segment length, 2^-4/dt
    double pr, pi;             // psi = e^{i omega t_g} e^{i a}
    double sa2, ca2;           // 2 sin a, 2 cos a
};
FFK_HD PhasedFrequency phased_frequency(double om, double dt, cplx ph, double sa, double ca) {
    PhasedFrequency f;
    f.om = om;
    f.dt = dt;
    // (a zero-length segment: every entry takes the exact branch, which yields I = 0 also at x == 0)
    f.thr = dt > 0.0 ? 0.0625*rcp(dt) : __builtin_huge_val();
    f.pr = fma(ph.re, ca, -(ph.im*sa));
    f.pi = fma(ph.re, sa, ph.im*ca);
    f.sa2 = sa + sa;
    f.ca2 = ca + ca;
    return f;
}
// the real factor 2 sin(a + b)/x of an entry (x == 0: dt); phased_q_near: its form for |x| < thr alone
FFK_HD double phased_q_near(double x, double dt) {
    const double s = sin_small<true>(0.5*(x*dt));
    return x == 0.0 ? dt : 2.0*s*rcp_fast(x);
}
FFK_HD double phased_q(const PhasedFrequency& f, double dE, double sb, double cb) {
    const double x = f.om + dE;
    double q;
    if (fabs(x) < f.thr) {
        q = phased_q_near(x, f.dt);
    } else {
        q = fma(f.sa2, cb, f.ca2*sb)*rcp_fast(x);
    }
    return q;
}
FFK_HD cplx phased_integral_aa(const PhasedFrequency& f, double dE, double sb, double cb) {
    const double er = fma(f.pr, cb, -(f.pi*sb));
    const double ei = fma(f.pr, sb, f.pi*cb);
    const double q = phased_q(f, dE, sb, cb);
    return {q*er, q*ei};
}

// exp(i x) as (cos, sin), util.py:136-162
template <bool PIN = false>
FFK_HD cplx cexp(double x) {
    cplx out;
    sincos_pi<PIN>(x, &out.im, &out.re);
    return out;
}

// ---------------------------------------------------------------------------------------
// The nested integral of the gradient (gradient.py:69-108),
//     J(x, b) = int_0^dt dtau e^{i x tau} int_0^tau dtau' e^{i b tau'},   x = omega + W_a,
// from the first-order integrals I1(x) and I1(x + b) the gradient kernels hold anyway.  With
// X = x dt, B = b dt and M_k = int_0^dt tau^k e^{i x tau} dtau (M_0 = I1(x)) three regimes:
//   |B| >= theta          the reference's divided difference (I1(x + b) - I1(x))/(i b); its rounding
//                         error is ~u/|B| of dt^2/2 (u = 2^-53), at most 4 u/theta = 4.5e-13;
//   |B| <  theta (and 0)  J = sum_{k<4} (i b)^k/(k+1)! M_{k+1}   (the inner integral expanded in b;
//                         the first term dropped is below theta^4/720 of dt^2), with
//       |X| >= 2^-9       M_k = (dt^k e^{i x dt} - k M_{k-1})/(i x) upwards from I1.  Step k multiplies
//                         the error by k/|X| and M_k enters with B^(k-1)/k!: M_1 costs 4 u/|X| <= 2.3e-13
//                         of dt^2/2, M_2 256 u, M_3 128 u, M_4 64 u.  At b == 0 the sum is M_1, the
//                         reference's own (dt e^{i x dt} - I1)/(i x);
//       |X| <  2^-9       where that recurrence cancels (the reference loses u/|X| here, everything
//                         at a resonance met to the last bit): M_4 from its Taylor series
//                         sum_j (iX)^j/(j! (j+5)) (6 terms, remainder < 1e-20), then DOWNWARDS
//                         k M_{k-1} = dt^k e^{i x dt} - i x M_k, which damps errors.
// The reference (and the oracle) test b == 0 and x == 0 exactly and lose u/|B|, u/|X| next to
// those points: a segment with amplitudes of 1e-9 or a level crossing costs them 7+ digits.
// Which side of theta: per segment and level pair, not per frequency -- derivative_integral_rcp
// is evaluated once where 1/W_mn used to be, and its zero selects the series.
// ---------------------------------------------------------------------------------------
constexpr double kDerivativeIntegralBand = 0.0009765625;      // theta = 2^-10
constexpr double kDerivativeIntegralTaylor = 0.001953125;     // 2^-9: |x dt| below which the moments come from series

// a constant materialised where it is used (pinned_bits): hoisted out of the callers' unrolled loops these
// would take scalar registers that the fused batched kernel does not have
#define FFK_PINNED(c) pinned_bits<__builtin_bit_cast(unsigned long long, static_cast<double>(c))>()

// one Horner step of the series, S_J = 1/(J+5) + (iX/(J+1)) S_{J+1}
template <int J>
FFK_HD void derivative_integral_series_step(double X, cplx& S) {
    const double f = X*FFK_PINNED(1.0/(J + 1));
    S = {fma(-f, S.im, FFK_PINNED(1.0/(J + 5))), f*S.re};
    if constexpr (J > 0) derivative_integral_series_step<J - 1>(X, S);
}

// 1/b for the divided difference; 0 where |b dt| < theta: the series
FFK_HD double derivative_integral_rcp(double b, double dt) {
    return fabs(b*dt) < kDerivativeIntegralBand ? 0.0 : 1.0/b;
}

// m_1 + (iB/2) (m_2 + (iB/3) (m_3 + (iB/4) m_4)), times unit
FFK_HD cplx derivative_integral_sum(double B, double unit, cplx m1, cplx m2, cplx m3, cplx m4) {
    const double B4 = 0.25*B, B2 = 0.5*B;
    const double B3 = FFK_PINNED(1.0/3.0)*B;
    cplx h = {fma(-B4, m4.im, m3.re), fma(B4, m4.re, m3.im)};
    h = {fma(-B3, h.im, m2.re), fma(B3, h.re, m2.im)};
    h = {fma(-B2, h.im, m1.re), fma(B2, h.re, m1.im)};
    return {unit*h.re, unit*h.im};
}

// J(x, b); rb = derivative_integral_rcp(b, dt), i1x = I1(x), i1xb = I1(x + b).  The two series branches stand side
// by side, not nested, and each one's condition is ONE comparison of a value made for it: one saved execution
// mask at a time (the fused batched kernel has no scalar register to spare; a third branch that stops after
// M_1 at b == 0 spills there).
FFK_HD cplx derivative_integral(double x, double b, double rb, double dt, cplx i1x, cplx i1xb) {
    const cplx df = {i1xb.re - i1x.re, i1xb.im - i1x.im};
    cplx j = {df.im*rb, -df.re*rb};                                    // df/(i b)
    const double X = x*dt;
    const double up = rb == 0.0 ? fabs(X) : -1.0, down = rb == 0.0 ? fabs(X) : 1.0;
    if (up >= kDerivativeIntegralTaylor) {
        const cplx ex = {1.0 - x*i1x.im, x*i1x.re};                    // e^{i x dt} = 1 + i x I1
        const double rx = 1.0/x;
        const cplx m1 = {(dt*ex.im - i1x.im)*rx, -(dt*ex.re - i1x.re)*rx};         // (dt e^{i x dt} - I1)/(i x)
        double p = dt*dt;
        const cplx m2 = {(p*ex.im - 2.0*m1.im)*rx, -(p*ex.re - 2.0*m1.re)*rx};
        p *= dt;
        const cplx m3 = {(p*ex.im - 3.0*m2.im)*rx, -(p*ex.re - 3.0*m2.re)*rx};
        p *= dt;
        const cplx m4 = {(p*ex.im - 4.0*m3.im)*rx, -(p*ex.re - 4.0*m3.re)*rx};
        j = derivative_integral_sum(b, 1.0, m1, m2, m3, m4);
    }
    if (down < kDerivativeIntegralTaylor) {
        // m_k = M_k/dt^(k+1) = int_0^1 u^k e^{i X u} du; Horner S_j = 1/(j+5) + (iX/(j+1)) S_{j+1}
        const cplx ex = {1.0 - x*i1x.im, x*i1x.re};
        cplx m4 = {FFK_PINNED(1.0/10.0), 0.0};                         // j = 5
        derivative_integral_series_step<4>(X, m4);
        const double third = FFK_PINNED(1.0/3.0);
        const cplx m3 = {0.25*(ex.re + X*m4.im), 0.25*(ex.im - X*m4.re)};          // (e^{iX} - iX m_4)/4
        const cplx m2 = {(ex.re + X*m3.im)*third, (ex.im - X*m3.re)*third};
        const cplx m1 = {0.5*(ex.re + X*m2.im), 0.5*(ex.im - X*m2.re)};
        j = derivative_integral_sum(b*dt, dt*dt, m1, m2, m3, m4);
    }
    return j;
}

// ---------------------------------------------------------------------------------------
// The nested integral of the second-order filter function (numeric.py:170-256) is the same J:
//     I_{ij,mn}(w) = (f(a) - f(a + b))/b = J(a, b),  f = i I1,  a = W_ij - w,  b = w + W_mn.
// The second-order kernels contract over ij before they meet mn (second.hip), so the series comes in two
// halves that are linear in between:
//     m_k(a) = M_k(a)/dt^(k+1), k = 1..4                         second_order_moments, per (w, ij)
//     J      = dt^2 sum_{k<4} (i b dt)^k/(k+1)! m_{k+1}          second_order_series, per (w, mn), of the
//                                                                moments or of sum_ij NB_{r,ij} m_k(a_ij)
// with derivative_integral's regimes and bounds: |b dt| >= theta the divided difference (4 u/theta of dt^2/2
// at most), below it -- b == 0 included -- the series, whose moments come upwards from I1(a) where
// |a dt| >= 2^-9 and from the Taylor series of m_4, downwards, below that (a == 0 included).  Inside the band
// f(a + b) is never evaluated: the reference (and the oracle) take it at fl(W_ij + W_mn), which is not the sum
// of the rounded a and b, and next to a resonance their numerator no longer vanishes with b.
// ---------------------------------------------------------------------------------------
struct SecondOrderMoments {
    cplx m1, m2, m3, m4;
};

// i1a = I1(a)
FFK_HD SecondOrderMoments second_order_moments(double a, double dt, cplx i1a) {
    const double X = a*dt;
    const cplx ex = {1.0 - a*i1a.im, a*i1a.re};                        // e^{i a dt} = 1 + i a I1
    SecondOrderMoments m;
    if (fabs(X) >= kDerivativeIntegralTaylor) {
        // m_k = (e^{iX} - k m_{k-1})/(iX), m_0 = I1/dt   (dt != 0 here)
        const double rX = 1.0/X, rdt = 1.0/dt;
        m.m1 = {(ex.im - i1a.im*rdt)*rX, -(ex.re - i1a.re*rdt)*rX};
        m.m2 = {(ex.im - 2.0*m.m1.im)*rX, -(ex.re - 2.0*m.m1.re)*rX};
        m.m3 = {(ex.im - 3.0*m.m2.im)*rX, -(ex.re - 3.0*m.m2.re)*rX};
        m.m4 = {(ex.im - 4.0*m.m3.im)*rX, -(ex.re - 4.0*m.m3.re)*rX};
    } else {
        // Horner S_j = 1/(j+5) + (iX/(j+1)) S_{j+1}, then k m_{k-1} = e^{iX} - iX m_k
        m.m4 = {0.1, 0.0};                                             // j = 5
        derivative_integral_series_step<4>(X, m.m4);
        m.m3 = {0.25*(ex.re + X*m.m4.im), 0.25*(ex.im - X*m.m4.re)};
        m.m2 = {(ex.re + X*m.m3.im)*(1.0/3.0), (ex.im - X*m.m3.re)*(1.0/3.0)};
        m.m1 = {0.5*(ex.re + X*m.m2.im), 0.5*(ex.im - X*m.m2.re)};
    }
    return m;
}

FFK_HD cplx second_order_series(double b, double dt, cplx s1, cplx s2, cplx s3, cplx s4) {
    return derivative_integral_sum(b*dt, dt*dt, s1, s2, s3, s4);
}

// One entry, as the kernels evaluate it; ab is the argument they use for f(a + b), fl(W_ij + W_mn).
FFK_HD cplx second_order_integral(double a, double b, double ab, double dt) {
    const cplx i1a = first_order_integral(a, 0.0, dt);
    const double rb = derivative_integral_rcp(b, dt);
    if (rb == 0.0) {
        const SecondOrderMoments m = second_order_moments(a, dt, i1a);
        return second_order_series(b, dt, m.m1, m.m2, m.m3, m.m4);
    }
    const cplx i1ab = first_order_integral(ab, 0.0, dt);
    return {-(i1a.im - i1ab.im)*rb, (i1a.re - i1ab.re)*rb};           // (f(a) - f(ab))/b, f = (-Im I1, Re I1)
}

#undef FFK_PINNED

}  // namespace ffk

// Test-only harness: exposes the host instantiation of the __host__ __device__ numerics in
// filter_functions_amd/csrc/ffk_math.h through a C ABI so that tests/test_math_host.py can
// compare them with NumPy on a machine without a GPU.  Not part of the product library.
#include "ffk_math.h"

extern "C" {

void ffk_host_sincos(long n, const double* x, double* s, double* c) {
    for (long i = 0; i < n; ++i) ffk::sincos_pi(x[i], &s[i], &c[i]);
}

void ffk_host_first_order_integral(long n, const double* omega, const double* dE, double dt,
                                   double* out) {
    for (long i = 0; i < n; ++i) {
        ffk::cplx v = ffk::first_order_integral(omega[i], dE[i], dt);
        out[2*i] = v.re;
        out[2*i + 1] = v.im;
    }
}

void ffk_host_first_order_integral_aa(long n, const double* omega, const double* dE, double dt,
                                      double* out) {
    for (long i = 0; i < n; ++i) {
        double sa, ca, sb, cb;
        ffk::sincos_pi(0.5*(omega[i]*dt), &sa, &ca);
        ffk::sincos_pi(0.5*(dE[i]*dt), &sb, &cb);
        ffk::cplx v = ffk::first_order_integral_aa(omega[i], dE[i], dt, sa, ca, sb, cb);
        out[2*i] = v.re;
        out[2*i + 1] = v.im;
    }
}

// J(x, b) of the gradient kernels, from I1(x) and I1 at the ROUNDED sum x + b as they form it
void ffk_host_derivative_integral(long n, const double* x, const double* b, double dt, double* out) {
    for (long i = 0; i < n; ++i) {
        const ffk::cplx i1x = ffk::first_order_integral(x[i], 0.0, dt);
        const ffk::cplx i1xb = ffk::first_order_integral(x[i] + b[i], 0.0, dt);
        ffk::cplx v = ffk::derivative_integral(x[i], b[i], ffk::derivative_integral_rcp(b[i], dt), dt,
                                               i1x, i1xb);
        out[2*i] = v.re;
        out[2*i + 1] = v.im;
    }
}

// I_{ij,mn} = J(a, b) of the second-order kernels, with f(a + b) taken at ab as they take it at fl(W_ij + W_mn)
void ffk_host_second_order_integral(long n, const double* a, const double* b, const double* ab, double dt,
                                    double* out) {
    for (long i = 0; i < n; ++i) {
        ffk::cplx v = ffk::second_order_integral(a[i], b[i], ab[i], dt);
        out[2*i] = v.re;
        out[2*i + 1] = v.im;
    }
}

// theta: below |b dt| < theta the series replaces the divided difference
double ffk_host_derivative_integral_band() { return ffk::kDerivativeIntegralBand; }

// inside the series: |x dt| below which the moments come from their Taylor series
double ffk_host_derivative_integral_taylor() { return ffk::kDerivativeIntegralTaylor; }

}  // extern "C"

// Test-only harness: the host instantiations of ffk_math.h::sin_small and of sincos_small's sine, side by side,
// through a C ABI (tests/test_sin_small_host.py).  Not part of the product library.
#include "ffk_math.h"

extern "C" {

void ffk_host_sin_small(long n, const double* x, double* s) {
    for (long i = 0; i < n; ++i) s[i] = ffk::sin_small(x[i]);
}

void ffk_host_sincos_small_sine(long n, const double* x, double* s) {
    for (long i = 0; i < n; ++i) {
        double c;
        ffk::sincos_small(x[i], &s[i], &c);
    }
}

// the near form of an entry as phased_q reaches it (|x| < thr)
void ffk_host_phased_q_near(long n, const double* x, double dt, double* q) {
    for (long i = 0; i < n; ++i) q[i] = ffk::phased_q_near(x[i], dt);
}

}  // extern "C"

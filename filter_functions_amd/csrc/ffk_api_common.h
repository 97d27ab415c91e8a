// ffk_api_common.h -- what the translation units of the extern "C" surface (ffk_api*.hip) share:
// error reporting, argument checks, the bump allocator over workspaces, the process-wide staging
// arena and the one scoped object through which the host-pointer entry points use it (StagedCall),
// the shape of a spectrum, workspace layouts used by more than one family of entry points.
//
//   ffk_api.hip           device / stream utilities, diagonalize, control matrix, filter function,
//                         infidelity, Liouville representation, the fused pipeline pass (SURVEY 8 a)
//   ffk_api_sequence.hip  concatenation rule, decay amplitudes, cumulant function, expm (SURVEY 8 f)
//   ffk_api_resident.hip  resident results behind PulseSequence / ff.infidelity, the batched, sequence and
//                         process passes on resident handles; host self test
//     ffk_api_gate_table.h  (included by it alone) the gate table that its passes over many sequences share: the
//                         view of their common arguments, checks, layout head, staging, device pointers
//   ffk_api_frozen.hip    second order and gradient (outside SURVEY 8, frozen since round 2)
//   ffk_api_batch.hip     many pulses of one shape in one pass of the pipeline (ffk_pipeline_batch_dev)
//   ffk_api_batch_grad.hip  the gradient of the filter function / infidelity of many pulses in one pass
//   ffk_api_batch_second.hip  the frequency shifts of many pulses in one pass, without F2 in memory
//   ffk_api_periodic.hip  periodic driving: many pulses at many repeat counts in one pass
#pragma once
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "ffk.h"
#include "ffk_internal.h"

#if defined(FFK_HOST_SANITIZE)
// Host-side sanitizer variant (make VARIANT=asan ...; tools/build_asan.sh): the allocation calls of
// the arena and of the block pools go to the C heap, so that their bookkeeping -- growth, reuse,
// eviction, the slicing of every workspace layout -- can run under AddressSanitizer / UBSan on a
// machine without a GPU (ffk_selftest_host below).  Never part of the shipped library.
#include <cstdlib>
namespace {
hipError_t stub_alloc(void** p, size_t n) {
    *p = std::malloc(n ? n : 1);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t stub_free(void* p) {
    std::free(p);
    return hipSuccess;
}
}  // namespace
#define hipMalloc(p, n) stub_alloc(reinterpret_cast<void**>(p), (n))
#define hipHostMalloc(p, n, flags) stub_alloc(reinterpret_cast<void**>(p), (n))
#define hipFree(p) stub_free(p)
#define hipHostFree(p) stub_free(p)
#define hipGetDevice(d) ((*(d) = 0), hipSuccess)
#define hipSetDevice(d) hipSuccess
#define hipDeviceSynchronize() hipSuccess
// the arena is on the C heap here, so what StagedCall copies to and from it is a plain copy (tools/check_staged_call.hip)
#define hipMemcpyAsync(dst, src, n, kind, stream) (std::memcpy((dst), (src), (n)), hipSuccess)
#define hipStreamSynchronize(stream) hipSuccess
#endif

using ffk::align_up;
using ffk::cplx;

namespace ffk_api {
using ffk::align_up;
using ffk::cplx;

extern thread_local std::string g_error;
extern thread_local ffk_stats g_stats;
// bumped by every call that changes how a pass is enqueued (tuning knobs, instrumentation events):
// captured passes are keyed on it (resident_pass)
extern std::atomic<unsigned long long> g_knob_epoch;
extern int g_forced_chunks;
extern thread_local hipEvent_t g_ev_start, g_ev_stop, g_ev_gate;

int fail(int code, const char* fmt, ...);
// the kernels' sticky fault word (ffk::kernel_fault_word, ffk_internal.h), read AFTER a synchronisation:
// FFK_OK, or FFK_EKERNEL with the message set and the word cleared; peek: the raw word
int kernel_fault_status();
int kernel_fault_peek(bool clear);
// at the top of a host-pointer entry point: a fault left by an earlier, never checked asynchronous launch of this
// thread is reported as such (and cleared) instead of being attributed to the call that is about to run
int kernel_fault_stale();
int kernel_fault_slot_for_selftest();


#define FFK_HIP(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(e_ == hipErrorOutOfMemory ? FFK_ENOMEM : FFK_EHIP, "%s failed: %s", \
                        #expr, hipGetErrorString(e_));                                     \
    } while (0)

#define FFK_REQUIRE(cond, ...) \
    do {                       \
        if (!(cond)) return fail(FFK_EINVAL, __VA_ARGS__); \
    } while (0)

inline bool d_ok(int d) { return d >= 2 && d <= FFK_MAX_D; }
// entry points whose kernels are compiled per dimension (see include/ffk.h)
inline bool d_templated_ok(int d) { return d >= 2 && d <= FFK_MAX_D_TEMPLATED; }

// internal flag of ffk_control_matrix_dev: the workspace already holds segtab/Tc/ops (written by
// the fused front end of ffk_pipeline_dev)
constexpr unsigned FFK_INTERNAL_PROLOGUE_DONE = 0x80000000u;
// ... and the compacted basis lists in the expansion workspace (same launch)
constexpr unsigned FFK_INTERNAL_COMPACT_DONE = 0x40000000u;
// What a caller INSIDE the library asks of the device-pointer entry points it is built from (the resident pass of
// ffk_api_resident.hip, ffk_pipeline_dev around its own stages).  Passed down explicitly to the *_impl functions
// below; the extern "C" entry points call them with the defaults.  (Rounds 3-5: seven thread_local variables.)
struct EighControls {
    const ffk::cplx* opers;      // (n_c, d, d), device
    const double* coeffs;        // (n_c, G), device
    int n_c;
};
struct PassOptions {
    // where the fidelity filter function should go if the control matrix's expansion launch can produce it too,
    // and (out) whether it did
    ffk::cplx* fuse_F = nullptr;
    bool fuse_F_done = false;
    // the eigensolver counts flagged segments into this mapped host word (no memset, no counting kernel)
    int* eigh_fail_count = nullptr;
    // the pipeline's Hamiltonian as its summands: the eigensolver kernel sums the control operators itself
    EighControls eigh_controls = {nullptr, nullptr, 0};
    // spectrum and idx of the infidelity integral are in mapped host memory (staged through LDS by the kernel)
    bool infid_spectrum_on_host = false;
};
int diagonalize_dev_impl(const double* hamiltonian, const double* dt, int G, int d, double* eigvals, double* eigvecs,
                         double* propagators, void* workspace, size_t workspace_bytes, void* stream,
                         const PassOptions& opt);
int control_matrix_dev_impl(const double* eigvals, const double* eigvecs, const double* propagators,
                            const double* omega, int W, const double* basis, int N, const double* n_opers, int A,
                            const double* n_coeffs, const double* dt, const double* t, int G, int d, unsigned flags,
                            double* control_matrix, double* noise_operators, void* workspace,
                            size_t workspace_bytes, void* stream, PassOptions& opt);
int infidelity_dev_impl(const double* filter_function, int A, int W, const double* spectrum, int s_ndim,
                        const double* omega, const int32_t* idx, int n_idx, int d, double* infid, void* workspace,
                        size_t workspace_bytes, void* stream, const PassOptions& opt);
int pipeline_dev_impl(const double* hamiltonian, const double* dt, const double* t, int G, int d,
                      const double* omega, int W, const double* basis, int N, const double* n_opers, int A,
                      const double* n_coeffs, const double* spectrum, int s_ndim, const int32_t* idx, int n_idx,
                      double* eigvals, double* eigvecs, double* propagators, double* control_matrix,
                      double* filter_function, double* infid, void* workspace, size_t workspace_bytes,
                      void* stream, PassOptions& opt);

// ffk_api_batch.hip: ffk_pipeline_batch_dev with the integral's dimension given apart (the resident batch pass)
int pipeline_batch_dev_impl(int P, const double* c_opers, int n_cops, const double* c_coeffs, const double* dt,
                            const double* t, int G, int d, const double* omega, int W, const double* basis, int N,
                            const double* n_opers, int A, const double* n_coeffs, const double* spectrum, int s_ndim,
                            const int32_t* idx, int n_idx, int d_infidelity, double* eigvals, double* eigvecs,
                            double* propagators, double* control_matrix, double* filter_function, double* infid,
                            void* workspace, size_t workspace_bytes, void* stream);

// ffk_api_resident.hip, for the passes of other translation units that read resident control matrices in place
// (ffk_api_periodic.hip): where each of n control matrices (A, N, W) lies on `device` -- in its handle (slot < 0: its
// single result, else that member of its pass), or, no handle, NULL: a row of the host table the caller uploads,
// counted in n_host.
int resident_locate_control_matrices(ffk_resident* const* handles, const int32_t* slots, int n, int device, int A,
                                     int N, int W, const char* what, std::vector<const unsigned char*>* at,
                                     int* n_host);

// Scratch from the shared arena is handed to kernels on a non-blocking stream while g_arena.mu is
// held; the lock may only be dropped once that stream has drained -- on EVERY exit path, also the
// early error returns after the first enqueue: the next holder may reuse or reallocate
// the arena.  Declared after the lock_guard, so it runs before the lock is released.
struct StreamDrain {
    hipStream_t stream;
    ~StreamDrain() { (void)hipStreamSynchronize(stream); }
};

// bump allocator over a caller- or arena-provided workspace
struct Bump {
    unsigned char* base;
    size_t size, used = 0;
    Bump(void* p, size_t n) : base(static_cast<unsigned char*>(p)), size(n) {}
    template <typename T>
    T* take(size_t count) {
        const size_t bytes = align_up(count*sizeof(T));
        if (used + bytes > size) return nullptr;
        T* out = reinterpret_cast<T*>(base + used);
        used += bytes;
        return out;
    }
};

// process-wide arena for the host-pointer flavour
struct Arena {
    std::mutex mu;
    void* ptr = nullptr;
    size_t size = 0;
    int device = -1;
};
extern Arena g_arena;
int arena_reserve(size_t bytes, void** out);
// ffk_release_arena
inline int arena_release() {
    std::lock_guard<std::mutex> lock(g_arena.mu);
    if (g_arena.ptr) {
        FFK_HIP(hipDeviceSynchronize());
        FFK_HIP(hipFree(g_arena.ptr));
        g_arena.ptr = nullptr;
        g_arena.size = 0;
    }
    return FFK_OK;
}

// One call of the host-pointer flavour: the only place that locks the arena, reserves, copies and synchronises for
// it.  Declare every array once, in elements of its type -- in() an input, out() scratch or an output, workspace()
// the bytes a *_workspace_bytes query reports -- which records offsets only; stage() reserves their sum and enqueues
// the copies of the inputs on the null stream; operator[] then gives the device pointers; copy_back() enqueues a D2H
// copy and finish() waits for the stream.  Every slice is bounded by what this call declared, whatever size the arena
// has grown to.  From stage() on work may be in flight: the destructor drains the null stream on every return that
// did not reach finish(), before the arena lock (the first member, released last) is dropped -- the StreamDrain rule.
class StagedCall {
public:
    template <typename T>
    struct Slice {
        size_t at = 0, count = 0;
    };
    StagedCall() = default;
    StagedCall(const StagedCall&) = delete;
    StagedCall& operator=(const StagedCall&) = delete;
    ~StagedCall() {
        if (in_flight_) (void)hipStreamSynchronize(nullptr);
    }
    // `count` elements on the device, the first `copied` of them from `host` (which may be NULL: an optional input)
    template <typename T>
    Slice<T> in(const void* host, size_t count, size_t copied) {
        const Slice<T> s = out<T>(count);
        if (host && copied) inputs_.push_back({s.at, host, sizeof(T)*std::min(copied, count)});
        return s;
    }
    template <typename T>
    Slice<T> in(const void* host, size_t count) { return in<T>(host, count, count); }
    template <typename T>
    Slice<T> out(size_t count) { return {put(sizeof(T)*count), count}; }
    // never empty: a callee given zero bytes still gets a pointer of its own
    Slice<unsigned char> workspace(size_t bytes) { return {put(bytes ? bytes : 1), bytes}; }
    int stage() {
        if (int rc = arena_reserve(total_, &base_)) return rc;
        in_flight_ = true;
        for (const Input& i : inputs_)
            FFK_HIP(hipMemcpyAsync(static_cast<unsigned char*>(base_) + i.at, i.host, i.bytes, hipMemcpyHostToDevice,
                                   nullptr));
        return FFK_OK;
    }
    // NULL before stage(), and for a slice that does not lie inside what this call declared
    template <typename T>
    T* operator[](Slice<T> s) const {
        if (!base_ || s.at + sizeof(T)*s.count > total_) return nullptr;
        return reinterpret_cast<T*>(static_cast<unsigned char*>(base_) + s.at);
    }
    // a declared workspace for a callee that slices it itself
    Bump bump(Slice<unsigned char> s) const { return Bump((*this)[s], (*this)[s] ? s.count : 0); }
    int d2h(void* host, const void* device, size_t bytes) {
        FFK_HIP(hipMemcpyAsync(host, device, bytes, hipMemcpyDeviceToHost, nullptr));
        return FFK_OK;
    }
    template <typename T>
    int copy_back(void* host, Slice<T> s) {
        FFK_REQUIRE((*this)[s], "internal: arena too small");
        return d2h(host, (*this)[s], sizeof(T)*s.count);
    }
    int finish() {
        in_flight_ = false;      // drained below, or the stream is in an error state that no second wait would mend
        FFK_HIP(hipStreamSynchronize(nullptr));
        return FFK_OK;
    }
    // ... for the entry points that report the kernels' fault word
    int finish_with_fault_status() {
        if (int rc = finish()) return rc;
        return kernel_fault_status();
    }

private:
    struct Input {
        size_t at;
        const void* host;
        size_t bytes;
    };
    size_t put(size_t bytes) {
        const size_t at = total_;
        total_ += align_up(bytes);
        return at;
    }
    std::lock_guard<std::mutex> lock_{g_arena.mu};
    std::vector<Input> inputs_;
    size_t total_ = 0;
    void* base_ = nullptr;
    bool in_flight_ = false;
};

// the nine arrays that describe a diagonalised pulse and its noise, as every entry point that starts from them stages
// them (complex arrays as pairs of doubles, like the C ABI); basis may be NULL
struct PulseSlices {
    StagedCall::Slice<double> eigvals, eigvecs, propagators, omega, basis, n_opers, n_coeffs, dt, t;
};
inline PulseSlices stage_pulse(StagedCall& c, const double* eigvals, const double* eigvecs, const double* propagators,
                               const double* omega, int W, const double* basis, int N, const double* n_opers, int A,
                               const double* n_coeffs, const double* dt, const double* t, int G, int d) {
    const size_t dd = size_t(d)*d;
    PulseSlices p;
    p.eigvals = c.in<double>(eigvals, size_t(G)*d);
    p.eigvecs = c.in<double>(eigvecs, 2*size_t(G)*dd);
    p.propagators = c.in<double>(propagators, 2*size_t(G + 1)*dd);
    p.omega = c.in<double>(omega, W);
    p.basis = c.in<double>(basis, 2*size_t(N)*dd);
    p.n_opers = c.in<double>(n_opers, 2*size_t(A)*dd);
    p.n_coeffs = c.in<double>(n_coeffs, size_t(A)*G);
    p.dt = c.in<double>(dt, G);
    p.t = c.in<double>(t, size_t(G) + 1);
    return p;
}

// The spectrum of an infidelity integral as the kernels read it: `rows` rows of W c128 values (one for all selected
// noise operators, one each, or one per pair), and the `n_out` integrals it gives per pulse.
struct SpectrumShape {
    size_t rows = 0, n_out = 0;
};
inline SpectrumShape spectrum_shape(int s_ndim, int n_idx) {
    return {s_ndim == 1 ? 1 : (s_ndim == 2 ? size_t(n_idx) : size_t(n_idx)*n_idx),
            s_ndim == 3 ? size_t(n_idx)*n_idx : size_t(n_idx)};
}

// --- workspace layouts ------------------------------------------------------------------------
size_t ctrl_ws_bytes(int W, int N, int A, int G, int d, int chunks);
int max_chunks_for(int W, int A, int G, int d);
double accumulate_flops(int W, int A, int G, int d);
// the geometry fields and the bytes of g_stats for an accumulate launch over G segments (ffk_get_stats)
void record_accumulate_launch(int W, int A, int G, int d, const ffk::AccumGeometry& geo);

// diagonalize workspace: [status: G ints][seg_prop: G d^2][Qloc: (G+1) d^2][totals / scan scratch]
struct DiagWs {
    int* status;
    cplx* seg_prop;
    cplx* qloc;
    void* small;
};
DiagWs slice_diag_ws(void* workspace, size_t bytes, int G, int d);

// ffk_api_sequence.hip: one concatenation of a sequence drawn from T pulses, operands on the device
size_t sequence_scratch_bytes(int G, int d, int A, int N, int W, int which, bool hermitian, bool want_F);
int sequence_on_device(const double* dU, const double* dP, const double* dR, const int32_t* dI,
                       const double* dB, int hermitian_basis, int T, int G, int d, int A, int N, int W,
                       int which, Bump& a, double* control_matrix, double* total_propagator,
                       double* propagators_liouville, double* filter_function, hipStream_t s,
                       double* resident_R = nullptr, double* resident_F = nullptr,
                       const cplx* const* dRtab = nullptr, const double* dTau = nullptr,
                       const double* dOmega = nullptr, double* omega_copy = nullptr);
}  // namespace ffk_api

using namespace ffk_api;

// ffk_api_resident.hip -- resident results: the user-facing PulseSequence.get_filter_function /
// ff.infidelity call with one H2D, one pass of ffk_pipeline_dev and one D2H of the small results
// (R stays in HBM), concatenations that read resident control matrices in place, hipGraph replay
// of repeated passes; and the host-logic self test of the sanitizer build.
#include <thread>

#include "ffk_api_common.h"
#include "ffk_api_gate_table.h"


namespace {

struct Block {
    void* ptr = nullptr;
    size_t size = 0;
    int device = -1;      // device blocks belong to one device; pinned host blocks are portable
};

// Grow-only pools of device and pinned-host blocks: a PulseSequence is short-lived in user code
// (one per gate), hipMalloc / hipHostMalloc cost more than the whole pass at config 2.
struct BlockPool {
    std::mutex mu;
    std::vector<Block> free_blocks;
    bool pinned;
    explicit BlockPool(bool p) : pinned(p) {}
    int take(size_t bytes, int device, Block* out) {
        std::lock_guard<std::mutex> lock(mu);
        int best = -1;
        for (int i = 0; i < int(free_blocks.size()); ++i)
            if (free_blocks[i].size >= bytes && free_blocks[i].size <= 2*bytes + (1 << 16) &&
                (pinned || free_blocks[i].device == device) &&
                (best < 0 || free_blocks[i].size < free_blocks[best].size))
                best = i;
        if (best >= 0) {
            *out = free_blocks[best];
            free_blocks.erase(free_blocks.begin() + best);
            return FFK_OK;
        }
        const size_t want = align_up(bytes, size_t(1) << 16);
        void* p = nullptr;
        if (pinned)
            FFK_HIP(hipHostMalloc(&p, want, hipHostMallocPortable));
        else
            FFK_HIP(hipMalloc(&p, want));
        *out = {p, want, pinned ? -1 : device};
        return FFK_OK;
    }
    void give(Block b) {
        if (!b.ptr) return;
        std::lock_guard<std::mutex> lock(mu);
        if (free_blocks.size() >= 16) {       // bound what an idle process keeps: the OLDEST idle
            const Block old = free_blocks.front();   // block goes (a loop over fresh pulses of one
            free_blocks.erase(free_blocks.begin());  // shape must find its block again even after
            if (pinned) (void)hipHostFree(old.ptr); else (void)hipFree(old.ptr);   // other shapes filled the pool)
        }
        free_blocks.push_back(b);
    }
    int release() {
        std::lock_guard<std::mutex> lock(mu);
        for (Block& b : free_blocks) {
            if (pinned) FFK_HIP(hipHostFree(b.ptr)); else FFK_HIP(hipFree(b.ptr));
        }
        free_blocks.clear();
        return FFK_OK;
    }
};
BlockPool g_dev_pool(false), g_pin_pool(true);

// A pinned block for the duration of one call.  Kernels read and write it as mapped host memory: declare the lease
// BEFORE the arena lock and the StreamDrain, so that the block goes back to the pool only after the stream has drained.
struct PinLease {
    Block block;
    PinLease() = default;
    PinLease(const PinLease&) = delete;
    PinLease& operator=(const PinLease&) = delete;
    ~PinLease() { g_pin_pool.give(block); }
    int take(size_t bytes, int device) { return g_pin_pool.take(bytes, device, &block); }
    unsigned char* ptr() const { return static_cast<unsigned char*>(block.ptr); }
};
// one stream per device for the resident passes, created on first use
std::mutex g_resident_stream_mu;
hipStream_t g_resident_streams[64] = {};

int resident_stream(hipStream_t* out) {
    int dev = 0;
    FFK_HIP(hipGetDevice(&dev));
    FFK_REQUIRE(dev >= 0 && dev < 64, "device index %d out of range", dev);
    std::lock_guard<std::mutex> lock(g_resident_stream_mu);
    if (!g_resident_streams[dev])
        FFK_HIP(hipStreamCreateWithFlags(&g_resident_streams[dev], hipStreamNonBlocking));
    *out = g_resident_streams[dev];
    return FFK_OK;
}

// byte offsets of the arrays inside the device block and (first two groups) the pinned block
struct ResidentLayout {
    size_t H, dt, t, omega, basis, n_opers, n_coeffs, inputs_end;     // one H2D
    size_t D, V, Q, F, status, outputs_end;                            // one D2H
    size_t R, S, idx, infid, end;                                      // device only (+ infid D2H)
};
ResidentLayout resident_layout(int G, int d, int W, int N, int A) {
    ResidentLayout L;
    const size_t dd = size_t(d)*d;
    size_t o = 0;
    auto put = [&o](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
    L.H = put(16*size_t(G)*dd);
    L.dt = put(8*size_t(G));
    L.t = put(8*size_t(G + 1));
    L.omega = put(8*size_t(W));
    L.basis = put(16*size_t(N)*dd);
    L.n_opers = put(16*size_t(A)*dd);
    L.n_coeffs = put(8*size_t(A)*G);
    L.inputs_end = o;
    L.D = put(8*size_t(G)*d);
    L.V = put(16*size_t(G)*dd);
    L.Q = put(16*size_t(G + 1)*dd);
    L.F = put(16*size_t(A)*A*W);
    L.status = put(sizeof(int32_t));
    L.outputs_end = o;
    L.R = put(16*size_t(A)*N*W);
    L.S = put(16*size_t(A)*A*W);          // largest spectrum: (A, A, W) c128
    L.idx = put(sizeof(int32_t)*size_t(A));
    L.infid = put(8*size_t(A)*A);
    L.end = o;
    return L;
}

// `others_ok`: what else the entry point asks of its spectrum arguments (an output array, W >= 2)
int check_spectrum_args(int s_ndim, const int32_t* idx, int n_idx, int A, int d, bool others_ok) {
    FFK_REQUIRE(idx && s_ndim >= 1 && s_ndim <= 3 && n_idx >= 1 && n_idx <= A && d >= 1 && others_ok,
                "bad spectrum arguments");
    for (int i = 0; i < n_idx; ++i)
        FFK_REQUIRE(idx[i] >= 0 && idx[i] < A, "idx[%d] = %d outside [0, %d)", i, idx[i], A);
    return FFK_OK;
}

// the spectrum (n values; a real one widened to c128) and the operator indices into a pinned block
void stage_spectrum(const double* spectrum, bool is_real, size_t n, const int32_t* idx, int n_idx, void* spectrum_at,
                    void* idx_at) {
    double* hs = static_cast<double*>(spectrum_at);
    if (is_real) {
        for (size_t i = 0; i < n; ++i) { hs[2*i] = spectrum[i]; hs[2*i + 1] = 0.0; }
    } else {
        std::memcpy(hs, spectrum, 16*n);
    }
    std::memcpy(idx_at, idx, sizeof(int32_t)*size_t(n_idx));
}

}  // namespace

struct ffk_resident {
    double t_stage = 0, t_enqueue = 0, t_wait = 0;   // seconds, last pass (host clock)
    int device = -1;
    Block dev, pin;
    // What the blocks hold: nothing, the result of one pulse (a single pass, a concatenation with a result), or the
    // members of a batched or sequence pass.  The single-pulse readers serve the first kind only, the batched readers
    // the second only.
    enum Kind { NOTHING, SINGLE, MEMBERS } kind = NOTHING;
    int P = 0;                               // members (1: a single result)
    int d = 0, W = 0, N = 0, A = 0;
    size_t R = 0, F = 0, omega = 0;          // device offsets: control matrices (P, A, N, W), filter functions
                                             // (P, A, A, W), the grid (W)
    // a single result only:
    size_t total_propagator = 0;             // pinned offset of the pulse's total propagator (d, d)
    size_t stage_bytes = 0;                  // pinned bytes from offset 0 that are free after the pass (its inputs):
                                             // where ffk_resident_infidelity stages its spectrum

    void hold(Kind k, int members, int d_, int W_, int N_, int A_, size_t R_, size_t F_, size_t omega_) {
        kind = k; P = members; d = d_; W = W_; N = N_; A = A_; R = R_; F = F_; omega = omega_;
    }
};

namespace {

// Blocks of at least these sizes on `device` for a pass that is about to overwrite the handle: what it held is gone.
int ensure_blocks(ffk_resident* r, int device, size_t device_bytes, size_t pinned_bytes) {
    r->kind = ffk_resident::NOTHING;
    if (r->device == device && r->dev.size >= device_bytes && r->pin.size >= pinned_bytes) return FFK_OK;
    g_dev_pool.give(r->dev);
    g_pin_pool.give(r->pin);
    r->dev = r->pin = Block{};
    if (int rc = g_dev_pool.take(device_bytes, device, &r->dev)) return rc;
    if (int rc = g_pin_pool.take(pinned_bytes, device, &r->pin)) return rc;
    r->device = device;
    return FFK_OK;
}

// the three host clocks behind ffk_resident_timing: staging the inputs, enqueueing, waiting for the stream
struct PassClock {
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    double laps[3] = {0, 0, 0};
    int n = 0;
    void lap() {
        const auto now = std::chrono::steady_clock::now();
        laps[n++] = std::chrono::duration<double>(now - last).count();
        last = now;
    }
    void store(ffk_resident* r) const { r->t_stage = laps[0]; r->t_enqueue = laps[1]; r->t_wait = laps[2]; }
};

int on_owning_device(const ffk_resident* r) {
    int dev = -1;
    FFK_HIP(hipGetDevice(&dev));
    FFK_REQUIRE(dev == r->device, "resident result lives on device %d, current device is %d",
                r->device, dev);
    return FFK_OK;
}

// The device address of the (A, N, W) control matrix of member `slot` of `g` (slot < 0: of its single result), after
// checking that the handle lives on `device`, holds control matrices of that shape (d = 0: of any dimension) and
// holds that member.  `what` number `k` of the call is named in the message.
int member_control_matrix(const ffk_resident* g, int slot, int device, int d, int A, int N, int W, const char* what,
                          int k, const unsigned char** at) {
    FFK_REQUIRE(g->kind != ffk_resident::NOTHING, "%s %d: no resident result in its handle", what, k);
    FFK_REQUIRE(g->device == device, "%s %d lives on device %d, not on device %d", what, k, g->device, device);
    FFK_REQUIRE((d == 0 || g->d == d) && g->A == A && g->N == N && g->W == W,
                "%s %d: shape (d=%d, A=%d, N=%d, W=%d) differs from the expected (d=%d, A=%d, N=%d, W=%d)", what, k,
                g->d, g->A, g->N, g->W, d ? d : g->d, A, N, W);
    if (slot < 0)
        FFK_REQUIRE(g->kind == ffk_resident::SINGLE, "%s %d: its handle holds no single result", what, k);
    else
        FFK_REQUIRE(g->kind == ffk_resident::MEMBERS && slot < g->P, "%s %d: slot %d is no member of its handle", what,
                    k, slot);
    *at = static_cast<const unsigned char*>(g->dev.ptr) + g->R + 16*size_t(A)*N*W*size_t(slot < 0 ? 0 : slot);
    return FFK_OK;
}

// Where each of n control matrices lies on the device: in its handle (member_control_matrix), or -- no handle -- in a
// row of the host table that the pass uploads: left NULL here and counted, placed by place_host_rows
// (ffk_api_gate_table.h).
int locate_control_matrices(ffk_resident* const* handles, const int32_t* slots, int n, int device, int d, int A, int N,
                            int W, const char* what, std::vector<const unsigned char*>* at, int* n_host) {
    at->assign(size_t(n), nullptr);
    *n_host = 0;
    for (int k = 0; k < n; ++k) {
        if (!handles[k])
            ++*n_host;
        else if (int rc = member_control_matrix(handles[k], slots[k], device, d, A, N, W, what, k, &(*at)[k]))
            return rc;
    }
    return FFK_OK;
}
// ... of the gates of a gate table, whose host table is then required
int locate_gates(const GateTable& g, int device, std::vector<const unsigned char*>* at, int* n_host) {
    if (int rc = locate_control_matrices(g.gates, g.slots, g.T, device, g.d, g.A, g.N, g.W, "gate", at, n_host))
        return rc;
    FFK_REQUIRE(*n_host == 0 || g.gate_table, "gate_table is NULL but %d gate(s) have no handle", *n_host);
    return FFK_OK;
}

}  // namespace

int ffk_api::resident_locate_control_matrices(ffk_resident* const* handles, const int32_t* slots, int n, int device,
                                              int A, int N, int W, const char* what,
                                              std::vector<const unsigned char*>* at, int* n_host) {
    return locate_control_matrices(handles, slots, n, device, 0, A, N, W, what, at, n_host);
}

extern "C" {

int ffk_resident_create(ffk_resident** out) {
    FFK_REQUIRE(out, "NULL argument");
    *out = new (std::nothrow) ffk_resident();
    FFK_REQUIRE(*out, "out of host memory");
    return FFK_OK;
}

int ffk_resident_destroy(ffk_resident* r) {
    if (!r) return FFK_OK;
    g_dev_pool.give(r->dev);
    g_pin_pool.give(r->pin);
    delete r;
    return FFK_OK;
}

int ffk_resident_release_pools(void) {
    if (int rc = g_dev_pool.release()) return rc;
    return g_pin_pool.release();
}

}  // extern "C"

namespace {

// H[g] = sum_i c_coeffs[i, g] c_opers[i]  (pulse_sequence.py:1300-1302, 'ijk,il->ljk'), summed in
// operator order
__global__ void assemble_hamiltonian_kernel(const cplx* __restrict__ opers, const double* __restrict__ coeffs,
                                            int n_c, int G, int dd, cplx* __restrict__ H) {
    const size_t e = static_cast<size_t>(blockIdx.x)*blockDim.x + threadIdx.x;
    if (e >= static_cast<size_t>(G)*dd) return;
    const int g = static_cast<int>(e / dd), k = static_cast<int>(e % dd);
    cplx acc = {0.0, 0.0};
    for (int i = 0; i < n_c; ++i) {
        const double c = coeffs[static_cast<size_t>(i)*G + g];
        const cplx o = opers[i*dd + k];
        acc.re = fma(c, o.re, acc.re);
        acc.im = fma(c, o.im, acc.im);
    }
    H[e] = acc;
}

// Captured resident passes.  The user-facing call builds a new PulseSequence (and handle) per pulse,
// but the block pools hand the same device / pinned blocks out again and the arena does not move:
// for a given shape the enqueue is then the SAME sequence of copies and launches on the same
// addresses, call after call.  It is captured once as a hipGraph and replayed with one launch
// (H2D of the packed inputs, up to 7 kernels, D2H of the outputs: 0.037 -> 0.012 ms of host time per
// call at config 2).  Key = everything the enqueue depends on; an entry whose addresses are no
// longer handed out simply never matches again and is evicted in turn (8 entries).
struct ResidentGraphKey {
    int dev, G, d, W, N, A, n_c, on_device;
    int s_ndim, n_idx, d_inf;                        // the integral riding in the pass (0: none)
    int fault_slot;                                  // the capturing thread's fault word is baked into the kernel arguments
    const void *dp, *hp, *ws;
    hipStream_t stream;
    unsigned long long epoch;
    bool operator==(const ResidentGraphKey& o) const {
        return dev == o.dev && G == o.G && d == o.d && W == o.W && N == o.N && A == o.A && n_c == o.n_c &&
               s_ndim == o.s_ndim && n_idx == o.n_idx && d_inf == o.d_inf && fault_slot == o.fault_slot &&
               on_device == o.on_device && dp == o.dp && hp == o.hp && ws == o.ws && stream == o.stream &&
               epoch == o.epoch;
    }
};
struct ResidentGraph {
    ResidentGraphKey key;
    hipGraphExec_t exec = nullptr;
    ffk_stats stats;
    unsigned long long used = 0;
};
constexpr int kResidentGraphs = 8;
ResidentGraph g_resident_graphs[kResidentGraphs];     // guarded by g_arena.mu (held by resident_pass)
unsigned long long g_resident_graph_clock = 0;
// A pass is captured on the SECOND sighting of its key only: the key contains the pool blocks'
// addresses, and a caller that keeps its pulses alive (a gate set, a list of pulses) never gets the
// same blocks back -- every call would pay capture + instantiate + destroy and evict the graphs
// that do repeat.  The first sighting is enqueued call by call and remembered here.
constexpr int kResidentSeen = 32;
ResidentGraphKey g_resident_seen[kResidentSeen];
bool g_resident_seen_valid[kResidentSeen] = {};
int g_resident_seen_next = 0;
bool resident_key_seen_before(const ResidentGraphKey& key) {
    for (int i = 0; i < kResidentSeen; ++i)
        if (g_resident_seen_valid[i] && g_resident_seen[i] == key) return true;
    g_resident_seen[g_resident_seen_next] = key;
    g_resident_seen_valid[g_resident_seen_next] = true;
    g_resident_seen_next = (g_resident_seen_next + 1) % kResidentSeen;
    return false;
}
bool resident_graphs_enabled() {
    static const bool on = [] {
        const char* e = std::getenv("FFK_RESIDENT_GRAPH");
        return e == nullptr || e[0] != '0';
    }();
    return on;
}

// One resident pass; the Hamiltonian either given (G, d, d) or as control operators and
// amplitudes, in which case only the amplitudes cross PCIe (8 n_c B per segment instead of
// 16 d^2) and the sum runs on the device.
// Optionally the infidelity integral rides in the same pass (spectrum != NULL): ff.infidelity on a
// pulse with nothing cached is then ONE round trip to the device instead of two.
int resident_pass(ffk_resident* r, const double* hamiltonian, const double* c_opers, int n_c,
                  const double* c_coeffs, const double* dt, const double* t, int G, int d,
                  const double* omega, int W, const double* basis, int N, const double* n_opers, int A,
                  const double* n_coeffs, double** eigvals, double** eigvecs, double** propagators,
                  double** filter_function, const double* spectrum = nullptr, int s_ndim = 0,
                  int spectrum_is_real = 0, const int32_t* idx = nullptr, int n_idx = 0, int d_inf = 0,
                  double* infid = nullptr) {
    FFK_REQUIRE(r, "NULL handle");
    FFK_REQUIRE(d_templated_ok(d), "unsupported dimension d=%d (need 2 <= d <= %d)", d, FFK_MAX_D_TEMPLATED);
    FFK_REQUIRE(W >= 1 && N >= 1 && A >= 1 && G >= 1, "empty axis: W=%d N=%d A=%d G=%d", W, N, A, G);
    FFK_REQUIRE(hamiltonian || (c_opers && c_coeffs && n_c >= 1), "NULL argument");
    FFK_REQUIRE(dt && t && omega && basis && n_opers && n_coeffs, "NULL argument");
    FFK_REQUIRE(eigvals && eigvecs && propagators && filter_function, "NULL output argument");
    if (spectrum)
        if (int rc = check_spectrum_args(s_ndim, idx, n_idx, A, d_inf, infid && W >= 2)) return rc;
    int dev = 0;
    FFK_HIP(hipGetDevice(&dev));
    const ResidentLayout L = resident_layout(G, d, W, N, A);
    // spectrum (as c128), idx and the integrals live behind the outputs in the pinned block: the kernel
    // reads and writes them there (mapped memory), nothing extra crosses PCIe by copy
    const SpectrumShape sh = spectrum ? spectrum_shape(s_ndim, n_idx) : SpectrumShape{};
    size_t o_spec = 0, o_idx = 0, o_out = 0, pin_need = L.outputs_end;
    if (spectrum) {
        o_spec = align_up(L.outputs_end);
        o_idx = o_spec + align_up(16*sh.rows*W);
        o_out = o_idx + align_up(sizeof(int32_t)*size_t(n_idx));
        pin_need = o_out + align_up(8*sh.n_out);
    }
    if (int rc = ensure_blocks(r, dev, L.end, pin_need)) return rc;
    unsigned char* hp = static_cast<unsigned char*>(r->pin.ptr);
    unsigned char* dp = static_cast<unsigned char*>(r->dev.ptr);
    const size_t dd = size_t(d)*d;
    PassClock clock;
    // controls travel in the slot of the Hamiltonian they replace (if they fit: always, but for
    // one- or two-segment pulses with many control operators, which are summed here instead)
    const size_t ctrl_opers = 16*size_t(hamiltonian ? 0 : n_c)*dd;
    const size_t ctrl_bytes = ctrl_opers + 8*size_t(hamiltonian ? 0 : n_c)*G;
    const bool on_device = !hamiltonian && ctrl_bytes <= 16*size_t(G)*dd;
    if (hamiltonian) {
        std::memcpy(hp + L.H, hamiltonian, 16*size_t(G)*dd);
    } else if (on_device) {
        std::memcpy(hp + L.H, c_opers, ctrl_opers);
        std::memcpy(hp + L.H + ctrl_opers, c_coeffs, 8*size_t(n_c)*G);
    } else {
        double* H = reinterpret_cast<double*>(hp + L.H);
        for (int g = 0; g < G; ++g)
            for (size_t k = 0; k < dd; ++k) {
                double re = 0.0, im = 0.0;
                for (int i = 0; i < n_c; ++i) {
                    const double c = c_coeffs[size_t(i)*G + g];
                    re = std::fma(c, c_opers[2*(i*dd + k)], re);
                    im = std::fma(c, c_opers[2*(i*dd + k) + 1], im);
                }
                H[2*(g*dd + k)] = re;
                H[2*(g*dd + k) + 1] = im;
            }
    }
    std::memcpy(hp + L.dt, dt, 8*size_t(G));
    std::memcpy(hp + L.t, t, 8*size_t(G + 1));
    std::memcpy(hp + L.omega, omega, 8*size_t(W));
    std::memcpy(hp + L.basis, basis, 16*size_t(N)*dd);
    std::memcpy(hp + L.n_opers, n_opers, 16*size_t(A)*dd);
    std::memcpy(hp + L.n_coeffs, n_coeffs, 8*size_t(A)*G);
    if (spectrum) stage_spectrum(spectrum, spectrum_is_real != 0, sh.rows*W, idx, n_idx, hp + o_spec, hp + o_idx);
    hipStream_t s;
    if (int rc = resident_stream(&s)) return rc;
    // scratch of the pass from the shared arena (held only for the duration of this call)
    std::lock_guard<std::mutex> lock(g_arena.mu);
    const size_t wsb = ffk_pipeline_workspace_bytes(W, N, A, G, d, 0, 0);
    const size_t hsb = on_device ? align_up(16*size_t(G)*dd) : 0;
    const size_t iwsb = spectrum ? align_up(ffk_infidelity_workspace_bytes(W, n_idx, s_ndim)) : 0;
    void* ws;
    if (int rc = arena_reserve(wsb + hsb + iwsb, &ws)) return rc;
    StreamDrain drain{s};      // (the successful path has synchronised already: a no-op then)
    clock.lap();
    auto dptr = [dp](size_t off) { return reinterpret_cast<double*>(dp + off); };
    const bool count_on_host = ffk::eigh_fail_count_supported(d) && ffk::use_fused_front(G, d);
    // copies in, kernels, copies out: on `s`, no synchronisation
    auto enqueue = [&]() -> int {
        const double* Hdev = dptr(L.H);
        const bool sum_in_eigensolver = on_device && count_on_host;     // (compiled d, fused front)
        if (on_device && !sum_in_eigensolver) {
            // the controls first, so that the sum runs while the rest of the inputs is still in flight
            FFK_HIP(hipMemcpyAsync(dp + L.H, hp + L.H, ctrl_bytes, hipMemcpyHostToDevice, s));
            cplx* Hsum = reinterpret_cast<cplx*>(static_cast<unsigned char*>(ws) + wsb);
            const size_t n = size_t(G)*dd;
            hipLaunchKernelGGL(assemble_hamiltonian_kernel, dim3(static_cast<unsigned>((n + 255)/256)), dim3(256),
                               0, s, reinterpret_cast<const cplx*>(dp + L.H),
                               reinterpret_cast<const double*>(dp + L.H + ctrl_opers), n_c, G, d*d, Hsum);
            FFK_HIP(hipGetLastError());
            FFK_HIP(hipMemcpyAsync(dp + L.dt, hp + L.dt, L.inputs_end - L.dt, hipMemcpyHostToDevice, s));
            Hdev = reinterpret_cast<const double*>(Hsum);
        } else {
            // one copy; with the controls in the Hamiltonian's slot the eigensolver sums them itself
            FFK_HIP(hipMemcpyAsync(dp, hp, L.inputs_end, hipMemcpyHostToDevice, s));
        }
        PassOptions opt;
        if (sum_in_eigensolver)
            opt.eigh_controls = {reinterpret_cast<const cplx*>(dp + L.H),
                                 reinterpret_cast<const double*>(dp + L.H + ctrl_opers), n_c};
        // the eigensolver counts its flagged segments straight into the pinned block's status word (zeroed below,
        // before the launch): no memset, no counting kernel, and the word stays out of the copy back
        opt.eigh_fail_count = count_on_host ? reinterpret_cast<int*>(hp + L.status) : nullptr;
        if (int rc = pipeline_dev_impl(Hdev, dptr(L.dt), dptr(L.t), G, d, dptr(L.omega), W, dptr(L.basis), N,
                                       dptr(L.n_opers), A, dptr(L.n_coeffs), nullptr, 0, nullptr, 0, dptr(L.D),
                                       dptr(L.V), dptr(L.Q), dptr(L.R), dptr(L.F), nullptr, ws, wsb, s, opt))
            return rc;
        if (!count_on_host)
            if (int rc = ffk_eigensolver_status_dev(ws, wsb, G, d, reinterpret_cast<int32_t*>(dp + L.status), s))
                return rc;
        if (spectrum) {
            opt.infid_spectrum_on_host = true;     // spectrum and idx are read from the pinned block
            if (int rc = infidelity_dev_impl(dptr(L.F), A, W, reinterpret_cast<const double*>(hp + o_spec), s_ndim,
                                             dptr(L.omega), reinterpret_cast<const int32_t*>(hp + o_idx), n_idx,
                                             d_inf, reinterpret_cast<double*>(hp + o_out),
                                             static_cast<unsigned char*>(ws) + wsb + hsb, iwsb, s, opt))
                return rc;
        }
        FFK_HIP(hipMemcpyAsync(hp + L.D, dp + L.D, (count_on_host ? L.status : L.outputs_end) - L.D,
                               hipMemcpyDeviceToHost, s));
        return FFK_OK;
    };
    if (count_on_host) *reinterpret_cast<volatile int32_t*>(hp + L.status) = 0;
    const ResidentGraphKey key{dev, G, d, W, N, A, hamiltonian ? 0 : n_c, on_device ? 1 : 0,
                               spectrum ? s_ndim : 0, spectrum ? n_idx : 0, spectrum ? d_inf : 0,
                               kernel_fault_slot_for_selftest(), dp, hp, ws, s, g_knob_epoch.load()};
    ResidentGraph* hit = nullptr;
    ResidentGraph* victim = &g_resident_graphs[0];
    if (resident_graphs_enabled()) {
        for (ResidentGraph& e : g_resident_graphs) {
            if (e.exec && e.key == key) hit = &e;
            if (e.used < victim->used) victim = &e;
        }
    }
    bool enqueued = false;
    if (hit) {
        if (hipGraphLaunch(hit->exec, s) == hipSuccess) {
            hit->used = ++g_resident_graph_clock;
            g_stats = hit->stats;
            enqueued = true;
        } else {
            (void)hipGetLastError();
            (void)hipGraphExecDestroy(hit->exec);
            hit->exec = nullptr;
            hit->used = 0;
        }
    } else if (resident_graphs_enabled() && resident_key_seen_before(key) &&
               hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) == hipSuccess) {
        // second pass of this shape on these blocks: capture it, then launch the capture
        const int rc = enqueue();
        hipGraph_t graph = nullptr;
        const hipError_t ce = hipStreamEndCapture(s, &graph);
        if (rc != FFK_OK) {
            if (graph) (void)hipGraphDestroy(graph);
            (void)hipGetLastError();
            return rc;
        }
        hipGraphExec_t exec = nullptr;
        if (ce == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess &&
            hipGraphLaunch(exec, s) == hipSuccess) {
            if (victim->exec) (void)hipGraphExecDestroy(victim->exec);
            victim->key = key;
            victim->exec = exec;
            victim->stats = g_stats;
            victim->used = ++g_resident_graph_clock;
            enqueued = true;
        } else {
            if (exec) (void)hipGraphExecDestroy(exec);
            (void)hipGetLastError();
        }
        if (graph) (void)hipGraphDestroy(graph);
    } else {
        (void)hipGetLastError();
    }
    if (!enqueued)
        if (int rc = enqueue()) return rc;
    clock.lap();
    FFK_HIP(hipStreamSynchronize(s));
    clock.lap();
    clock.store(r);
    const int32_t failed = *reinterpret_cast<const int32_t*>(hp + L.status);
    if (failed != 0)
        return fail(FFK_ENOCONV, "Jacobi eigensolver did not converge for %d segment(s)", int(failed));
    if (int rc = kernel_fault_status()) return rc;
    *eigvals = reinterpret_cast<double*>(hp + L.D);
    *eigvecs = reinterpret_cast<double*>(hp + L.V);
    *propagators = reinterpret_cast<double*>(hp + L.Q);
    *filter_function = reinterpret_cast<double*>(hp + L.F);
    if (spectrum) std::memcpy(infid, hp + o_out, 8*sh.n_out);
    r->hold(ffk_resident::SINGLE, 1, d, W, N, A, L.R, L.F, L.omega);
    r->total_propagator = L.Q + 16*size_t(G)*dd;
    r->stage_bytes = L.inputs_end;
    return FFK_OK;
}

}  // namespace

extern "C" {

int ffk_resident_filter_function_infidelity(ffk_resident* r, const double* c_opers, int n_cops,
                                            const double* c_coeffs, const double* dt, const double* t, int G,
                                            int d, const double* omega, int W, const double* basis, int N,
                                            const double* n_opers, int A, const double* n_coeffs,
                                            const double* spectrum, int s_ndim, int spectrum_is_real,
                                            const int32_t* idx, int n_idx, int d_infidelity, double** eigvals,
                                            double** eigvecs, double** propagators, double** filter_function,
                                            double* infidelity) {
    FFK_REQUIRE(spectrum && idx && infidelity, "NULL argument");
    return resident_pass(r, nullptr, c_opers, n_cops, c_coeffs, dt, t, G, d, omega, W, basis, N, n_opers, A,
                         n_coeffs, eigvals, eigvecs, propagators, filter_function, spectrum, s_ndim,
                         spectrum_is_real, idx, n_idx, d_infidelity, infidelity);
}

int ffk_resident_filter_function(ffk_resident* r, const double* hamiltonian, const double* dt,
                                 const double* t, int G, int d, const double* omega, int W,
                                 const double* basis, int N, const double* n_opers, int A,
                                 const double* n_coeffs, double** eigvals, double** eigvecs,
                                 double** propagators, double** filter_function) {
    FFK_REQUIRE(hamiltonian, "NULL argument");
    return resident_pass(r, hamiltonian, nullptr, 0, nullptr, dt, t, G, d, omega, W, basis, N, n_opers, A,
                         n_coeffs, eigvals, eigvecs, propagators, filter_function);
}

int ffk_resident_filter_function_from_controls(ffk_resident* r, const double* c_opers, int n_cops,
                                               const double* c_coeffs, const double* dt,
                                               const double* t, int G, int d, const double* omega,
                                               int W, const double* basis, int N,
                                               const double* n_opers, int A, const double* n_coeffs,
                                               double** eigvals, double** eigvecs,
                                               double** propagators, double** filter_function) {
    FFK_REQUIRE(c_opers && c_coeffs && n_cops >= 1, "NULL or empty control Hamiltonian");
    return resident_pass(r, nullptr, c_opers, n_cops, c_coeffs, dt, t, G, d, omega, W, basis, N, n_opers, A,
                         n_coeffs, eigvals, eigvecs, propagators, filter_function);
}

int ffk_resident_timing(ffk_resident* r, double* seconds) {
    FFK_REQUIRE(r && seconds, "NULL argument");
    seconds[0] = r->t_stage;
    seconds[1] = r->t_enqueue;
    seconds[2] = r->t_wait;
    return FFK_OK;
}


// ffk_concatenate_sequence for distinct pulses whose control matrices are still resident (every one
// evaluated by ffk_resident_filter_function* on the same frequency grid): the table is assembled
// by device-to-device copies, the total propagators come from the handles' host blocks, the total
// phase factors exp(i omega tau_k) are formed on the device -- per call only index, basis and tau
// cross PCIe.  With `result` (which = 0, filter_function wanted) the summed control matrix, its filter
// function and the grid STAY in that handle (control_matrix may then be NULL): the new pulse is as
// resident as its parts -- ffk_resident_control_matrix / _infidelity serve it, and it can be an
// input of the next concatenation.
int ffk_concatenate_sequence_resident(ffk_resident* const* pulses, const double* tau,
                                      const int32_t* index, const double* basis, int hermitian_basis,
                                      int T, int G, int which, double* control_matrix,
                                      double* total_propagator, double* propagators_liouville,
                                      double* filter_function, ffk_resident* result) {
    FFK_REQUIRE(pulses && tau && index && basis && total_propagator, "NULL argument");
    FFK_REQUIRE(control_matrix || result, "NULL argument");
    FFK_REQUIRE(!result || (which == 0 && filter_function), "a resident result holds the summed control "
                "matrix and its filter function");
    for (int k = 0; result && k < T; ++k) FFK_REQUIRE(pulses[k] != result, "result must not be an input");
    FFK_REQUIRE(T >= 1 && T <= 65535 && G >= 1, "empty or oversized axis: T=%d G=%d", T, G);
    FFK_REQUIRE(which == 0 || which == 1, "invalid which=%d", which);
    FFK_REQUIRE(!filter_function || which == 0, "the filter function needs the summed control matrix");
    FFK_REQUIRE(pulses[0], "pulse 0 has no resident result");
    const ffk_resident* first = pulses[0];
    const int d = first->d, A = first->A, N = first->N, W = first->W;
    std::vector<const unsigned char*> tab(T);        // the control matrices are read where they lie
    for (int k = 0; k < T; ++k) {
        FFK_REQUIRE(pulses[k], "pulse %d has no resident result", k);
        if (int rc = member_control_matrix(pulses[k], -1, first->device, d, A, N, W, "pulse", k, &tab[k])) return rc;
    }
    for (int g = 0; g < G; ++g)
        FFK_REQUIRE(index[g] >= 0 && index[g] < T, "index[%d] = %d outside [0, %d)", g, index[g], T);
    if (int rc = on_owning_device(first)) return rc;
    hipStream_t s;
    if (int rc = resident_stream(&s)) return rc;
    const size_t dd = size_t(d)*d;
    const size_t nU = 16*size_t(T)*dd, nP = 16*size_t(T)*W, nI = 4*size_t(G);
    const size_t nB = 16*size_t(N)*dd, nT = 8*size_t(T), nX = 8*size_t(T);
    // host staging (propagators | tau | index | basis | pointers to the resident control matrices) in
    // one pinned block, one H2D.  The control matrices are read where they lie (round 3: assembling
    // a contiguous table cost T device-to-device copies per call, 24 of ~0.5 MB at config 3)
    const size_t oU = 0, oT = oU + align_up(nU), oI = oT + align_up(nT), oB = oI + align_up(nI);
    const size_t oX = oB + align_up(nB);
    const size_t stage = oX + align_up(nX);
    PinLease pin;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    if (int rc = pin.take(stage, first->device)) return rc;
    unsigned char* hp = pin.ptr();
    for (int k = 0; k < T; ++k)         // the pulses' total propagators
        std::memcpy(hp + oU + 16*size_t(k)*dd,
                    static_cast<const unsigned char*>(pulses[k]->pin.ptr) + pulses[k]->total_propagator, 16*dd);
    std::memcpy(hp + oT, tau, nT);
    std::memcpy(hp + oI, index, nI);
    std::memcpy(hp + oB, basis, nB);
    std::memcpy(hp + oX, tab.data(), nX);
    void* base;
    if (int rc = arena_reserve(stage + align_up(nP) +
                               sequence_scratch_bytes(G, d, A, N, W, which, hermitian_basis != 0,
                                                      filter_function != nullptr), &base))
        return rc;
    Bump a(base, g_arena.size);
    unsigned char* dS = a.take<unsigned char>(stage);
    double* dP = a.take<double>(nP/8);
    // a result handle takes the layout of a one-segment pass: R, F and the grid in its device block,
    // (identity, total propagator) where the propagators of a pass sit in its host block
    const ResidentLayout RL = resident_layout(1, d, W, N, A);
    double *keep_R = nullptr, *keep_F = nullptr, *omega_copy = nullptr;
    if (result) {
        if (int rc = ensure_blocks(result, first->device, RL.end, RL.outputs_end)) return rc;
        unsigned char* rp = static_cast<unsigned char*>(result->dev.ptr);
        keep_R = reinterpret_cast<double*>(rp + RL.R);
        keep_F = reinterpret_cast<double*>(rp + RL.F);
        omega_copy = reinterpret_cast<double*>(rp + RL.omega);
    }
    StreamDrain drain{s};
    FFK_HIP(hipMemcpyAsync(dS, hp, stage, hipMemcpyHostToDevice, s));
    const double* dOmega = reinterpret_cast<const double*>(static_cast<const unsigned char*>(first->dev.ptr) +
                                                           first->omega);
    if (int rc = sequence_on_device(reinterpret_cast<const double*>(dS + oU), dP, nullptr,
                                    reinterpret_cast<const int32_t*>(dS + oI),
                                    reinterpret_cast<const double*>(dS + oB), hermitian_basis, T, G, d, A, N, W,
                                    which, a, control_matrix, total_propagator, propagators_liouville,
                                    filter_function, s, keep_R, keep_F,
                                    reinterpret_cast<const cplx* const*>(dS + oX),
                                    reinterpret_cast<const double*>(dS + oT), dOmega, omega_copy))
        return rc;
    FFK_HIP(hipStreamSynchronize(s));
    if (result) {
        double* q = reinterpret_cast<double*>(static_cast<unsigned char*>(result->pin.ptr) + RL.Q);
        for (size_t e = 0; e < dd; ++e) {
            q[2*e] = (e / d == e % d) ? 1.0 : 0.0;
            q[2*e + 1] = 0.0;
        }
        std::memcpy(q + 2*dd, total_propagator, 16*dd);
        result->t_stage = result->t_enqueue = result->t_wait = 0.0;
        result->hold(ffk_resident::SINGLE, 1, d, W, N, A, RL.R, RL.F, RL.omega);
        result->total_propagator = RL.Q + 16*dd;
        result->stage_bytes = RL.inputs_end;
    }
    return FFK_OK;
}

namespace {
// member `slot` (slot < 0: the single result) of the handle's control matrices, copied to the host
int read_control_matrix(const ffk_resident* r, int slot, double* control_matrix) {
    FFK_REQUIRE(control_matrix, "NULL argument");
    const unsigned char* at;
    if (int rc = member_control_matrix(r, slot, r->device, r->d, r->A, r->N, r->W, "member", slot, &at)) return rc;
    if (int rc = on_owning_device(r)) return rc;
    hipStream_t s;
    if (int rc = resident_stream(&s)) return rc;
    FFK_HIP(hipMemcpyAsync(control_matrix, at, 16*size_t(r->A)*r->N*r->W, hipMemcpyDeviceToHost, s));
    FFK_HIP(hipStreamSynchronize(s));
    return FFK_OK;
}
}  // namespace

int ffk_resident_control_matrix(ffk_resident* r, double* control_matrix) {
    FFK_REQUIRE(r && r->kind == ffk_resident::SINGLE, "no resident result");
    return read_control_matrix(r, -1, control_matrix);
}

int ffk_resident_batch_control_matrix(ffk_resident* r, int pulse, double* control_matrix) {
    FFK_REQUIRE(r && r->kind == ffk_resident::MEMBERS, "no resident batch result");
    FFK_REQUIRE(pulse >= 0 && pulse < r->P, "pulse %d out of range [0, %d)", pulse, r->P);
    return read_control_matrix(r, pulse, control_matrix);
}

namespace {

// the batched pass: [inputs: one H2D][outputs: one D2H] in both blocks, then the control matrices on the device only
struct BatchLayout {
    size_t c_opers, c_coeffs, dt, t, omega, basis, n_opers, n_coeffs, S, idx, inputs_end;
    size_t D, V, Q, F, infid, failed, outputs_end;
    size_t R, end;
};
BatchLayout batch_layout(int P, int n_c, int G, int d, int W, int N, int A, SpectrumShape sh, int n_idx) {
    BatchLayout L;
    const size_t dd = size_t(d)*d, PG = size_t(P)*G;
    size_t o = 0;
    auto put = [&o](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
    L.c_opers = put(16*size_t(P)*n_c*dd);
    L.c_coeffs = put(8*size_t(P)*n_c*G);
    L.dt = put(8*PG);
    L.t = put(8*size_t(P)*(G + 1));
    L.omega = put(8*size_t(W));
    L.basis = put(16*size_t(N)*dd);
    L.n_opers = put(16*size_t(P)*A*dd);
    L.n_coeffs = put(8*size_t(P)*A*G);
    L.S = put(16*sh.rows*W);
    L.idx = put(sizeof(int32_t)*size_t(n_idx));
    L.inputs_end = o;
    L.D = put(8*PG*d);
    L.V = put(16*PG*dd);
    L.Q = put(16*size_t(P)*(G + 1)*dd);
    L.F = put(16*size_t(P)*A*A*W);
    L.infid = put(8*size_t(P)*sh.n_out);
    L.failed = put(sizeof(int32_t)*P);
    L.outputs_end = o;
    L.R = put(16*size_t(P)*A*N*W);
    L.end = o;
    return L;
}

}  // namespace

int ffk_resident_batch_filter_function_infidelity(ffk_resident* r, int P, const double* c_opers, int n_c,
                                                  const double* c_coeffs, const double* dt, const double* t, int G,
                                                  int d, const double* omega, int W, const double* basis, int N,
                                                  const double* n_opers, int A, const double* n_coeffs,
                                                  const double* spectrum, int s_ndim, int spectrum_is_real,
                                                  const int32_t* idx, int n_idx, int d_inf, double** eigvals,
                                                  double** eigvecs, double** propagators, double** filter_function,
                                                  double* infid, int32_t* n_failed) {
    FFK_REQUIRE(r, "NULL handle");
    FFK_REQUIRE(P >= 1 && P <= 65535, "need 1 <= P <= 65535 pulses, got P=%d", P);
    FFK_REQUIRE(d_templated_ok(d), "unsupported dimension d=%d (need 2 <= d <= %d)", d, FFK_MAX_D_TEMPLATED);
    FFK_REQUIRE(W >= 1 && N >= 1 && A >= 1 && G >= 1 && n_c >= 1, "empty axis: W=%d N=%d A=%d G=%d n_cops=%d", W, N,
                A, G, n_c);
    FFK_REQUIRE(c_opers && c_coeffs && dt && t && omega && basis && n_opers && n_coeffs, "NULL argument");
    FFK_REQUIRE(eigvals && eigvecs && propagators && filter_function && n_failed, "NULL output argument");
    if (spectrum)
        if (int rc = check_spectrum_args(s_ndim, idx, n_idx, A, d_inf, infid && W >= 2)) return rc;
    const SpectrumShape sh = spectrum ? spectrum_shape(s_ndim, n_idx) : SpectrumShape{};
    int dev = 0;
    FFK_HIP(hipGetDevice(&dev));
    const size_t dd = size_t(d)*d, PG = size_t(P)*G;
    const BatchLayout L = batch_layout(P, n_c, G, d, W, N, A, sh, n_idx);
    if (int rc = ensure_blocks(r, dev, L.end, L.outputs_end)) return rc;
    unsigned char* hp = static_cast<unsigned char*>(r->pin.ptr);
    unsigned char* dp = static_cast<unsigned char*>(r->dev.ptr);
    PassClock clock;
    std::memcpy(hp + L.c_opers, c_opers, 16*size_t(P)*n_c*dd);
    std::memcpy(hp + L.c_coeffs, c_coeffs, 8*size_t(P)*n_c*G);
    std::memcpy(hp + L.dt, dt, 8*PG);
    std::memcpy(hp + L.t, t, 8*size_t(P)*(G + 1));
    std::memcpy(hp + L.omega, omega, 8*size_t(W));
    std::memcpy(hp + L.basis, basis, 16*size_t(N)*dd);
    std::memcpy(hp + L.n_opers, n_opers, 16*size_t(P)*A*dd);
    std::memcpy(hp + L.n_coeffs, n_coeffs, 8*size_t(P)*A*G);
    if (spectrum) stage_spectrum(spectrum, spectrum_is_real != 0, sh.rows*W, idx, n_idx, hp + L.S, hp + L.idx);
    hipStream_t s;
    if (int rc = resident_stream(&s)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    const size_t wsb = ffk_pipeline_batch_workspace_bytes(P, W, N, A, G, d, n_idx, s_ndim);
    void* ws;
    if (int rc = arena_reserve(wsb, &ws)) return rc;
    StreamDrain drain{s};
    clock.lap();
    auto dptr = [dp](size_t off) { return reinterpret_cast<double*>(dp + off); };
    FFK_HIP(hipMemcpyAsync(dp, hp, L.inputs_end, hipMemcpyHostToDevice, s));
    if (int rc = pipeline_batch_dev_impl(P, dptr(L.c_opers), n_c, dptr(L.c_coeffs), dptr(L.dt), dptr(L.t), G, d,
                                         dptr(L.omega), W, dptr(L.basis), N, dptr(L.n_opers), A, dptr(L.n_coeffs),
                                         spectrum ? dptr(L.S) : nullptr, s_ndim,
                                         reinterpret_cast<const int32_t*>(dp + L.idx), n_idx, d_inf, dptr(L.D),
                                         dptr(L.V), dptr(L.Q), dptr(L.R), dptr(L.F),
                                         spectrum ? dptr(L.infid) : nullptr, ws, wsb, s))
        return rc;
    if (int rc = ffk_eigensolver_status_batch_dev(ws, wsb, P, G, d, reinterpret_cast<int32_t*>(dp + L.failed), s))
        return rc;
    FFK_HIP(hipMemcpyAsync(hp + L.D, dp + L.D, L.outputs_end - L.D, hipMemcpyDeviceToHost, s));
    clock.lap();
    FFK_HIP(hipStreamSynchronize(s));
    clock.lap();
    clock.store(r);
    if (int rc = kernel_fault_status()) return rc;
    std::memcpy(n_failed, hp + L.failed, sizeof(int32_t)*P);
    for (int p = 0; p < P; ++p)
        if (n_failed[p] != 0)
            return fail(FFK_ENOCONV, "Jacobi eigensolver did not converge for %d segment(s) of pulse %d of the batch",
                        int(n_failed[p]), p);
    *eigvals = reinterpret_cast<double*>(hp + L.D);
    *eigvecs = reinterpret_cast<double*>(hp + L.V);
    *propagators = reinterpret_cast<double*>(hp + L.Q);
    *filter_function = reinterpret_cast<double*>(hp + L.F);
    if (spectrum) std::memcpy(infid, hp + L.infid, 8*size_t(P)*sh.n_out);
    r->hold(ffk_resident::MEMBERS, P, d, W, N, A, L.R, L.F, L.omega);
    return FFK_OK;
}

int ffk_resident_control_matrix_dev(ffk_resident* r, const double** control_matrix,
                                    const double** filter_function, const double** omega) {
    FFK_REQUIRE(r && r->kind == ffk_resident::SINGLE, "no resident result");
    const unsigned char* dp = static_cast<const unsigned char*>(r->dev.ptr);
    if (control_matrix) *control_matrix = reinterpret_cast<const double*>(dp + r->R);
    if (filter_function) *filter_function = reinterpret_cast<const double*>(dp + r->F);
    if (omega) *omega = reinterpret_cast<const double*>(dp + r->omega);
    return FFK_OK;
}

int ffk_resident_infidelity(ffk_resident* r, const double* spectrum, int s_ndim, int spectrum_is_real,
                            const int32_t* idx, int n_idx, int d, double* infid) {
    FFK_REQUIRE(r && r->kind == ffk_resident::SINGLE, "no resident result");
    FFK_REQUIRE(spectrum && idx && infid, "NULL argument");
    if (int rc = check_spectrum_args(s_ndim, idx, n_idx, r->A, d, true)) return rc;
    if (int rc = on_owning_device(r)) return rc;
    const int W = r->W, A = r->A;
    const SpectrumShape sh = spectrum_shape(s_ndim, n_idx);
    unsigned char* dp = static_cast<unsigned char*>(r->dev.ptr);
    // stage spectrum (as c128), idx and the result in the pinned input region (free after the pass).
    // Round 3: the kernel reads spectrum and idx FROM that pinned block and writes the integrals INTO
    // it (pinned host memory is mapped into the device's address space): one launch and one
    // synchronisation instead of two H2D copies, the launch, a D2H copy into pageable memory and
    // the synchronisation -- the spectrum is read once (64 KB over PCIe at config 2)
    const size_t o_idx = align_up(16*sh.rows*W), o_out = o_idx + align_up(sizeof(int32_t)*size_t(n_idx));
    const size_t stage = o_out + align_up(8*sh.n_out);
    hipStream_t s;
    if (int rc = resident_stream(&s)) return rc;
    PinLease extra;                    // a spectrum larger than the pass's inputs gets a block of its own
    unsigned char* stage_ptr = static_cast<unsigned char*>(r->pin.ptr);
    if (stage > r->stage_bytes) {
        if (int rc = extra.take(stage, r->device)) return rc;
        stage_ptr = extra.ptr();
    }
    stage_spectrum(spectrum, spectrum_is_real != 0, sh.rows*W, idx, n_idx, stage_ptr, stage_ptr + o_idx);
    std::lock_guard<std::mutex> lock(g_arena.mu);
    const size_t iwsb = ffk_infidelity_workspace_bytes(W, n_idx, s_ndim);
    void* iws;
    if (int rc = arena_reserve(iwsb, &iws)) return rc;
    StreamDrain drain{s};
    PassOptions opt;
    opt.infid_spectrum_on_host = true;
    if (int rc = infidelity_dev_impl(reinterpret_cast<const double*>(dp + r->F), A, W,
                                     reinterpret_cast<const double*>(stage_ptr), s_ndim,
                                     reinterpret_cast<const double*>(dp + r->omega),
                                     reinterpret_cast<const int32_t*>(stage_ptr + o_idx), n_idx, d,
                                     reinterpret_cast<double*>(stage_ptr + o_out), iws, iwsb, s, opt))
        return rc;
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(FFK_EHIP, "infidelity failed: %s", hipGetErrorString(e));
    std::memcpy(infid, stage_ptr + o_out, 8*sh.n_out);
    return FFK_OK;
}

// ---- many sequences from one gate table in ONE pass (ff.concatenate_sequences; sequences.hip) ----------------
namespace {

// (every layout of these passes: the gate table first -- ffk_api_gate_table.h --, then what the pass adds)
struct SeqLayout {
    GateTableLayout table;
    size_t S, idx, inputs_end;                                                          // one H2D
    size_t Q, F, infid, outputs_end;                                                    // one D2H
    size_t R, phases, L, end;                                                           // device only
};

SeqLayout seq_layout(int T, int P, size_t n_index, int n_host, int d, int A, int N, int W, SpectrumShape sh, int n_idx) {
    SeqLayout L;
    const size_t dd = size_t(d)*d, row = 16*size_t(A)*N*W;
    size_t o = 0;
    auto put = [&o](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
    L.table = gate_table_layout(put, T, P, n_index, n_host, d, A, N, W);
    L.S = put(16*sh.rows*W);
    L.idx = put(4*size_t(n_idx));
    L.inputs_end = o;
    L.Q = put(16*size_t(P)*dd);
    L.F = put(16*size_t(P)*A*A*W);
    L.infid = put(8*size_t(P)*sh.n_out);
    L.outputs_end = o;
    L.R = put(row*size_t(P));
    L.phases = put(16*size_t(T)*W);
    L.L = put(8*size_t(T)*N*N);
    L.end = o;
    return L;
}

}  // namespace

size_t ffk_concatenate_sequences_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A, int N, int W,
                                                 int n_idx, int s_ndim) {
    if (T < 1 || P < 1 || n_index < P || n_host < 0 || n_host > T || !ffk::sequences_supported(d, N, A) || W < 1)
        return 0;
    if (s_ndim != 0 && (s_ndim < 1 || s_ndim > 3 || n_idx < 1 || n_idx > A)) return 0;
    return seq_layout(T, P, size_t(n_index), n_host, d, A, N, W,
                      s_ndim ? spectrum_shape(s_ndim, n_idx) : SpectrumShape{}, s_ndim ? n_idx : 0).end;
}

int ffk_concatenate_sequences_resident(ffk_resident* result, ffk_resident* const* gates, const int32_t* slots,
                                       const double* gate_table, const double* gate_propagators, const double* tau,
                                       int T, const int32_t* offsets, const int32_t* index, int P,
                                       const double* omega, int W, const double* basis, int hermitian_basis, int d,
                                       int A, int N, const double* spectrum, int s_ndim, int spectrum_is_real,
                                       const int32_t* idx, int n_idx, int d_infidelity, double* total_propagators,
                                       double** filter_function, double* infid) {
    const GateTable g{gates, slots, gate_table, gate_propagators, tau, T, offsets, index, P, omega, W, basis,
                      hermitian_basis, d, A, N};
    FFK_REQUIRE(result, "NULL argument");
    FFK_REQUIRE(total_propagators && filter_function, "NULL output argument");
    FFK_REQUIRE(ffk::sequences_supported(d, N, A), "unsupported shape d=%d N=%d A=%d (need d = 2, N = 4, 1 <= A <= 4)",
                d, N, A);
    size_t n_index = 0;
    if (int rc = check_gate_table(g, 1, &n_index)) return rc;
    if (spectrum) {
        if (int rc = check_spectrum_args(s_ndim, idx, n_idx, A, d_infidelity, infid && W >= 2)) return rc;
    } else {
        n_idx = 0;
    }
    const SpectrumShape sh = spectrum ? spectrum_shape(s_ndim, n_idx) : SpectrumShape{};
    int dev = 0;
    FFK_HIP(hipGetDevice(&dev));
    for (int k = 0; k < T; ++k)
        FFK_REQUIRE(gates[k] != result, "gate %d: the result handle must not be an input", k);
    // where each gate's control matrix lies on the device: in its own handle, or in the uploaded host table
    std::vector<const unsigned char*> tab;
    int n_host = 0;
    if (int rc = locate_gates(g, dev, &tab, &n_host)) return rc;
    const SeqLayout L = seq_layout(T, P, n_index, n_host, d, A, N, W, sh, n_idx);
    if (int rc = ensure_blocks(result, dev, L.end, L.outputs_end)) return rc;
    unsigned char* hp = static_cast<unsigned char*>(result->pin.ptr);
    unsigned char* dp = static_cast<unsigned char*>(result->dev.ptr);
    const size_t dd = size_t(d)*d;
    PassClock clock;
    stage_gate_table(g, L.table, n_index, longest_first(offsets, P).data(), &tab, hp, dp);
    if (spectrum) stage_spectrum(spectrum, spectrum_is_real != 0, sh.rows*W, idx, n_idx, hp + L.S, hp + L.idx);
    hipStream_t s;
    if (int rc = resident_stream(&s)) return rc;
    StreamDrain drain{s};
    clock.lap();
    auto at = [dp](size_t off) { return dp + off; };
    FFK_HIP(hipMemcpyAsync(dp, hp, L.inputs_end, hipMemcpyHostToDevice, s));
    const GateTableDevice D(dp, L.table);
    cplx* dPh = reinterpret_cast<cplx*>(at(L.phases));
    double* dL = reinterpret_cast<double*>(at(L.L));
    cplx* dF = reinterpret_cast<cplx*>(at(L.F));
    FFK_HIP(launch_gate_table_front(g, D, dPh, dL, reinterpret_cast<cplx*>(at(L.Q)), s));
    FFK_HIP(ffk::launch_sequences_rule(dPh, D.tab, dL, D.offsets, D.index, D.order, P, T, A, W,
                                       reinterpret_cast<cplx*>(at(L.R)), dF, s));
    if (spectrum)
        FFK_HIP(ffk::launch_infidelity_pulses(dF, A, W, P, reinterpret_cast<const cplx*>(at(L.S)), s_ndim, D.omega,
                                              reinterpret_cast<const int32_t*>(at(L.idx)), n_idx, d_infidelity,
                                              reinterpret_cast<double*>(at(L.infid)), s));
    FFK_HIP(hipMemcpyAsync(hp + L.Q, dp + L.Q, L.outputs_end - L.Q, hipMemcpyDeviceToHost, s));
    clock.lap();
    FFK_HIP(hipStreamSynchronize(s));
    clock.lap();
    clock.store(result);
    if (int rc = kernel_fault_status()) return rc;
    std::memcpy(total_propagators, hp + L.Q, 16*size_t(P)*dd);
    *filter_function = reinterpret_cast<double*>(hp + L.F);
    if (spectrum) std::memcpy(infid, hp + L.infid, 8*size_t(P)*sh.n_out);
    result->hold(ffk_resident::MEMBERS, P, d, W, N, A, L.R, L.F, L.table.omega);
    return FFK_OK;
}

// The infidelity integral of a subset of a batched pass's members on their resident filter functions: ONE launch of
// the pulse-axis integral (infid_pulses_kernel).  Runs of consecutive members are read in place; otherwise their
// filter functions are first gathered by device-to-device copies.
int ffk_resident_batch_infidelity(ffk_resident* r, const int32_t* members, int n_members, const double* spectrum,
                                  int s_ndim, int spectrum_is_real, const int32_t* idx, int n_idx, int d,
                                  double* infid) {
    FFK_REQUIRE(r && r->kind == ffk_resident::MEMBERS, "no resident batch result");
    FFK_REQUIRE(members && spectrum && idx && infid, "NULL argument");
    FFK_REQUIRE(n_members >= 1 && n_members <= 65535, "need 1 <= n_members <= 65535, got %d", n_members);
    if (int rc = check_spectrum_args(s_ndim, idx, n_idx, r->A, d, r->W >= 2)) return rc;
    for (int m = 0; m < n_members; ++m)
        FFK_REQUIRE(members[m] >= 0 && members[m] < r->P, "members[%d] = %d outside [0, %d)", m, members[m], r->P);
    if (int rc = on_owning_device(r)) return rc;
    const int W = r->W, A = r->A;
    const SpectrumShape sh = spectrum_shape(s_ndim, n_idx);
    const size_t fbytes = 16*size_t(A)*A*W, out_bytes = 8*size_t(n_members)*sh.n_out;
    bool consecutive = true;
    for (int m = 1; m < n_members; ++m) consecutive = consecutive && members[m] == members[m - 1] + 1;
    const size_t o_idx = align_up(16*sh.rows*W), o_out = o_idx + align_up(4*size_t(n_idx));
    const size_t stage = o_out + align_up(out_bytes);
    PinLease pin;
    if (int rc = pin.take(stage, r->device)) return rc;
    unsigned char* hp = pin.ptr();
    stage_spectrum(spectrum, spectrum_is_real != 0, sh.rows*W, idx, n_idx, hp, hp + o_idx);
    hipStream_t s;
    if (int rc = resident_stream(&s)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    void* base = nullptr;
    if (int rc = arena_reserve(stage + (consecutive ? 0 : align_up(fbytes*n_members)), &base)) return rc;
    StreamDrain drain{s};
    unsigned char* ws = static_cast<unsigned char*>(base);
    const unsigned char* dF = static_cast<const unsigned char*>(r->dev.ptr) + r->F;
    FFK_HIP(hipMemcpyAsync(ws, hp, o_out, hipMemcpyHostToDevice, s));
    const unsigned char* F = dF + fbytes*size_t(members[0]);
    if (!consecutive) {
        unsigned char* gathered = ws + stage;
        for (int m = 0; m < n_members;) {
            int e = m + 1;
            while (e < n_members && members[e] == members[e - 1] + 1) ++e;
            FFK_HIP(hipMemcpyAsync(gathered + fbytes*size_t(m), dF + fbytes*size_t(members[m]), fbytes*size_t(e - m),
                                   hipMemcpyDeviceToDevice, s));
            m = e;
        }
        F = gathered;
    }
    FFK_HIP(ffk::launch_infidelity_pulses(reinterpret_cast<const cplx*>(F), A, W, n_members,
                                          reinterpret_cast<const cplx*>(ws), s_ndim,
                                          reinterpret_cast<const double*>(static_cast<const unsigned char*>(r->dev.ptr) +
                                                                          r->omega),
                                          reinterpret_cast<const int32_t*>(ws + o_idx), n_idx, d,
                                          reinterpret_cast<double*>(ws + o_out), s));
    FFK_HIP(hipMemcpyAsync(hp + o_out, ws + o_out, out_bytes, hipMemcpyDeviceToHost, s));
    FFK_HIP(hipStreamSynchronize(s));
    if (int rc = kernel_fault_status()) return rc;
    std::memcpy(infid, hp + o_out, out_bytes);
    return FFK_OK;
}

// ---- pulse-correlation infidelities of many sequences from one gate table in ONE pass
//      (ff.correlation_infidelities; correlations.hip) ------------------------------------------------------------
namespace {

// (the table's `order` holds the sequences sorted by length class)
struct CorrLayout {
    GateTableLayout table;
    size_t out_offsets, S, idx, inputs_end;                                                             // one H2D
    size_t infid, outputs_end;                                                                          // one D2H
    size_t Q, phases, L, Qc, scale, part, end;                                                          // device only
};

// total: the sum of G_p^2 (the rows of the ragged output)
CorrLayout corr_layout(int T, int P, size_t n_index, int n_host, int d, int A, int N, int W, SpectrumShape sh,
                       int n_idx, size_t total) {
    CorrLayout L;
    const size_t dd = size_t(d)*d;
    size_t o = 0;
    auto put = [&o](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
    L.table = gate_table_layout(put, T, P, n_index, n_host, d, A, N, W);
    L.out_offsets = put(8*(size_t(P) + 1));
    L.S = put(16*sh.rows*W);
    L.idx = put(4*size_t(n_idx));
    L.inputs_end = o;
    L.infid = put(8*total*n_idx);
    L.outputs_end = o;
    L.Q = put(16*size_t(P)*dd);
    L.phases = put(16*size_t(T)*W);
    L.L = put(8*size_t(T)*N*N);
    L.Qc = put(8*n_index*N*N);
    L.scale = put(16*sh.rows*W);
    L.part = put(8*size_t(ffk::correlation_slabs(W, nullptr))*n_idx*total);
    L.end = o;
    return L;
}

bool corr_shape_ok(bool two_qubit, int T, int P, int d, int A, int N, int W, int n_idx, int s_ndim) {
    return T >= 1 && T <= (1 << 20) && P >= 1 && P <= (1 << 24) &&
           (two_qubit ? ffk::sequences4_supported(d, N, A) : ffk::sequences_supported(d, N, A)) && W >= 1 &&
           (s_ndim == 1 || s_ndim == 2) && n_idx >= 1 && n_idx <= A;
}

size_t corr_workspace_bytes(bool two_qubit, int T, int P, int n_index, int n_host, int d, int A, int N, int W,
                            int n_idx, int s_ndim) {
    if (!corr_shape_ok(two_qubit, T, P, d, A, N, W, n_idx, s_ndim) || n_index < P || n_host < 0 || n_host > T) return 0;
    // the lengths are not known here: no sequence is longer than the cap or than all positions together
    const size_t longest = std::min(size_t(ffk::correlation_max_length()), size_t(n_index));
    return corr_layout(T, P, size_t(n_index), n_host, d, A, N, W, spectrum_shape(s_ndim, n_idx), n_idx,
                       size_t(n_index)*longest).end;
}

// The pass of both entries: single-qubit gates on the kernels of correlations.hip, two-qubit gates (two_qubit) on
// those of correlations_d4.hip behind the front launch of their dimension.
int correlation_pass(bool two_qubit, ffk_resident* const* gates, const int32_t* slots, const double* gate_table,
                     const double* gate_propagators, const double* tau, int T, const int32_t* offsets,
                     const int32_t* index, int P, const double* omega, int W, const double* basis,
                     int hermitian_basis, int d, int A, int N, const double* spectrum, int s_ndim,
                     int spectrum_is_real, const int32_t* idx, int n_idx, int d_infidelity,
                     const int64_t* out_offsets, double* infidelity) {
    const GateTable g{gates, slots, gate_table, gate_propagators, tau, T, offsets, index, P, omega, W, basis,
                      hermitian_basis, d, A, N};
    FFK_REQUIRE(spectrum && idx && out_offsets && infidelity, "NULL argument");
    if (two_qubit)
        FFK_REQUIRE(ffk::sequences4_supported(d, N, A),
                    "unsupported shape d=%d N=%d A=%d (need d = 4, N = 16, 1 <= A <= 4)", d, N, A);
    else
        FFK_REQUIRE(ffk::sequences_supported(d, N, A), "unsupported shape d=%d N=%d A=%d (need d = 2, N = 4, 1 <= A <= 4)",
                    d, N, A);
    FFK_REQUIRE(hermitian_basis != 0, "the batched pass needs a Hermitian basis");
    FFK_REQUIRE(s_ndim == 1 || s_ndim == 2, "spectrum of %d dimensions: cross-spectra are not integrated here", s_ndim);
    size_t n_index = 0;
    if (int rc = check_gate_table(g, 1, &n_index)) return rc;
    if (int rc = check_spectrum_args(s_ndim, idx, n_idx, A, d_infidelity, W >= 2)) return rc;
    const int max_length = ffk::correlation_max_length();
    FFK_REQUIRE(out_offsets[0] == 0, "offsets[0] = %d, out_offsets[0] = %lld, expected 0", offsets[0],
                static_cast<long long>(out_offsets[0]));
    for (int p = 0; p < P; ++p) {
        const int64_t G = int64_t(offsets[p + 1]) - offsets[p];
        FFK_REQUIRE(G <= max_length, "sequence %d has %lld positions, need 1 ... %d", p, static_cast<long long>(G),
                    max_length);
        FFK_REQUIRE(out_offsets[p + 1] - out_offsets[p] == G*G, "out_offsets is not the prefix sum of G^2 at sequence %d",
                    p);
    }
    const size_t total = size_t(out_offsets[P]);
    if (s_ndim <= 2 && !spectrum_is_real)
        for (size_t i = 0; i < spectrum_shape(s_ndim, n_idx).rows*W; ++i)
            FFK_REQUIRE(spectrum[2*i + 1] == 0.0, "the spectrum has an imaginary part at element %zu", i);
    const SpectrumShape sh = spectrum_shape(s_ndim, n_idx);
    int dev = 0;
    FFK_HIP(hipGetDevice(&dev));
    std::vector<const unsigned char*> tab;
    int n_host = 0;
    if (int rc = locate_gates(g, dev, &tab, &n_host)) return rc;
    const CorrLayout L = corr_layout(T, P, n_index, n_host, d, A, N, W, sh, n_idx, total);
    // the sequences sorted by the length class whose kernel serves them (stable), and how many of each
    std::vector<int32_t> members(P);
    int class_counts[4] = {0, 0, 0, 0};
    for (int p = 0; p < P; ++p) {
        members[p] = p;
        ++class_counts[ffk::correlation_class(offsets[p + 1] - offsets[p])];
    }
    std::stable_sort(members.begin(), members.end(), [offsets](int32_t a, int32_t b) {
        return ffk::correlation_class(offsets[a + 1] - offsets[a]) < ffk::correlation_class(offsets[b + 1] - offsets[b]);
    });
    PinLease pin;
    if (int rc = pin.take(L.outputs_end, dev)) return rc;
    unsigned char* hp = pin.ptr();
    hipStream_t s;
    if (int rc = resident_stream(&s)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    void* base = nullptr;
    if (int rc = arena_reserve(L.end, &base)) return rc;
    unsigned char* dp = static_cast<unsigned char*>(base);
    stage_gate_table(g, L.table, n_index, members.data(), &tab, hp, dp);
    std::memcpy(hp + L.out_offsets, out_offsets, 8*(size_t(P) + 1));
    stage_spectrum(spectrum, spectrum_is_real != 0, sh.rows*W, idx, n_idx, hp + L.S, hp + L.idx);
    StreamDrain drain{s};
    auto at = [dp](size_t off) { return dp + off; };
    FFK_HIP(hipMemcpyAsync(dp, hp, L.inputs_end, hipMemcpyHostToDevice, s));
    const GateTableDevice D(dp, L.table);
    const int64_t* dOut = reinterpret_cast<const int64_t*>(at(L.out_offsets));
    cplx* dPh = reinterpret_cast<cplx*>(at(L.phases));
    double* dL = reinterpret_cast<double*>(at(L.L));
    double* dQc = reinterpret_cast<double*>(at(L.Qc));
    cplx* dScale = reinterpret_cast<cplx*>(at(L.scale));
    double* dPart = reinterpret_cast<double*>(at(L.part));
    const int32_t* dSel = reinterpret_cast<const int32_t*>(at(L.idx));
    FFK_HIP(launch_gate_table_front(g, D, dPh, dL, reinterpret_cast<cplx*>(at(L.Q)), s));
    if (two_qubit)
        FFK_HIP(ffk::launch_correlations4_prefix(dL, D.offsets, D.index, P, dQc, s));
    else
        FFK_HIP(ffk::launch_correlation_prefix(dL, D.offsets, D.index, P, dQc, s));
    FFK_HIP(ffk::launch_spectral_weights(reinterpret_cast<const cplx*>(at(L.S)), int(sh.rows), W, D.omega, W, 0, dScale,
                                         s));
    if (two_qubit)
        FFK_HIP(ffk::launch_correlations4_gram(dPh, D.tab, dQc, D.offsets, D.index, dOut, D.order, class_counts, W,
                                               dScale, s_ndim, dSel, n_idx, d_infidelity, int64_t(total), dPart, s));
    else
        FFK_HIP(ffk::launch_correlation_gram(dPh, D.tab, dQc, D.offsets, D.index, dOut, D.order, class_counts, W,
                                             dScale, s_ndim, dSel, n_idx, d_infidelity, int64_t(total), dPart, s));
    FFK_HIP(ffk::launch_correlation_reduce(dPart, dOut, D.offsets, P, n_idx, W, int64_t(total),
                                           reinterpret_cast<double*>(at(L.infid)), s));
    FFK_HIP(hipMemcpyAsync(hp + L.infid, dp + L.infid, 8*total*n_idx, hipMemcpyDeviceToHost, s));
    FFK_HIP(hipStreamSynchronize(s));
    if (int rc = kernel_fault_status()) return rc;
    std::memcpy(infidelity, hp + L.infid, 8*total*n_idx);
    return FFK_OK;
}

}  // namespace

size_t ffk_sequence_correlation_infidelities_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A,
                                                             int N, int W, int n_idx, int s_ndim) {
    return corr_workspace_bytes(false, T, P, n_index, n_host, d, A, N, W, n_idx, s_ndim);
}

int ffk_sequence_correlation_infidelities(ffk_resident* const* gates, const int32_t* slots, const double* gate_table,
                                          const double* gate_propagators, const double* tau, int T,
                                          const int32_t* offsets, const int32_t* index, int P, const double* omega,
                                          int W, const double* basis, int hermitian_basis, int d, int A, int N,
                                          const double* spectrum, int s_ndim, int spectrum_is_real, const int32_t* idx,
                                          int n_idx, int d_infidelity, const int64_t* out_offsets, double* infidelity) {
    return correlation_pass(false, gates, slots, gate_table, gate_propagators, tau, T, offsets, index, P, omega, W, basis,
                            hermitian_basis, d, A, N, spectrum, s_ndim, spectrum_is_real, idx, n_idx, d_infidelity,
                            out_offsets, infidelity);
}

// ---- the same for two-qubit gates, (d, N) = (4, 16) (ff.sequence_correlation_infidelities; correlations_d4.hip) ----
size_t ffk_sequence_correlation_infidelities4_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A,
                                                              int N, int W, int n_idx, int s_ndim) {
    return corr_workspace_bytes(true, T, P, n_index, n_host, d, A, N, W, n_idx, s_ndim);
}

int ffk_sequence_correlation_infidelities4(ffk_resident* const* gates, const int32_t* slots, const double* gate_table,
                                           const double* gate_propagators, const double* tau, int T,
                                           const int32_t* offsets, const int32_t* index, int P, const double* omega,
                                           int W, const double* basis, int hermitian_basis, int d, int A, int N,
                                           const double* spectrum, int s_ndim, int spectrum_is_real, const int32_t* idx,
                                           int n_idx, int d_infidelity, const int64_t* out_offsets,
                                           double* infidelity) {
    return correlation_pass(true, gates, slots, gate_table, gate_propagators, tau, T, offsets, index, P, omega, W, basis,
                            hermitian_basis, d, A, N, spectrum, s_ndim, spectrum_is_real, idx, n_idx, d_infidelity,
                            out_offsets, infidelity);
}

// ---- infidelities of many sequences from one gate table in ONE pass, single- or two-qubit gates
//      (ff.sequence_infidelities; sequences.hip, sequences_d4.hip) ------------------------------------------------
namespace {

struct SeqInfidLayout {
    GateTableLayout table;
    size_t S, idx, inputs_end;                                                            // one H2D
    size_t infid, Q, small_outputs_end, F, outputs_end;                                   // one D2H (F if asked for)
    size_t phases, L, end;                                                                // device only
};

SeqInfidLayout seq_infid_layout(int T, int P, size_t n_index, int n_host, int d, int A, int N, int W, SpectrumShape sh,
                                int n_idx) {
    SeqInfidLayout L;
    const size_t dd = size_t(d)*d;
    size_t o = 0;
    auto put = [&o](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
    L.table = gate_table_layout(put, T, P, n_index, n_host, d, A, N, W);
    L.S = put(16*sh.rows*W);
    L.idx = put(4*size_t(n_idx));
    L.inputs_end = o;
    L.infid = put(8*size_t(P)*sh.n_out);
    L.Q = put(16*size_t(P)*dd);
    L.small_outputs_end = o;
    L.F = put(16*size_t(P)*A*A*W);
    L.outputs_end = o;
    L.phases = put(16*size_t(T)*W);
    L.L = put(8*size_t(T)*N*N);
    L.end = o;
    return L;
}

bool seq_infid_shape_ok(int T, int P, int d, int A, int N, int W) {
    return T >= 1 && T <= (1 << 20) && P >= 1 && P <= (1 << 24) && W >= 1 &&
           (ffk::sequences_supported(d, N, A) || ffk::sequences4_supported(d, N, A));
}

}  // namespace

size_t ffk_sequence_infidelities_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A, int N, int W,
                                                 int n_idx, int s_ndim) {
    if (!seq_infid_shape_ok(T, P, d, A, N, W) || n_index < P || n_host < 0 || n_host > T) return 0;
    if (s_ndim != 0 && (s_ndim < 1 || s_ndim > 3 || n_idx < 1 || n_idx > A)) return 0;
    return seq_infid_layout(T, P, size_t(n_index), n_host, d, A, N, W,
                            s_ndim ? spectrum_shape(s_ndim, n_idx) : SpectrumShape{}, s_ndim ? n_idx : 0).end;
}

int ffk_sequence_infidelities(ffk_resident* const* gates, const int32_t* slots, const double* gate_table,
                              const double* gate_propagators, const double* tau, int T, const int32_t* offsets,
                              const int32_t* index, int P, const double* omega, int W, const double* basis,
                              int hermitian_basis, int d, int A, int N, const double* spectrum, int s_ndim,
                              int spectrum_is_real, const int32_t* idx, int n_idx, int d_infidelity,
                              double* infidelity, double* total_propagators, double* filter_function) {
    const GateTable g{gates, slots, gate_table, gate_propagators, tau, T, offsets, index, P, omega, W, basis,
                      hermitian_basis, d, A, N};
    FFK_REQUIRE(spectrum ? infidelity != nullptr : (total_propagators || filter_function),
                "NULL output argument: a spectrum needs infidelity, no spectrum another output");
    FFK_REQUIRE(ffk::sequences_supported(d, N, A) || ffk::sequences4_supported(d, N, A),
                "unsupported shape d=%d N=%d A=%d (need (d, N) = (2, 4) or (4, 16), 1 <= A <= 4)", d, N, A);
    size_t n_index = 0;
    if (int rc = check_gate_table(g, 1, &n_index)) return rc;
    if (spectrum) {
        if (int rc = check_spectrum_args(s_ndim, idx, n_idx, A, d_infidelity, W >= 2)) return rc;
        FFK_REQUIRE(P <= 65535, "the integral takes at most 65535 sequences per pass, got %d", P);
    } else {
        n_idx = 0;
    }
    const SpectrumShape sh = spectrum ? spectrum_shape(s_ndim, n_idx) : SpectrumShape{};
    int dev = 0;
    FFK_HIP(hipGetDevice(&dev));
    std::vector<const unsigned char*> tab;
    int n_host = 0;
    if (int rc = locate_gates(g, dev, &tab, &n_host)) return rc;
    const SeqInfidLayout L = seq_infid_layout(T, P, n_index, n_host, d, A, N, W, sh, n_idx);
    const size_t dd = size_t(d)*d;
    const size_t copied_end = filter_function ? L.outputs_end : L.small_outputs_end;
    PinLease pin;
    if (int rc = pin.take(copied_end, dev)) return rc;
    unsigned char* hp = pin.ptr();
    hipStream_t s;
    if (int rc = resident_stream(&s)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    void* base = nullptr;
    if (int rc = arena_reserve(L.end, &base)) return rc;
    unsigned char* dp = static_cast<unsigned char*>(base);
    stage_gate_table(g, L.table, n_index, longest_first(offsets, P).data(), &tab, hp, dp);
    if (spectrum) stage_spectrum(spectrum, spectrum_is_real != 0, sh.rows*W, idx, n_idx, hp + L.S, hp + L.idx);
    StreamDrain drain{s};
    auto at = [dp](size_t off) { return dp + off; };
    FFK_HIP(hipMemcpyAsync(dp, hp, L.inputs_end, hipMemcpyHostToDevice, s));
    const GateTableDevice D(dp, L.table);
    cplx* dPh = reinterpret_cast<cplx*>(at(L.phases));
    double* dL = reinterpret_cast<double*>(at(L.L));
    cplx* dF = reinterpret_cast<cplx*>(at(L.F));
    FFK_HIP(launch_gate_table_front(g, D, dPh, dL, reinterpret_cast<cplx*>(at(L.Q)), s));
    if (d == 2)
        FFK_HIP(ffk::launch_sequences_rule(dPh, D.tab, dL, D.offsets, D.index, D.order, P, T, A, W, nullptr, dF, s));
    else
        FFK_HIP(ffk::launch_sequences4_rule(dPh, D.tab, dL, D.offsets, D.index, D.order, P, T, A, W, dF, s));
    if (spectrum)
        FFK_HIP(ffk::launch_infidelity_pulses(dF, A, W, P, reinterpret_cast<const cplx*>(at(L.S)), s_ndim, D.omega,
                                              reinterpret_cast<const int32_t*>(at(L.idx)), n_idx, d_infidelity,
                                              reinterpret_cast<double*>(at(L.infid)), s));
    FFK_HIP(hipMemcpyAsync(hp + L.infid, dp + L.infid, copied_end - L.infid, hipMemcpyDeviceToHost, s));
    FFK_HIP(hipStreamSynchronize(s));
    if (int rc = kernel_fault_status()) return rc;
    if (spectrum) std::memcpy(infidelity, hp + L.infid, 8*size_t(P)*sh.n_out);
    if (total_propagators) std::memcpy(total_propagators, hp + L.Q, 16*size_t(P)*dd);
    if (filter_function) std::memcpy(filter_function, hp + L.F, 16*size_t(P)*A*A*W);
    return FFK_OK;
}

// ---- decay amplitudes, cumulant functions and error transfer matrices of many pulses in ONE pass, their control
//      matrices read where they lie in HBM (ff.decay_amplitudes, ff.cumulant_functions, ff.error_transfer_matrices;
//      processes.hip) ----------------------------------------------------------------------------------------------
namespace {

struct ProcLayout {
    size_t tab, omega, basis, S, idx, host, inputs_end;           // one H2D
    size_t outputs, gamma, K, U, flags, outputs_end;              // one D2H of [outputs, outputs_end)
    size_t scale, partials, cumulant, end;                        // device only
};

// The requested results lie next to each other in front of the flags; what is only an intermediate of this call lies
// behind them with the workspace.  stage: 1 decay amplitudes, 2 + cumulant function, 3 + error transfer matrix.
ProcLayout proc_layout(int P, int n_host, int A, int N, int W, int d, int n_idx, int s_ndim, bool single_qubit,
                       bool want_gamma, bool want_K, bool want_U) {
    ProcLayout L;
    const size_t dd = size_t(d)*d, nn = size_t(N)*N;
    const SpectrumShape sh = spectrum_shape(s_ndim, n_idx);
    const size_t pairs = sh.n_out, s_rows = sh.rows;
    const int stage = want_U ? 3 : (want_K ? 2 : 1);
    size_t o = 0;
    auto put = [&o](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
    L.tab = put(8*size_t(P));
    L.omega = put(8*size_t(W));
    L.basis = put(16*size_t(N)*dd);
    L.S = put(16*s_rows*W);
    L.idx = put(4*size_t(n_idx));
    L.host = put(16*size_t(A)*N*W*size_t(n_host));
    L.inputs_end = o;
    L.outputs = o;
    L.gamma = L.K = L.U = 0;
    if (want_gamma) L.gamma = put(8*size_t(P)*pairs*nn);
    if (want_K) L.K = put(8*size_t(P)*pairs*nn);
    if (want_U) L.U = put(8*size_t(P)*nn);
    L.flags = put(4*size_t(P));
    L.outputs_end = o;
    if (!want_gamma) L.gamma = put(8*size_t(P)*pairs*nn);
    if (!want_K && stage >= 2) L.K = put(8*size_t(P)*pairs*nn);
    L.scale = put(16*s_rows*W);
    const int chunks = ffk::processes_decay_chunks(W, nullptr);
    L.partials = put(chunks > 1 ? 8*size_t(chunks)*P*pairs*nn : 0);
    L.cumulant = put(stage >= 2 && !single_qubit ? ffk::cumulant_workspace_bytes(size_t(P)*pairs, N, d) : 0);
    L.end = o;
    return L;
}

bool proc_shape_ok(int P, int n_host, int A, int N, int W, int d, int n_idx, int s_ndim) {
    return P >= 1 && P <= 65535 && n_host >= 0 && n_host <= P && A >= 1 && N >= 1 && N <= 16 && W >= 1 &&
           d_templated_ok(d) && N <= d*d && s_ndim >= 1 && s_ndim <= 3 && n_idx >= 1 && n_idx <= A;
}

}  // namespace

size_t ffk_resident_batch_processes_workspace_bytes(int P, int n_host, int A, int N, int W, int d, int n_idx,
                                                    int s_ndim) {
    if (!proc_shape_ok(P, n_host, A, N, W, d, n_idx, s_ndim)) return 0;
    return proc_layout(P, n_host, A, N, W, d, n_idx, s_ndim, false, true, true, true).end;
}

int ffk_resident_batch_processes(ffk_resident* const* pulses, const int32_t* slots, const double* control_matrices,
                                 int P, int A, int N, int W, int d, const double* omega, const double* basis,
                                 int single_qubit, const double* spectrum, int s_ndim, const int32_t* idx, int n_idx,
                                 double* decay_amplitudes, double* cumulant_function, double* error_transfer_matrix,
                                 int32_t* not_finite) {
    FFK_REQUIRE(pulses && slots && omega && basis && spectrum && idx, "NULL argument");
    FFK_REQUIRE(decay_amplitudes || cumulant_function || error_transfer_matrix, "no output requested");
    FFK_REQUIRE(!error_transfer_matrix || not_finite, "not_finite is NULL but the error transfer matrices are requested");
    FFK_REQUIRE(proc_shape_ok(P, 0, A, N, W, d, n_idx, s_ndim),
                "unsupported shape P=%d A=%d N=%d W=%d d=%d n_idx=%d s_ndim=%d (need 1 <= P <= 65535, N <= 16, "
                "N <= d^2, 1 <= n_idx <= A, 1 <= s_ndim <= 3)", P, A, N, W, d, n_idx, s_ndim);
    FFK_REQUIRE(!single_qubit || (d == 2 && N == 4), "single-qubit expression needs d = 2, N = 4");
    if (int rc = check_spectrum_args(s_ndim, idx, n_idx, A, d, true)) return rc;
    const SpectrumShape sh = spectrum_shape(s_ndim, n_idx);
    const size_t pairs = sh.n_out, s_rows = sh.rows;
    const bool want_gamma = decay_amplitudes != nullptr, want_K = cumulant_function != nullptr;
    const bool want_U = error_transfer_matrix != nullptr;
    const int stage = want_U ? 3 : (want_K ? 2 : 1);
    FFK_REQUIRE(stage < 2 || single_qubit || size_t(P)*pairs <= 65535,
                "%d pulses of %zu operator pairs exceed the 65535 cumulant functions of one launch", P, pairs);
    int dev = 0;
    FFK_HIP(hipGetDevice(&dev));
    // where each pulse's control matrix lies on the device: in its handle (of any dimension: only the shape of the
    // control matrix matters here), or in the uploaded host table
    std::vector<const unsigned char*> tab;
    int n_host = 0;
    if (int rc = locate_control_matrices(pulses, slots, P, dev, 0, A, N, W, "pulse", &tab, &n_host)) return rc;
    FFK_REQUIRE(n_host == 0 || control_matrices, "control_matrices is NULL but %d pulse(s) have no handle", n_host);
    const ProcLayout L = proc_layout(P, n_host, A, N, W, d, n_idx, s_ndim, single_qubit != 0, want_gamma, want_K,
                                     want_U);
    const size_t dd = size_t(d)*d, nn = size_t(N)*N;
    const size_t row = 16*size_t(A)*N*W, out_bytes = L.outputs_end - L.outputs;
    // a spectrum of one or two dimensions with an imaginary part: Gamma is not symmetric, every weight is complex
    int complex_weights = 0;
    if (s_ndim != 3)
        for (size_t i = 0; i < s_rows*W && !complex_weights; ++i) complex_weights = spectrum[2*i + 1] != 0.0;
    PinLease pin;
    if (int rc = pin.take(L.outputs_end, dev)) return rc;
    unsigned char* hp = pin.ptr();
    hipStream_t s;
    if (int rc = resident_stream(&s)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    void* base = nullptr;
    if (int rc = arena_reserve(L.end, &base)) return rc;
    unsigned char* dp = static_cast<unsigned char*>(base);
    place_host_rows(&tab, dp + L.host, row);
    std::memcpy(hp + L.tab, tab.data(), 8*size_t(P));
    std::memcpy(hp + L.omega, omega, 8*size_t(W));
    std::memcpy(hp + L.basis, basis, 16*size_t(N)*dd);
    stage_spectrum(spectrum, false, s_rows*W, idx, n_idx, hp + L.S, hp + L.idx);
    if (n_host) std::memcpy(hp + L.host, control_matrices, row*size_t(n_host));
    StreamDrain drain{s};
    FFK_HIP(hipMemcpyAsync(dp, hp, L.inputs_end, hipMemcpyHostToDevice, s));
    const cplx* dS = reinterpret_cast<const cplx*>(dp + L.S);
    const double* dOmega = reinterpret_cast<const double*>(dp + L.omega);
    const int32_t* dIdx = reinterpret_cast<const int32_t*>(dp + L.idx);
    cplx* dScale = reinterpret_cast<cplx*>(dp + L.scale);
    double* dGamma = reinterpret_cast<double*>(dp + L.gamma);
    double* dK = reinterpret_cast<double*>(dp + L.K);
    int32_t* dFlags = reinterpret_cast<int32_t*>(dp + L.flags);
    FFK_HIP(hipMemsetAsync(dFlags, 0, 4*size_t(P), s));
    FFK_HIP(ffk::launch_spectral_weights(dS, int(s_rows), W, dOmega, W, 0, dScale, s));
    FFK_HIP(ffk::launch_processes_decay(reinterpret_cast<const cplx* const*>(dp + L.tab), P, N, W, dScale, s_ndim,
                                        complex_weights, dIdx, n_idx, dGamma,
                                        reinterpret_cast<double*>(dp + L.partials), s));
    if (stage >= 2)
        FFK_HIP(ffk::launch_cumulant_function(dGamma, size_t(P)*pairs, N, d,
                                              reinterpret_cast<const cplx*>(dp + L.basis), single_qubit, dK,
                                              dp + L.cumulant, s));
    if (stage >= 3)
        FFK_HIP(ffk::launch_processes_expm(dK, P, int(pairs), N, reinterpret_cast<double*>(dp + L.U), dFlags, s));
    FFK_HIP(hipMemcpyAsync(hp + L.outputs, dp + L.outputs, out_bytes, hipMemcpyDeviceToHost, s));
    FFK_HIP(hipStreamSynchronize(s));
    if (int rc = kernel_fault_status()) return rc;
    if (want_gamma) std::memcpy(decay_amplitudes, hp + L.gamma, 8*size_t(P)*pairs*nn);
    if (want_K) std::memcpy(cumulant_function, hp + L.K, 8*size_t(P)*pairs*nn);
    if (want_U) std::memcpy(error_transfer_matrix, hp + L.U, 8*size_t(P)*nn);
    if (not_finite) std::memcpy(not_finite, hp + L.flags, 4*size_t(P));
    return FFK_OK;
}

// ---- decay amplitudes, cumulant functions and error transfer matrices of many sequences from one gate table in ONE
//      pass, under any number of spectra (ff.sequence_decay_amplitudes, ...; sequence_processes.hip) ----------------
namespace {

struct SeqProcLayout {
    GateTableLayout table;
    size_t S, idx, inputs_end;                                                            // one H2D
    size_t out, flags, Q, outputs_end;                                                    // one D2H
    size_t phases, L, scale, partial, gamma, K, cumulant, end;                            // device only
};

// stage: 1 decay amplitudes, 2 cumulant function, 3 error transfer matrix (the requested one lies in `out`)
SeqProcLayout seq_proc_layout(int T, int P, size_t n_index, int n_host, int d, int A, int N, int W, int n_idx,
                              int s_ndim, int n_spectra, int stage, bool single_qubit) {
    SeqProcLayout L;
    const size_t dd = size_t(d)*d, nn = size_t(N)*N;
    const size_t rows = size_t(n_spectra)*spectrum_shape(s_ndim, n_idx).rows;
    const size_t tiles = size_t(n_spectra)*P*n_idx;
    const int width = ffk::sequence_processes_block_width(d, A);
    size_t o = 0;
    auto put = [&o](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
    L.table = gate_table_layout(put, T, P, n_index, n_host, d, A, N, W);
    L.S = put(16*rows*W);
    L.idx = put(4*size_t(n_idx));
    L.inputs_end = o;
    L.out = put(stage == 3 ? 8*size_t(n_spectra)*P*nn : 8*tiles*nn);
    L.flags = put(4*size_t(n_spectra)*P);
    L.Q = put(16*size_t(P)*dd);
    L.outputs_end = o;
    L.phases = put(16*size_t(T)*W);
    L.L = put(8*size_t(T)*nn);
    L.scale = put(16*rows*W);
    L.partial = put(8*size_t((W + width - 1)/width)*tiles*nn);
    L.gamma = stage == 1 ? L.out : put(8*tiles*nn);
    L.K = stage == 2 ? L.out : put(stage == 3 ? 8*tiles*nn : 0);
    L.cumulant = put(stage >= 2 && !single_qubit ? ffk::cumulant_workspace_bytes(tiles, N, d) : 0);
    L.end = o;
    return L;
}

bool seq_proc_shape_ok(int T, int P, int d, int A, int N, int W, int n_idx, int s_ndim, int n_spectra, int stage) {
    return seq_infid_shape_ok(T, P, d, A, N, W) && W >= 2 && (s_ndim == 1 || s_ndim == 2) && n_idx >= 1 &&
           n_idx <= A && n_spectra >= 1 && n_spectra <= 65535 && stage >= 1 && stage <= 3;
}

}  // namespace

size_t ffk_sequence_processes_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A, int N, int W,
                                              int n_idx, int s_ndim, int n_spectra, int stage) {
    if (!seq_proc_shape_ok(T, P, d, A, N, W, n_idx, s_ndim, n_spectra, stage) || n_index < P || n_host < 0 ||
        n_host > T)
        return 0;
    return seq_proc_layout(T, P, size_t(n_index), n_host, d, A, N, W, n_idx, s_ndim, n_spectra, stage, false).end;
}

int ffk_sequence_processes(ffk_resident* const* gates, const int32_t* slots, const double* gate_table,
                           const double* gate_propagators, const double* tau, int T, const int32_t* offsets,
                           const int32_t* index, int P, const double* omega, int W, const double* basis,
                           int hermitian_basis, int d, int A, int N, int single_qubit, const double* spectrum,
                           int s_ndim, int n_spectra, const int32_t* idx, int n_idx, int stage, double* out,
                           int32_t* not_finite, double* total_propagators) {
    const GateTable g{gates, slots, gate_table, gate_propagators, tau, T, offsets, index, P, omega, W, basis,
                      hermitian_basis, d, A, N};
    FFK_REQUIRE(spectrum && idx && out && not_finite, "NULL argument");
    FFK_REQUIRE(ffk::sequences_supported(d, N, A) || ffk::sequences4_supported(d, N, A),
                "unsupported shape d=%d N=%d A=%d (need (d, N) = (2, 4) or (4, 16), 1 <= A <= 4)", d, N, A);
    FFK_REQUIRE(!single_qubit || d == 2, "single-qubit expression needs d = 2, N = 4");
    size_t n_index = 0;
    if (int rc = check_gate_table(g, 2, &n_index)) return rc;
    FFK_REQUIRE(s_ndim == 1 || s_ndim == 2, "spectrum of %d dimensions: cross-spectra are not integrated here", s_ndim);
    FFK_REQUIRE(n_spectra >= 1 && n_spectra <= 65535, "n_spectra = %d, need 1 ... 65535", n_spectra);
    FFK_REQUIRE(stage >= 1 && stage <= 3, "stage = %d, need 1 (decay amplitudes), 2 (cumulant function) or 3 (error "
                "transfer matrix)", stage);
    if (int rc = check_spectrum_args(s_ndim, idx, n_idx, A, d, true)) return rc;
    const size_t tiles = size_t(n_spectra)*P*n_idx, members = size_t(n_spectra)*P;
    FFK_REQUIRE(tiles <= (size_t(1) << 26), "%zu decay-amplitude tiles exceed one pass", tiles);
    FFK_REQUIRE(stage < 2 || single_qubit || tiles <= 65535,
                "%d spectra x %d sequences x %d operators exceed the 65535 cumulant functions of one launch",
                n_spectra, P, n_idx);
    const size_t s_rows = size_t(n_spectra)*spectrum_shape(s_ndim, n_idx).rows;
    int dev = 0;
    FFK_HIP(hipGetDevice(&dev));
    std::vector<const unsigned char*> tab;
    int n_host = 0;
    if (int rc = locate_gates(g, dev, &tab, &n_host)) return rc;
    const SeqProcLayout L = seq_proc_layout(T, P, n_index, n_host, d, A, N, W, n_idx, s_ndim, n_spectra, stage,
                                            single_qubit != 0);
    const size_t dd = size_t(d)*d, nn = size_t(N)*N;
    const size_t out_bytes = stage == 3 ? 8*members*nn : 8*tiles*nn;
    PinLease pin;
    if (int rc = pin.take(L.outputs_end, dev)) return rc;
    unsigned char* hp = pin.ptr();
    hipStream_t s;
    if (int rc = resident_stream(&s)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    void* base = nullptr;
    if (int rc = arena_reserve(L.end, &base)) return rc;
    unsigned char* dp = static_cast<unsigned char*>(base);
    stage_gate_table(g, L.table, n_index, longest_first(offsets, P).data(), &tab, hp, dp);
    stage_spectrum(spectrum, true, s_rows*W, idx, n_idx, hp + L.S, hp + L.idx);
    StreamDrain drain{s};
    auto at = [dp](size_t off) { return dp + off; };
    FFK_HIP(hipMemcpyAsync(dp, hp, L.inputs_end, hipMemcpyHostToDevice, s));
    const GateTableDevice D(dp, L.table);
    const int32_t* dIdx = reinterpret_cast<const int32_t*>(at(L.idx));
    cplx* dPh = reinterpret_cast<cplx*>(at(L.phases));
    double* dL = reinterpret_cast<double*>(at(L.L));
    cplx* dScale = reinterpret_cast<cplx*>(at(L.scale));
    double* dGamma = reinterpret_cast<double*>(at(L.gamma));
    double* dK = reinterpret_cast<double*>(at(L.K));
    int32_t* dFlags = reinterpret_cast<int32_t*>(at(L.flags));
    FFK_HIP(hipMemsetAsync(dFlags, 0, 4*members, s));
    FFK_HIP(launch_gate_table_front(g, D, dPh, dL, reinterpret_cast<cplx*>(at(L.Q)), s));
    FFK_HIP(ffk::launch_spectral_weights(reinterpret_cast<const cplx*>(at(L.S)), int(s_rows), W, D.omega, W, 0, dScale,
                                         s));
    FFK_HIP(ffk::launch_sequences_gamma(d, dPh, D.tab, dL, D.offsets, D.index, D.order, P, T, A, W, dScale, s_ndim,
                                        n_spectra, dIdx, n_idx, reinterpret_cast<double*>(at(L.partial)), dGamma, s));
    if (stage >= 2)
        FFK_HIP(ffk::launch_cumulant_function(dGamma, tiles, N, d, D.basis, single_qubit, dK, at(L.cumulant), s));
    if (stage >= 3)
        FFK_HIP(ffk::launch_processes_expm(dK, int(members), n_idx, N, reinterpret_cast<double*>(at(L.out)), dFlags,
                                           s));
    FFK_HIP(hipMemcpyAsync(hp + L.out, dp + L.out, L.outputs_end - L.out, hipMemcpyDeviceToHost, s));
    FFK_HIP(hipStreamSynchronize(s));
    if (int rc = kernel_fault_status()) return rc;
    std::memcpy(out, hp + L.out, out_bytes);
    std::memcpy(not_finite, hp + L.flags, 4*members);
    if (total_propagators) std::memcpy(total_propagators, hp + L.Q, 16*size_t(P)*dd);
    return FFK_OK;
}

// ---- frequency shifts (second order) of many sequences from one gate table in ONE pass, under any number of spectra
//      (ff.sequence_frequency_shifts; sequence_second_order.hip) -----------------------------------------------------
namespace {

struct SeqShiftLayout {
    GateTableLayout table;
    size_t S, idx, shifts, inputs_end;                                                            // one H2D
    size_t out, Q, outputs_end;                                                                   // one D2H
    size_t phases, L, scale, partial, end;                                                        // device only
};

SeqShiftLayout seq_shift_layout(int T, int P, size_t n_index, int n_host, int d, int A, int N, int W, int n_idx,
                                int s_ndim, int n_spectra) {
    SeqShiftLayout L;
    const size_t dd = size_t(d)*d, nn = size_t(N)*N;
    const size_t rows = size_t(n_spectra)*spectrum_shape(s_ndim, n_idx).rows;
    const size_t tiles = size_t(n_spectra)*P*n_idx;
    const int width = ffk::sequence_second_order_block_width(d, A);
    size_t o = 0;
    auto put = [&o](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
    L.table = gate_table_layout(put, T, P, n_index, n_host, d, A, N, W);
    L.S = put(16*rows*W);
    L.idx = put(4*size_t(n_idx));
    L.shifts = put(8*size_t(n_spectra)*T*n_idx*nn);
    L.inputs_end = o;
    L.out = put(8*tiles*nn);
    L.Q = put(16*size_t(P)*dd);
    L.outputs_end = o;
    L.phases = put(16*size_t(T)*W);
    L.L = put(8*size_t(T)*nn);
    L.scale = put(16*rows*W);
    L.partial = put(8*size_t((W + width - 1)/width)*tiles*nn);
    L.end = o;
    return L;
}

bool seq_shift_shape_ok(int T, int P, int d, int A, int N, int W, int n_idx, int s_ndim, int n_spectra) {
    return seq_infid_shape_ok(T, P, d, A, N, W) && W >= 2 && (s_ndim == 1 || s_ndim == 2) && n_idx >= 1 &&
           n_idx <= A && n_spectra >= 1 && n_spectra <= 65535;
}

}  // namespace

size_t ffk_sequence_frequency_shifts_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A, int N, int W,
                                                     int n_idx, int s_ndim, int n_spectra) {
    if (!seq_shift_shape_ok(T, P, d, A, N, W, n_idx, s_ndim, n_spectra) || n_index < P || n_host < 0 || n_host > T)
        return 0;
    return seq_shift_layout(T, P, size_t(n_index), n_host, d, A, N, W, n_idx, s_ndim, n_spectra).end;
}

int ffk_sequence_frequency_shifts(ffk_resident* const* gates, const int32_t* slots, const double* gate_table,
                                  const double* gate_propagators, const double* tau, int T, const int32_t* offsets,
                                  const int32_t* index, int P, const double* omega, int W, const double* basis,
                                  int hermitian_basis, int d, int A, int N, const double* spectrum, int s_ndim,
                                  int n_spectra, const int32_t* idx, int n_idx, const double* gate_shifts, double* out,
                                  int32_t* not_finite, double* total_propagators) {
    const GateTable g{gates, slots, gate_table, gate_propagators, tau, T, offsets, index, P, omega, W, basis,
                      hermitian_basis, d, A, N};
    FFK_REQUIRE(spectrum && idx && gate_shifts && out && not_finite, "NULL argument");
    FFK_REQUIRE(ffk::sequences_supported(d, N, A) || ffk::sequences4_supported(d, N, A),
                "unsupported shape d=%d N=%d A=%d (need (d, N) = (2, 4) or (4, 16), 1 <= A <= 4)", d, N, A);
    size_t n_index = 0;
    if (int rc = check_gate_table(g, 2, &n_index)) return rc;
    FFK_REQUIRE(s_ndim == 1 || s_ndim == 2, "spectrum of %d dimensions: cross-spectra are not integrated here", s_ndim);
    FFK_REQUIRE(n_spectra >= 1 && n_spectra <= 65535, "n_spectra = %d, need 1 ... 65535", n_spectra);
    if (int rc = check_spectrum_args(s_ndim, idx, n_idx, A, d, true)) return rc;
    for (int i = 0; i < n_idx; ++i)
        for (int m = 0; m < i; ++m)
            FFK_REQUIRE(idx[i] != idx[m], "idx[%d] = idx[%d] = %d: the selected operators must be distinct", m, i,
                        idx[i]);
    const size_t tiles = size_t(n_spectra)*P*n_idx, members = size_t(n_spectra)*P;
    FFK_REQUIRE(tiles <= (size_t(1) << 26), "%zu tiles exceed one pass", tiles);
    const size_t s_rows = size_t(n_spectra)*spectrum_shape(s_ndim, n_idx).rows;
    int dev = 0;
    FFK_HIP(hipGetDevice(&dev));
    std::vector<const unsigned char*> tab;
    int n_host = 0;
    if (int rc = locate_gates(g, dev, &tab, &n_host)) return rc;
    const SeqShiftLayout L = seq_shift_layout(T, P, n_index, n_host, d, A, N, W, n_idx, s_ndim, n_spectra);
    const size_t dd = size_t(d)*d, nn = size_t(N)*N;
    PinLease pin;
    if (int rc = pin.take(L.outputs_end, dev)) return rc;
    unsigned char* hp = pin.ptr();
    hipStream_t s;
    if (int rc = resident_stream(&s)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    void* base = nullptr;
    if (int rc = arena_reserve(L.end, &base)) return rc;
    unsigned char* dp = static_cast<unsigned char*>(base);
    stage_gate_table(g, L.table, n_index, longest_first(offsets, P).data(), &tab, hp, dp);
    stage_spectrum(spectrum, true, s_rows*W, idx, n_idx, hp + L.S, hp + L.idx);
    std::memcpy(hp + L.shifts, gate_shifts, 8*size_t(n_spectra)*T*n_idx*nn);
    StreamDrain drain{s};
    auto at = [dp](size_t off) { return dp + off; };
    FFK_HIP(hipMemcpyAsync(dp, hp, L.inputs_end, hipMemcpyHostToDevice, s));
    const GateTableDevice D(dp, L.table);
    const int32_t* dIdx = reinterpret_cast<const int32_t*>(at(L.idx));
    cplx* dPh = reinterpret_cast<cplx*>(at(L.phases));
    double* dL = reinterpret_cast<double*>(at(L.L));
    cplx* dScale = reinterpret_cast<cplx*>(at(L.scale));
    FFK_HIP(launch_gate_table_front(g, D, dPh, dL, reinterpret_cast<cplx*>(at(L.Q)), s));
    FFK_HIP(ffk::launch_spectral_weights(reinterpret_cast<const cplx*>(at(L.S)), int(s_rows), W, D.omega, W, 0, dScale,
                                         s));
    FFK_HIP(ffk::launch_sequence_second_order(d, dPh, D.tab, dL, D.offsets, D.index, D.order, P, T, A, W, dScale, s_ndim,
                                              n_spectra, dIdx, n_idx, reinterpret_cast<const double*>(at(L.shifts)),
                                              reinterpret_cast<double*>(at(L.partial)),
                                              reinterpret_cast<double*>(at(L.out)), s));
    FFK_HIP(hipMemcpyAsync(hp + L.out, dp + L.out, L.outputs_end - L.out, hipMemcpyDeviceToHost, s));
    FFK_HIP(hipStreamSynchronize(s));
    if (int rc = kernel_fault_status()) return rc;
    std::memcpy(out, hp + L.out, 8*tiles*nn);
    // a (spectrum, sequence) whose tiles hold a NaN or Inf
    const double* values = reinterpret_cast<const double*>(hp + L.out);
    const size_t member = size_t(n_idx)*nn;
    for (size_t m = 0; m < members; ++m) {
        int32_t bad = 0;
        for (size_t e = 0; e < member && !bad; ++e) {
            const double v = values[m*member + e];
            bad = !(v - v == 0.0);
        }
        not_finite[m] = bad;
    }
    if (total_propagators) std::memcpy(total_propagators, hp + L.Q, 16*size_t(P)*dd);
    return FFK_OK;
}

// ---- infidelities or decay amplitudes of every prefix of many sequences from one gate table in ONE pass, under any
//      number of spectra (ff.sequence_prefix_infidelities, ff.sequence_prefix_decay_amplitudes; sequence_prefix.hip) --
namespace {

struct SeqPrefixLayout {
    GateTableLayout table;
    size_t S, idx, closing, inputs_end;                                                           // one H2D
    size_t out, outputs_end;                                                                      // one D2H
    size_t phases, L, Q, scale, partial, end;                                                     // device only
};

// doubles of one (position, spectrum, operator) in `out` and in the frequency blocks' partial sums
size_t seq_prefix_out_tile(int N, int mode) { return mode == 2 ? size_t(N)*N : mode == 1 ? size_t(N) : 1; }
size_t seq_prefix_partial_tile(int N, int mode) { return mode == 2 ? size_t(N)*N : size_t(N); }

SeqPrefixLayout seq_prefix_layout(int T, int P, size_t n_index, int n_host, int d, int A, int N, int W, int n_idx,
                                  int s_ndim, int n_spectra, int mode, bool has_closing) {
    SeqPrefixLayout L;
    const size_t dd = size_t(d)*d, nn = size_t(N)*N;
    const size_t rows = size_t(n_spectra)*spectrum_shape(s_ndim, n_idx).rows;
    const size_t members = size_t(n_spectra)*n_index*n_idx;
    const int width = ffk::sequence_prefix_block_width(d, A);
    size_t o = 0;
    auto put = [&o](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
    L.table = gate_table_layout(put, T, P, n_index, n_host, d, A, N, W);
    L.S = put(16*rows*W);
    L.idx = put(4*size_t(n_idx));
    L.closing = put(has_closing ? 4*n_index : 0);
    L.inputs_end = o;
    L.out = put(8*members*seq_prefix_out_tile(N, mode));
    L.outputs_end = o;
    L.phases = put(16*size_t(T)*W);
    L.L = put(8*size_t(T)*nn);
    L.Q = put(16*size_t(P)*dd);
    L.scale = put(16*rows*W);
    L.partial = put(8*size_t((W + width - 1)/width)*members*seq_prefix_partial_tile(N, mode));
    L.end = o;
    return L;
}

bool seq_prefix_shape_ok(int T, int P, int d, int A, int N, int W, int n_idx, int s_ndim, int n_spectra, int mode) {
    return seq_infid_shape_ok(T, P, d, A, N, W) && W >= 2 && (s_ndim == 1 || s_ndim == 2) && n_idx >= 1 &&
           n_idx <= A && n_spectra >= 1 && n_spectra <= 65535 && mode >= 0 && mode <= 2;
}

}  // namespace

size_t ffk_sequence_prefix_processes_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A, int N, int W,
                                                     int n_idx, int s_ndim, int n_spectra, int mode, int has_closing) {
    if (!seq_prefix_shape_ok(T, P, d, A, N, W, n_idx, s_ndim, n_spectra, mode) || n_index < P || n_host < 0 ||
        n_host > T)
        return 0;
    return seq_prefix_layout(T, P, size_t(n_index), n_host, d, A, N, W, n_idx, s_ndim, n_spectra, mode,
                             has_closing != 0).end;
}

int ffk_sequence_prefix_processes(ffk_resident* const* gates, const int32_t* slots, const double* gate_table,
                                  const double* gate_propagators, const double* tau, int T, const int32_t* offsets,
                                  const int32_t* index, int P, const double* omega, int W, const double* basis,
                                  int hermitian_basis, int d, int A, int N, const int32_t* closing,
                                  const double* spectrum, int s_ndim, int n_spectra, const int32_t* idx, int n_idx,
                                  int mode, double* out) {
    const GateTable g{gates, slots, gate_table, gate_propagators, tau, T, offsets, index, P, omega, W, basis,
                      hermitian_basis, d, A, N};
    FFK_REQUIRE(spectrum && idx && out, "NULL argument");
    FFK_REQUIRE(ffk::sequences_supported(d, N, A) || ffk::sequences4_supported(d, N, A),
                "unsupported shape d=%d N=%d A=%d (need (d, N) = (2, 4) or (4, 16), 1 <= A <= 4)", d, N, A);
    size_t n_index = 0;
    if (int rc = check_gate_table(g, 2, &n_index)) return rc;
    FFK_REQUIRE(s_ndim == 1 || s_ndim == 2, "spectrum of %d dimensions: cross-spectra are not integrated here", s_ndim);
    FFK_REQUIRE(n_spectra >= 1 && n_spectra <= 65535, "n_spectra = %d, need 1 ... 65535", n_spectra);
    FFK_REQUIRE(mode >= 0 && mode <= 2, "mode = %d, need 0 (infidelities), 1 (diagonal of the decay amplitudes) or 2 "
                "(decay amplitudes)", mode);
    if (int rc = check_spectrum_args(s_ndim, idx, n_idx, A, d, true)) return rc;
    for (int i = 0; i < n_idx; ++i)
        for (int m = 0; m < i; ++m)
            FFK_REQUIRE(idx[i] != idx[m], "idx[%d] = idx[%d] = %d: the selected operators must be distinct", m, i,
                        idx[i]);
    if (closing)
        for (size_t k = 0; k < n_index; ++k)
            FFK_REQUIRE(closing[k] >= 0 && closing[k] < T, "closing[%zu] = %d outside [0, %d)", k, closing[k], T);
    const size_t members = size_t(n_spectra)*n_index*n_idx;
    FFK_REQUIRE(members*seq_prefix_partial_tile(N, mode) <= (size_t(1) << 32),
                "%zu prefix results exceed one pass", members);
    const size_t s_rows = size_t(n_spectra)*spectrum_shape(s_ndim, n_idx).rows;
    int dev = 0;
    FFK_HIP(hipGetDevice(&dev));
    std::vector<const unsigned char*> tab;
    int n_host = 0;
    if (int rc = locate_gates(g, dev, &tab, &n_host)) return rc;
    const SeqPrefixLayout L = seq_prefix_layout(T, P, n_index, n_host, d, A, N, W, n_idx, s_ndim, n_spectra, mode,
                                                closing != nullptr);
    PinLease pin;
    if (int rc = pin.take(L.outputs_end, dev)) return rc;
    unsigned char* hp = pin.ptr();
    hipStream_t s;
    if (int rc = resident_stream(&s)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    void* base = nullptr;
    if (int rc = arena_reserve(L.end, &base)) return rc;
    unsigned char* dp = static_cast<unsigned char*>(base);
    stage_gate_table(g, L.table, n_index, longest_first(offsets, P).data(), &tab, hp, dp);
    stage_spectrum(spectrum, true, s_rows*W, idx, n_idx, hp + L.S, hp + L.idx);
    if (closing) std::memcpy(hp + L.closing, closing, 4*n_index);
    StreamDrain drain{s};
    auto at = [dp](size_t off) { return dp + off; };
    FFK_HIP(hipMemcpyAsync(dp, hp, L.inputs_end, hipMemcpyHostToDevice, s));
    const GateTableDevice D(dp, L.table);
    const int32_t* dIdx = reinterpret_cast<const int32_t*>(at(L.idx));
    cplx* dPh = reinterpret_cast<cplx*>(at(L.phases));
    double* dL = reinterpret_cast<double*>(at(L.L));
    cplx* dScale = reinterpret_cast<cplx*>(at(L.scale));
    FFK_HIP(launch_gate_table_front(g, D, dPh, dL, reinterpret_cast<cplx*>(at(L.Q)), s));
    FFK_HIP(ffk::launch_spectral_weights(reinterpret_cast<const cplx*>(at(L.S)), int(s_rows), W, D.omega, W, 0, dScale,
                                         s));
    FFK_HIP(ffk::launch_sequence_prefix(d, dPh, D.tab, dL, D.offsets, D.index,
                                        closing ? reinterpret_cast<const int32_t*>(at(L.closing)) : nullptr, D.order, P,
                                        n_index, T, A, W, dScale, s_ndim, n_spectra, dIdx, n_idx, mode,
                                        reinterpret_cast<double*>(at(L.partial)),
                                        reinterpret_cast<double*>(at(L.out)), s));
    FFK_HIP(hipMemcpyAsync(hp + L.out, dp + L.out, L.outputs_end - L.out, hipMemcpyDeviceToHost, s));
    FFK_HIP(hipStreamSynchronize(s));
    if (int rc = kernel_fault_status()) return rc;
    std::memcpy(out, hp + L.out, 8*members*seq_prefix_out_tile(N, mode));
    return FFK_OK;
}

// ---- frequency shifts (second order) of every prefix of many sequences from one gate table in ONE pass, under any
//      number of spectra (ff.sequence_prefix_frequency_shifts; sequence_prefix_second_order.hip) ----------------------
namespace {

struct SeqPrefixShiftLayout {
    GateTableLayout table;
    size_t S, idx, closing, shifts, inputs_end;                                                   // one H2D
    size_t out, outputs_end;                                                                      // one D2H
    size_t phases, L, Q, scale, partial, end;                                                     // device only
};

SeqPrefixShiftLayout seq_prefix_shift_layout(int T, int P, size_t n_index, int n_host, int d, int A, int N, int W,
                                             int n_idx, int s_ndim, int n_spectra, bool has_closing) {
    SeqPrefixShiftLayout L;
    const size_t dd = size_t(d)*d, nn = size_t(N)*N;
    const size_t rows = size_t(n_spectra)*spectrum_shape(s_ndim, n_idx).rows;
    const size_t tiles = size_t(n_spectra)*n_index*n_idx;
    const int width = ffk::sequence_prefix_second_order_block_width(d, A);
    size_t o = 0;
    auto put = [&o](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
    L.table = gate_table_layout(put, T, P, n_index, n_host, d, A, N, W);
    L.S = put(16*rows*W);
    L.idx = put(4*size_t(n_idx));
    L.closing = put(has_closing ? 4*n_index : 0);
    L.shifts = put(8*size_t(n_spectra)*T*n_idx*nn);
    L.inputs_end = o;
    L.out = put(8*tiles*nn);
    L.outputs_end = o;
    L.phases = put(16*size_t(T)*W);
    L.L = put(8*size_t(T)*nn);
    L.Q = put(16*size_t(P)*dd);
    L.scale = put(16*rows*W);
    L.partial = put(8*size_t((W + width - 1)/width)*tiles*nn);
    L.end = o;
    return L;
}

}  // namespace

size_t ffk_sequence_prefix_frequency_shifts_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A, int N,
                                                            int W, int n_idx, int s_ndim, int n_spectra,
                                                            int has_closing) {
    if (!seq_shift_shape_ok(T, P, d, A, N, W, n_idx, s_ndim, n_spectra) || n_index < P || n_host < 0 || n_host > T)
        return 0;
    return seq_prefix_shift_layout(T, P, size_t(n_index), n_host, d, A, N, W, n_idx, s_ndim, n_spectra,
                                   has_closing != 0).end;
}

int ffk_sequence_prefix_frequency_shifts(ffk_resident* const* gates, const int32_t* slots, const double* gate_table,
                                         const double* gate_propagators, const double* tau, int T,
                                         const int32_t* offsets, const int32_t* index, int P, const double* omega,
                                         int W, const double* basis, int hermitian_basis, int d, int A, int N,
                                         const int32_t* closing, const double* spectrum, int s_ndim, int n_spectra,
                                         const int32_t* idx, int n_idx, const double* gate_shifts, double* out) {
    const GateTable g{gates, slots, gate_table, gate_propagators, tau, T, offsets, index, P, omega, W, basis,
                      hermitian_basis, d, A, N};
    FFK_REQUIRE(spectrum && idx && gate_shifts && out, "NULL argument");
    FFK_REQUIRE(ffk::sequences_supported(d, N, A) || ffk::sequences4_supported(d, N, A),
                "unsupported shape d=%d N=%d A=%d (need (d, N) = (2, 4) or (4, 16), 1 <= A <= 4)", d, N, A);
    size_t n_index = 0;
    if (int rc = check_gate_table(g, 2, &n_index)) return rc;
    FFK_REQUIRE(s_ndim == 1 || s_ndim == 2, "spectrum of %d dimensions: cross-spectra are not integrated here", s_ndim);
    FFK_REQUIRE(n_spectra >= 1 && n_spectra <= 65535, "n_spectra = %d, need 1 ... 65535", n_spectra);
    if (int rc = check_spectrum_args(s_ndim, idx, n_idx, A, d, true)) return rc;
    for (int i = 0; i < n_idx; ++i)
        for (int m = 0; m < i; ++m)
            FFK_REQUIRE(idx[i] != idx[m], "idx[%d] = idx[%d] = %d: the selected operators must be distinct", m, i,
                        idx[i]);
    if (closing)
        for (size_t k = 0; k < n_index; ++k)
            FFK_REQUIRE(closing[k] >= 0 && closing[k] < T, "closing[%zu] = %d outside [0, %d)", k, closing[k], T);
    const size_t nn = size_t(N)*N;
    const size_t tiles = size_t(n_spectra)*n_index*n_idx;
    FFK_REQUIRE(tiles*nn <= (size_t(1) << 32), "%zu prefix tiles exceed one pass", tiles);
    const size_t s_rows = size_t(n_spectra)*spectrum_shape(s_ndim, n_idx).rows;
    int dev = 0;
    FFK_HIP(hipGetDevice(&dev));
    std::vector<const unsigned char*> tab;
    int n_host = 0;
    if (int rc = locate_gates(g, dev, &tab, &n_host)) return rc;
    const SeqPrefixShiftLayout L = seq_prefix_shift_layout(T, P, n_index, n_host, d, A, N, W, n_idx, s_ndim, n_spectra,
                                                           closing != nullptr);
    PinLease pin;
    if (int rc = pin.take(L.outputs_end, dev)) return rc;
    unsigned char* hp = pin.ptr();
    hipStream_t s;
    if (int rc = resident_stream(&s)) return rc;
    std::lock_guard<std::mutex> lock(g_arena.mu);
    void* base = nullptr;
    if (int rc = arena_reserve(L.end, &base)) return rc;
    unsigned char* dp = static_cast<unsigned char*>(base);
    stage_gate_table(g, L.table, n_index, longest_first(offsets, P).data(), &tab, hp, dp);
    stage_spectrum(spectrum, true, s_rows*W, idx, n_idx, hp + L.S, hp + L.idx);
    if (closing) std::memcpy(hp + L.closing, closing, 4*n_index);
    std::memcpy(hp + L.shifts, gate_shifts, 8*size_t(n_spectra)*T*n_idx*nn);
    StreamDrain drain{s};
    auto at = [dp](size_t off) { return dp + off; };
    FFK_HIP(hipMemcpyAsync(dp, hp, L.inputs_end, hipMemcpyHostToDevice, s));
    const GateTableDevice D(dp, L.table);
    const int32_t* dIdx = reinterpret_cast<const int32_t*>(at(L.idx));
    cplx* dPh = reinterpret_cast<cplx*>(at(L.phases));
    double* dL = reinterpret_cast<double*>(at(L.L));
    cplx* dScale = reinterpret_cast<cplx*>(at(L.scale));
    FFK_HIP(launch_gate_table_front(g, D, dPh, dL, reinterpret_cast<cplx*>(at(L.Q)), s));
    FFK_HIP(ffk::launch_spectral_weights(reinterpret_cast<const cplx*>(at(L.S)), int(s_rows), W, D.omega, W, 0, dScale,
                                         s));
    FFK_HIP(ffk::launch_sequence_prefix_second_order(
        d, dPh, D.tab, dL, D.offsets, D.index, closing ? reinterpret_cast<const int32_t*>(at(L.closing)) : nullptr,
        D.order, P, n_index, T, A, W, dScale, s_ndim, n_spectra, dIdx, n_idx,
        reinterpret_cast<const double*>(at(L.shifts)), reinterpret_cast<double*>(at(L.partial)),
        reinterpret_cast<double*>(at(L.out)), s));
    FFK_HIP(hipMemcpyAsync(hp + L.out, dp + L.out, L.outputs_end - L.out, hipMemcpyDeviceToHost, s));
    FFK_HIP(hipStreamSynchronize(s));
    if (int rc = kernel_fault_status()) return rc;
    std::memcpy(out, hp + L.out, 8*tiles*nn);
    return FFK_OK;
}

}  // extern "C"

#if defined(FFK_HOST_SANITIZE)
// ---------------------------------------------------------------------------------------------
// Host-logic self test for the sanitizer variant: arena growth, block-pool reuse and eviction, every
// workspace layout sliced with the size its *_workspace_bytes query reports and each slice written
// end to end (an overrun of a slice or of the reservation is a heap-buffer-overflow under ASan).
// ---------------------------------------------------------------------------------------------
#include <random>
extern "C" int ffk_selftest_host(int rounds, unsigned seed, char* report, int report_len) {
    if (rounds < 0) {
        // negative control: a deliberate one-byte overrun, which the sanitizer must report
        volatile unsigned char* p = static_cast<unsigned char*>(std::malloc(16));
        p[16] = 1;
        std::free(const_cast<unsigned char*>(p));
        return 0;
    }
    std::mt19937 rng(seed);
    auto pick = [&](int lo, int hi) { return lo + static_cast<int>(rng() % static_cast<unsigned>(hi - lo + 1)); };
    long checked = 0;
    auto touch = [&](void* p, size_t n) {
        if (p && n) {
            std::memset(p, 0xA5, n);
            ++checked;
        }
    };
    for (int r = 0; r < rounds; ++r) {
        const int d = pick(2, FFK_MAX_D_TEMPLATED), G = pick(1, 300), A = pick(1, 9), W = pick(1, 700);
        const int N = pick(1, d*d);
        // (a) arena: reserve, write all of it, grow, shrink requests
        void* base = nullptr;
        const size_t want = size_t(pick(1, 1 << 20))*pick(1, 8);
        {
            std::lock_guard<std::mutex> lock(g_arena.mu);
            if (arena_reserve(want, &base) != FFK_OK) return -1;
            touch(base, g_arena.size);
        }
        // (a') the kernels' fault words: one per host thread -- a word set for this thread is seen (and cleared) by this
        // thread's check and by no other thread's; the word the launchers would hand their kernels is this thread's
        if (r == 0) {
            int* mine = ffk::kernel_fault_word();
            if (mine == nullptr) return -20;
            if (kernel_fault_peek(false) != 0) return -21;
            *static_cast<volatile int*>(mine) = ffk::kernel_fault_code_for_selftest();
            int other_saw = -1, other_slot = -1;
            int* others = nullptr;
            std::thread peer([&] {
                others = ffk::kernel_fault_word();
                other_slot = kernel_fault_slot_for_selftest();
                other_saw = kernel_fault_peek(true);          // must not see (or clear) this thread's fault
            });
            peer.join();
            if (others == nullptr || others == mine || other_slot == kernel_fault_slot_for_selftest()) return -22;
            if (other_saw != 0) return -23;
            if (kernel_fault_stale() != FFK_EKERNEL) return -24;      // reported to the thread that owns it, once
            if (kernel_fault_peek(false) != 0 || kernel_fault_status() != FFK_OK) return -25;
            if (ffk::kernel_fault_word() != mine) return -26;          // a thread keeps its word
        }
        // (b) control-matrix workspace: the slices of ffk_control_matrix_dev
        {
            const ffk::AccumGeometry geo = ffk::accumulate_geometry(W, A, G, d, 0);
            const size_t bytes = ffk_control_matrix_workspace_bytes(W, N, A, G, d);
            if (bytes < ctrl_ws_bytes(W, N, A, G, d, geo.chunks)) return -2;
            void* ws = std::malloc(bytes);
            Bump b(ws, bytes);
            double* segtab = b.take<double>(size_t(G)*ffk::seg_stride(d));
            cplx* Tc = b.take<cplx>(size_t(G)*d*d);
            cplx* ops = b.take<cplx>(size_t(G)*(1 + A)*d*d);
            cplx* Ypart = b.take<cplx>(size_t(geo.chunks)*A*d*d*W);
            cplx* Bt = b.take<cplx>(size_t(A)*d*d*W);
            void* ews = b.take<unsigned char>(ffk::expand_workspace_bytes(N, d));
            if (!segtab || !Tc || !ops || !Ypart || !Bt || !ews) { std::free(ws); return -3; }
            touch(segtab, sizeof(double)*size_t(G)*ffk::seg_stride(d));
            touch(Tc, sizeof(cplx)*size_t(G)*d*d);
            touch(ops, sizeof(cplx)*size_t(G)*(1 + A)*d*d);
            touch(Ypart, sizeof(cplx)*size_t(geo.chunks)*A*d*d*W);
            touch(Bt, sizeof(cplx)*size_t(A)*d*d*W);
            touch(ews, ffk::expand_workspace_bytes(N, d));
            int *nnz, *rows;
            cplx* vals;
            ffk::expand_workspace_slices(ews, N, d, &nnz, &rows, &vals);
            touch(nnz, sizeof(int)*N);
            touch(rows, sizeof(int)*size_t(N)*d*d);
            touch(vals, sizeof(cplx)*size_t(N)*d*d);
            std::free(ws);
        }
        // (c) diagonalize + pipeline workspaces
        {
            const size_t dwsb = ffk_diagonalize_workspace_bytes(G, d);
            void* ws = std::malloc(dwsb);
            const DiagWs w = slice_diag_ws(ws, dwsb, G, d);
            touch(w.status, sizeof(int)*G);
            touch(w.seg_prop, sizeof(cplx)*size_t(G)*d*d);
            touch(w.qloc, sizeof(cplx)*size_t(G + 1)*d*d);
            std::free(ws);
            const int n_idx = pick(1, A), s_ndim = pick(1, 3);
            const size_t pb = ffk_pipeline_workspace_bytes(W, N, A, G, d, n_idx, s_ndim);
            if (pb < dwsb + ffk_control_matrix_workspace_bytes(W, N, A, G, d)) return -4;
            void* pws = std::malloc(pb);
            Bump b(pws, pb);
            void* a1 = b.take<unsigned char>(dwsb);
            void* a2 = b.take<unsigned char>(ffk_control_matrix_workspace_bytes(W, N, A, G, d));
            double* D = b.take<double>(size_t(G)*d);
            double* V = b.take<double>(2*size_t(G)*d*d);
            double* Q = b.take<double>(2*size_t(G + 1)*d*d);
            double* R = b.take<double>(2*size_t(A)*N*W);
            double* F = b.take<double>(2*size_t(A)*A*W);
            void* iws = b.take<unsigned char>(ffk_infidelity_workspace_bytes(W, n_idx, s_ndim));
            if (!a1 || !a2 || !D || !V || !Q || !R || !F || !iws) { std::free(pws); return -5; }
            touch(F, 16*size_t(A)*A*W);
            touch(iws, ffk_infidelity_workspace_bytes(W, n_idx, s_ndim));
            std::free(pws);
        }
        // (d) sequence scratch of the concatenation entry points
        {
            const int Gs = pick(1, 1200), which = pick(0, 1);
            const bool herm = pick(0, 1) != 0, wantF = which == 0 && pick(0, 1);
            const int d2 = pick(2, 4), N2 = d2*d2, A2 = pick(1, 3), W2 = pick(1, 300);
            const size_t sb = sequence_scratch_bytes(Gs, d2, A2, N2, W2, which, herm, wantF);
            void* ws = std::malloc(sb);
            Bump a(ws, sb);
            const size_t dd = size_t(d2)*d2;
            const int nl = Gs > 1 ? Gs - 1 : 1;
            cplx* dSeq = a.take<cplx>(size_t(Gs)*dd);
            cplx* dQ = a.take<cplx>(size_t(Gs + 1)*dd);
            double* dL = a.take<double>((herm ? 1 : 2)*size_t(nl)*N2*N2);
            double* dO = a.take<double>(2*(which ? size_t(Gs) : 1)*A2*N2*W2);
            void* w1 = a.take<unsigned char>(ffk::scan_workspace_bytes(Gs, d2));
            void* w2 = a.take<unsigned char>(ffk::liouville_workspace_bytes(nl, d2, N2));
            void* w3 = a.take<unsigned char>(ffk_control_matrix_from_atomic_workspace_bytes(Gs, A2, N2, W2));
            double* dF = wantF ? a.take<double>(2*size_t(A2)*A2*W2) : nullptr;
            if (!dSeq || !dQ || !dL || !dO || !w1 || !w2 || !w3 || (wantF && !dF)) { std::free(ws); return -6; }
            touch(dSeq, 16*size_t(Gs)*dd);
            touch(dQ, 16*size_t(Gs + 1)*dd);
            touch(dL, (herm ? 8 : 16)*size_t(nl)*N2*N2);
            touch(dO, 16*(which ? size_t(Gs) : 1)*A2*N2*W2);
            touch(w3, ffk_control_matrix_from_atomic_workspace_bytes(Gs, A2, N2, W2));
            if (dF) touch(dF, 16*size_t(A2)*A2*W2);
            std::free(ws);
        }
        // (e) block pools: take / write / give in random order, past the eviction bound
        {
            std::vector<Block> held;
            for (int k = 0; k < 40; ++k) {
                if (held.empty() || pick(0, 2)) {
                    Block b = {nullptr, 0, -1};
                    BlockPool& pool = pick(0, 1) ? g_dev_pool : g_pin_pool;
                    const size_t bytes = size_t(pick(1, 1 << 18));
                    if (pool.take(bytes, 0, &b) != FFK_OK || b.size < bytes) return -7;
                    touch(b.ptr, b.size);
                    b.device = (&pool == &g_dev_pool) ? 0 : -1;
                    held.push_back(b);
                } else {
                    const int i = pick(0, int(held.size()) - 1);
                    (held[i].device == 0 ? g_dev_pool : g_pin_pool).give(held[i]);
                    held.erase(held.begin() + i);
                }
            }
            for (const Block& b : held) (b.device == 0 ? g_dev_pool : g_pin_pool).give(b);
        }
        // (f) the layouts of the resident, batched, sequence and process passes: offsets ascending (no array starts
        // inside another), every array inside `end`; where a workspace query exists, `end` is what it reports
        {
            // (a layout is a struct of offsets declared in the order in which they are laid out)
            auto ascending = [](const auto& L) {
                const size_t* o = reinterpret_cast<const size_t*>(&L);
                return std::is_sorted(o, o + sizeof(L)/sizeof(size_t));           // (`end` is the last of them)
            };
            const int P = pick(1, 40), n_c = pick(1, 5), T = pick(1, 30), n_host = pick(0, T);
            const int n_idx = pick(1, A), s_ndim = pick(1, 3), n_index = P + pick(0, 500);
            const SpectrumShape sh = spectrum_shape(s_ndim, n_idx);
            const ResidentLayout RL = resident_layout(G, d, W, N, A);
            if (!ascending(RL) || RL.infid + 8*size_t(A)*A > RL.end) return -8;
            const BatchLayout BL = batch_layout(P, n_c, G, d, W, N, A, sh, n_idx);
            if (!ascending(BL) || BL.R + 16*size_t(P)*A*N*W > BL.end) return -13;
            const int As = pick(1, 4), si = pick(1, As);       // the sequence pass: d = 2, N = 4, A <= 4
            const SeqLayout SL = seq_layout(T, P, size_t(n_index), n_host, 2, As, 4, W, spectrum_shape(s_ndim, si), si);
            if (!ascending(SL) || SL.L + 8*size_t(T)*16 > SL.end ||
                SL.end != ffk_concatenate_sequences_workspace_bytes(T, P, n_index, n_host, 2, As, 4, W, si, s_ndim))
                return -14;
            // the correlation pass: the workspace query bounds the layout of any lengths of at most 256 positions
            const int sc = pick(1, 2);
            const size_t longest = std::min(size_t(n_index - P + 1), size_t(256));
            const size_t total = longest*longest + size_t(P - 1);      // one sequence as long as can be, the rest of 1
            const CorrLayout CL = corr_layout(T, P, size_t(n_index), n_host, 2, As, 4, W, spectrum_shape(sc, si), si, total);
            if (n_index - P + 1 <= 256 &&
                (!ascending(CL) || CL.part + 8*size_t(ffk::correlation_slabs(W, nullptr))*si*total > CL.end ||
                 CL.end > ffk_sequence_correlation_infidelities_workspace_bytes(T, P, n_index, n_host, 2, As, 4, W, si, sc)))
                return -16;
            // the frequency-shift pass of the sequences: what the query reports, the partial tiles inside it
            const int sn = pick(1, 2), ks = pick(1, 5);
            if (W >= 2) {
                const SeqShiftLayout HL = seq_shift_layout(T, P, size_t(n_index), n_host, 2, As, 4, W, si, sn, ks);
                if (!ascending(HL) || HL.partial + 8*size_t((W + 63)/64)*ks*P*si*16 > HL.end ||
                    HL.end != ffk_sequence_frequency_shifts_workspace_bytes(T, P, n_index, n_host, 2, As, 4, W, si, sn, ks))
                    return -17;
                // the prefix pass: what the query reports, the partial sums of every position inside it
                const int pm = pick(0, 2), pc = pick(0, 1);
                const SeqPrefixLayout XL = seq_prefix_layout(T, P, size_t(n_index), n_host, 2, As, 4, W, si, sn, ks, pm,
                                                             pc != 0);
                if (!ascending(XL) ||
                    XL.partial + 8*size_t((W + 63)/64)*ks*n_index*si*seq_prefix_partial_tile(4, pm) > XL.end ||
                    XL.end != ffk_sequence_prefix_processes_workspace_bytes(T, P, n_index, n_host, 2, As, 4, W, si, sn,
                                                                            ks, pm, pc))
                    return -27;
                // the process pass of the sequences, two-qubit gates: any stage, the cumulant workspace last (below stage
                // 3 the requested array IS `out`, so gamma or K names an earlier offset a second time)
                const int stage = pick(1, 3);
                const size_t tiles = size_t(ks)*P*si;
                const SeqProcLayout QL = seq_proc_layout(T, P, size_t(n_index), n_host, 4, As, 16, W, si, sn, ks, stage,
                                                         false);
                if ((stage == 3 && !ascending(QL)) || QL.inputs_end > QL.out || QL.outputs_end > QL.phases ||
                    QL.cumulant + (stage >= 2 ? ffk::cumulant_workspace_bytes(tiles, 16, 4) : 0) > QL.end ||
                    QL.end != ffk_sequence_processes_workspace_bytes(T, P, n_index, n_host, 4, As, 16, W, si, sn, ks, stage))
                    return -18;
            }
            // the infidelity pass of the sequences, either dimension
            const int di = pick(0, 1) ? 4 : 2;
            const SeqInfidLayout IL = seq_infid_layout(T, P, size_t(n_index), n_host, di, As, di*di, W,
                                                       spectrum_shape(s_ndim, si), si);
            if (!ascending(IL) || IL.L + 8*size_t(T)*di*di*di*di > IL.end ||
                IL.end != ffk_sequence_infidelities_workspace_bytes(T, P, n_index, n_host, di, As, di*di, W, si, s_ndim))
                return -19;
            const int Np = N < 16 ? N : 16, hosts = pick(0, P);
            const ProcLayout PL = proc_layout(P, hosts, A, Np, W, d, n_idx, s_ndim, false, true, true, true);
            if (!ascending(PL) || PL.end != ffk_resident_batch_processes_workspace_bytes(P, hosts, A, Np, W, d, n_idx, s_ndim))
                return -15;
            ffk_resident* h = nullptr;
            if (ffk_resident_create(&h) != FFK_OK) return -9;
            if (ffk_resident_destroy(h) != FFK_OK) return -10;
        }
    }
    if (g_dev_pool.release() != FFK_OK || g_pin_pool.release() != FFK_OK) return -11;
    if (ffk_release_arena() != FFK_OK) return -12;
    if (report && report_len > 0)
        snprintf(report, report_len, "%d rounds, %ld regions written end to end, pools and arena released", rounds, checked);
    return 0;
}
#endif

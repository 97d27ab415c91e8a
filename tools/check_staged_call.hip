// Stand-alone host check of StagedCall (filter_functions_amd/csrc/ffk_api_common.h), the object every host-pointer
// entry point stages its arrays through: for random shapes it declares inputs (whole, partly copied, not copied,
// without a host array), outputs, empty and non-empty workspaces, stages them into a reservation of EXACTLY the
// declared size on the C heap, and writes every slice end to end.  Under AddressSanitizer / UBSan an overrun of a
// slice or of the reservation, or arithmetic on a null base, is reported; overlap and copies are checked here.
// Needs no GPU and is never run on one:
//   hipcc -std=c++17 --offload-arch=gfx950 -Wno-unused-function -DFFK_HOST_SANITIZE -Xarch_host -fsanitize=address,undefined \
//         -Iinclude -Ifilter_functions_amd/csrc tools/check_staged_call.hip -o build/check_staged_call
//   build/check_staged_call [rounds] [seed]
#include <random>

#include "ffk_api_common.h"

namespace ffk_api {
thread_local std::string g_error;
Arena g_arena;
int fail(int code, const char* fmt, ...) {
    g_error = fmt;
    return code;
}
int kernel_fault_status() { return FFK_OK; }
// exactly the bytes asked for, and a fresh block for every call
int arena_reserve(size_t bytes, void** out) {
    std::free(g_arena.ptr);
    g_arena.ptr = std::malloc(bytes ? bytes : 1);
    g_arena.size = bytes;
    *out = g_arena.ptr;
    return g_arena.ptr ? FFK_OK : FFK_ENOMEM;
}
}  // namespace ffk_api

namespace {
struct Span {
    unsigned char* at;
    size_t bytes;
};
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "line %d: %s (round %d)\n", __LINE__, #cond, r); \
            return 1;                                                           \
        }                                                                       \
    } while (0)
}  // namespace

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 200;
    std::mt19937 rng(argc > 2 ? static_cast<unsigned>(std::atoi(argv[2])) : 1u);
    auto pick = [&](int lo, int hi) { return lo + static_cast<int>(rng() % static_cast<unsigned>(hi - lo + 1)); };
    for (int r = 0; r < rounds; ++r) {
        const int d = pick(2, 8), G = pick(1, 40), A = pick(1, 5), W = pick(1, 300);
        const int N = pick(0, 1) ? d*d : 0;                       // N = 0: an entry point without a basis
        const size_t dd = size_t(d)*d;
        std::vector<double> host(2*size_t(G + 1)*dd + 2*size_t(A + N)*dd + size_t(A)*G + W + 64);
        for (size_t i = 0; i < host.size(); ++i) host[i] = double(i);
        const double* h = host.data();
        StagedCall c;
        std::vector<Span> spans;
        const PulseSlices p = stage_pulse(c, h, h, h, h, W, N ? h : nullptr, N, h, A, h, h, h, G, d);
        const size_t n_partial = size_t(pick(1, 50)), n_copied = size_t(pick(0, int(n_partial)));
        const auto partial = c.in<cplx>(h, n_partial, n_copied);
        const auto optional = c.in<double>(nullptr, size_t(pick(1, 50)));
        const auto idx = c.in<int32_t>(h, size_t(pick(1, 9)));
        const auto out = c.out<cplx>(size_t(pick(0, 2000)));
        const auto none = c.workspace(0);
        const auto ws = c.workspace(256*size_t(pick(1, 20)));
        CHECK(c[out] == nullptr);                                 // no pointers before stage()
        CHECK(c.stage() == FFK_OK);
        auto add = [&](auto slice) {
            using T = std::remove_pointer_t<decltype(c[slice])>;
            spans.push_back({reinterpret_cast<unsigned char*>(c[slice]), sizeof(T)*slice.count});
            return c[slice] != nullptr;
        };
        CHECK(add(p.eigvals) && add(p.eigvecs) && add(p.propagators) && add(p.omega) && add(p.basis) &&
              add(p.n_opers) && add(p.n_coeffs) && add(p.dt) && add(p.t));
        CHECK(add(partial) && add(optional) && add(idx) && add(out) && add(none) && add(ws));
        // the inputs arrived, as many elements as were to be copied
        CHECK(std::memcmp(c[p.propagators], h, 16*size_t(G + 1)*dd) == 0);
        CHECK(std::memcmp(c[p.t], h, 8*size_t(G + 1)) == 0);
        CHECK(std::memcmp(c[partial], h, 16*n_copied) == 0);
        CHECK(std::memcmp(c[idx], h, 4*idx.count) == 0);
        // every slice written end to end with a byte of its own, aligned, inside the reservation, none overlapping
        unsigned char* base = static_cast<unsigned char*>(g_arena.ptr);
        for (size_t i = 0; i < spans.size(); ++i) {
            CHECK((spans[i].at - base) % 256 == 0 && spans[i].at + spans[i].bytes <= base + g_arena.size);
            std::memset(spans[i].at, int(i + 1), spans[i].bytes);
        }
        for (size_t i = 0; i < spans.size(); ++i)
            for (size_t k = 0; k < spans[i].bytes; ++k) CHECK(spans[i].at[k] == i + 1);
        // an empty workspace still has a place of its own
        CHECK(c[none] != reinterpret_cast<unsigned char*>(c[out]) && c[none] != c[ws]);
        // a callee's bump allocator ends where the declared workspace ends
        Bump b = c.bump(ws);
        CHECK(b.size == ws.count && b.take<unsigned char>(ws.count + 1) == nullptr);
        CHECK(b.take<unsigned char>(ws.count) == c[ws] && b.take<unsigned char>(1) == nullptr);
        // a slice that was not declared on this call is refused
        StagedCall::Slice<double> foreign;
        foreign.at = g_arena.size;
        foreign.count = 1;
        CHECK(c[foreign] == nullptr && c.copy_back(host.data(), foreign) == FFK_EINVAL);
        std::vector<cplx> back(out.count + 1);
        CHECK(c.copy_back(back.data(), out) == FFK_OK);
        CHECK(out.count == 0 || reinterpret_cast<unsigned char*>(back.data())[0] == 13);
        CHECK(r % 2 ? c.finish() == FFK_OK : c.finish_with_fault_status() == FFK_OK);
    }
    std::free(g_arena.ptr);
    g_arena.ptr = nullptr;
    std::printf("StagedCall: %d rounds ok\n", rounds);
    return 0;
}

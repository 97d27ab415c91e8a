// Stand-alone host check of the gate table that the passes over many gate sequences share
// (filter_functions_amd/csrc/ffk_api_gate_table.h): for random tables -- T gates of d = 2 or 4, some with a handle, some
// rows of a host table, P sequences of random lengths -- it lays out the common head plus a tail of random size, stages
// the table into a pinned side of EXACTLY inputs_end bytes on the C heap and verifies every staged array against its
// source, the pointer table against the located gates, the order, the typed device view after a plain copy, and that
// the checker refuses malformed tables with the messages the entry points report.  Under AddressSanitizer / UBSan an
// overrun of an array or of the block is reported.  Needs no GPU and is never run on one:
//   hipcc -std=c++17 --offload-arch=gfx950 -Wno-unused-function -DFFK_HOST_SANITIZE -Xarch_host -fsanitize=address,undefined \
//         -Iinclude -Ifilter_functions_amd/csrc tools/check_gate_table.hip -o build/check_gate_table
//   build/check_gate_table [rounds] [seed]
#include <random>

#include "ffk_api_gate_table.h"

namespace ffk_api {
thread_local std::string g_error;
int fail(int code, const char* fmt, ...) {
    char text[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    g_error = text;
    return code;
}
}  // namespace ffk_api

namespace {
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "line %d: %s (round %d)\n", __LINE__, #cond, r); \
            return 1;                                                           \
        }                                                                       \
    } while (0)

// whether the checker says `message` of a table of ONE gate and two sequences with these CSR arrays (NULL: accepts it)
bool verdict(const int32_t (&offsets)[3], const int32_t (&index)[3], int d, int min_W, const char* message) {
    ffk_resident* none = nullptr;
    const int32_t slot = -1;
    const double x[2*16*16] = {};
    const GateTable g{&none, &slot, x, x, x, 1, offsets, index, 2, x, 7, x, 1, d, 1, d*d};
    size_t n_index = 0;
    const int rc = check_gate_table(g, min_W, &n_index);
    return message ? rc == FFK_EINVAL && std::strcmp(g_error.c_str(), message) == 0 : rc == FFK_OK && n_index == 3;
}
}  // namespace

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 200;
    std::mt19937 rng(argc > 2 ? static_cast<unsigned>(std::atoi(argv[2])) : 1u);
    auto pick = [&](int lo, int hi) { return lo + static_cast<int>(rng() % static_cast<unsigned>(hi - lo + 1)); };
    for (int r = 0; r < rounds; ++r) {
        const int d = pick(0, 1) ? 4 : 2, N = d*d, A = pick(1, 4), W = pick(1, 70), T = pick(1, 12), P = pick(1, 20);
        const int min_W = pick(1, 2);
        const size_t dd = size_t(d)*d, row = 16*size_t(A)*N*W;
        // the table: sequences, gates with a handle (a device address that is never read) or a row of the host table
        std::vector<int32_t> offsets(P + 1, 0), index;
        for (int p = 0; p < P; ++p) {
            const int length = pick(1, 9);
            offsets[p + 1] = offsets[p] + length;
            for (int k = 0; k < length; ++k) index.push_back(pick(0, T - 1));
        }
        ffk_resident* gates[12] = {};
        int32_t slots[12];
        static const unsigned char elsewhere[12] = {};
        const unsigned char* located[12] = {};
        int n_host = 0;
        for (int k = 0; k < T; ++k) {
            slots[k] = -1;
            if (pick(0, 2) == 0)
                located[k] = elsewhere + k;
            else
                ++n_host;
        }
        double counter = 1.0;
        auto values = [&counter](size_t n) {
            std::vector<double> v(n);
            for (double& x : v) x = counter++;
            return v;
        };
        const std::vector<double> tau = values(T), omega = values(W), basis = values(2*size_t(N)*dd);
        const std::vector<double> U = values(2*size_t(T)*dd), host_table = values(row/8*size_t(n_host));
        const GateTable g{gates, slots, n_host ? host_table.data() : nullptr, U.data(), tau.data(), T,
                          offsets.data(), index.data(), P, omega.data(), W, basis.data(), 1, d, A, N};
        size_t n_index = 0;
        if (W < min_W) {
            CHECK(check_gate_table(g, min_W, &n_index) == FFK_EINVAL);
            CHECK(g_error.find("(need W >= 2)") != std::string::npos);
            continue;
        }
        CHECK(check_gate_table(g, min_W, &n_index) == FFK_OK && n_index == index.size());
        // the head of a layout, then what a pass would add
        size_t o = 0;
        auto put = [&o](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
        const GateTableLayout L = gate_table_layout(put, T, P, n_index, n_host, d, A, N, W);
        const size_t tail = put(size_t(pick(0, 5000)));
        const size_t inputs_end = o;
        const size_t* first = &L.offsets;
        CHECK(std::is_sorted(first, first + sizeof(L)/sizeof(size_t)) && L.offsets == 0);
        CHECK(L.host + row*size_t(n_host) <= tail && L.tab + 8*size_t(T) <= L.host);
        unsigned char* hp = static_cast<unsigned char*>(std::malloc(inputs_end));
        unsigned char* dp = static_cast<unsigned char*>(std::malloc(inputs_end));
        CHECK(hp && dp);
        std::memset(hp, 0xEE, inputs_end);
        // the order: a permutation, longest first, equal lengths in input order
        const std::vector<int32_t> order = longest_first(offsets.data(), P);
        std::vector<int> seen(P, 0);
        for (int p = 0; p < P; ++p) {
            CHECK(order[p] >= 0 && order[p] < P && !seen[order[p]]++);
            if (p == 0) continue;
            const int before = offsets[order[p - 1] + 1] - offsets[order[p - 1]];
            const int here = offsets[order[p] + 1] - offsets[order[p]];
            CHECK(before > here || (before == here && order[p - 1] < order[p]));
        }
        std::vector<const unsigned char*> tab(located, located + T);
        stage_gate_table(g, L, n_index, order.data(), &tab, hp, dp);
        // every staged array is its source
        CHECK(std::memcmp(hp + L.offsets, offsets.data(), 4*(size_t(P) + 1)) == 0);
        CHECK(std::memcmp(hp + L.index, index.data(), 4*n_index) == 0);
        CHECK(std::memcmp(hp + L.order, order.data(), 4*size_t(P)) == 0);
        CHECK(std::memcmp(hp + L.tau, tau.data(), 8*size_t(T)) == 0);
        CHECK(std::memcmp(hp + L.omega, omega.data(), 8*size_t(W)) == 0);
        CHECK(std::memcmp(hp + L.basis, basis.data(), 16*size_t(N)*dd) == 0);
        CHECK(std::memcmp(hp + L.U, U.data(), 16*size_t(T)*dd) == 0);
        CHECK(n_host == 0 || std::memcmp(hp + L.host, host_table.data(), row*size_t(n_host)) == 0);
        // the pointer table: a gate with a handle where it was located, the others in consecutive rows of the
        // device-side table region, in gate order
        const unsigned char* staged[12];
        std::memcpy(staged, hp + L.tab, 8*size_t(T));
        size_t next_row = 0;
        for (int k = 0; k < T; ++k) {
            CHECK(staged[k] == tab[k]);
            if (located[k])
                CHECK(staged[k] == located[k]);
            else
                CHECK(staged[k] == dp + L.host + row*next_row++);
        }
        CHECK(next_row == size_t(n_host));
        // what the pass adds behind the head is untouched
        for (size_t k = tail; k < inputs_end; ++k) CHECK(hp[k] == 0xEE);
        // the device view after the one copy of [0, inputs_end)
        std::memcpy(dp, hp, inputs_end);
        const GateTableDevice D(dp, L);
        CHECK(D.offsets[P] == offsets[P] && D.index[n_index - 1] == index.back() && D.order[P - 1] == order.back());
        CHECK(D.tau[T - 1] == tau.back() && D.omega[W - 1] == omega.back());
        CHECK(D.basis[size_t(N)*dd - 1].im == basis.back() && D.U[size_t(T)*dd - 1].im == U.back());
        CHECK(reinterpret_cast<const unsigned char*>(D.tab[T - 1]) == staged[T - 1]);
        std::free(hp);
        std::free(dp);
        // malformed tables are refused, with the texts of the entry points
        CHECK(verdict({0, 2, 3}, {0, 1, 0}, d, min_W, "index[1] = 1 outside [0, 1)"));
        CHECK(verdict({0, 2, 1}, {0, 0, 0}, d, min_W, "offsets not increasing at sequence 1 (2 -> 1)"));
        CHECK(verdict({1, 2, 3}, {0, 0, 0}, d, min_W, "offsets[0] = 1, expected 0"));
        CHECK(verdict({0, 2, 3}, {0, 0, 0}, d, min_W, nullptr));
    }
    std::printf("gate table: %d rounds ok\n", rounds);
    return 0;
}

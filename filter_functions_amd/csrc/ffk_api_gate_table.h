// ffk_api_gate_table.h -- what the passes over many gate sequences from ONE gate table share (ffk_api_resident.hip:
// ffk_concatenate_sequences_resident, ffk_sequence_correlation_infidelities[4], ffk_sequence_infidelities,
// ffk_sequence_processes, ffk_sequence_frequency_shifts): their sixteen leading arguments as one view, the checks on
// them, the head of their layouts, the order in which the device deals the sequences out, the staging of the table
// into the pinned block, the typed device pointers and the front launch.  Nothing here knows which pass calls it:
// spectra, further inputs, outputs and where the blocks come from stay in the entries.  Needs ffk_api_common.h only
// (no resident handle, no pool, no lease), so that a stand-alone program can drive it (tools/check_gate_table.hip).
#pragma once
#include "ffk_api_common.h"

namespace ffk_api {

// The leading arguments of every gate-table entry, as the caller passed them (include/ffk.h): T gates, each with a
// resident handle (and member slot) or -- no handle -- the next row of gate_table; P sequences in CSR form.
struct GateTable {
    ffk_resident* const* gates;
    const int32_t* slots;
    const double *gate_table, *gate_propagators, *tau;
    int T;
    const int32_t *offsets, *index;
    int P;
    const double* omega;
    int W;
    const double* basis;
    int hermitian_basis, d, A, N;
    size_t row_bytes() const { return 16*size_t(A)*N*W; }      // one gate's control matrix (A, N, W)
};

// Pointers, axes (W against the entry's minimum), the Hermitian basis and the CSR arrays; *n_index = offsets[P], which
// is read only after the axes are known to be sane.
inline int check_gate_table(const GateTable& g, int min_W, size_t* n_index) {
    FFK_REQUIRE(g.gates && g.slots && g.gate_propagators && g.tau && g.offsets && g.index && g.omega && g.basis,
                "NULL argument");
    FFK_REQUIRE(g.hermitian_basis != 0, "the batched rule needs a Hermitian basis");
    const bool axes_ok = g.T >= 1 && g.T <= (1 << 20) && g.P >= 1 && g.P <= (1 << 24) && g.W >= min_W;
    if (min_W >= 2)
        FFK_REQUIRE(axes_ok, "empty or oversized axis: T=%d P=%d W=%d (need W >= 2)", g.T, g.P, g.W);
    else
        FFK_REQUIRE(axes_ok, "empty or oversized axis: T=%d P=%d W=%d", g.T, g.P, g.W);
    FFK_REQUIRE(g.offsets[0] == 0, "offsets[0] = %d, expected 0", g.offsets[0]);
    for (int p = 0; p < g.P; ++p)
        FFK_REQUIRE(g.offsets[p + 1] > g.offsets[p], "offsets not increasing at sequence %d (%d -> %d)", p,
                    g.offsets[p], g.offsets[p + 1]);
    *n_index = size_t(g.offsets[g.P]);
    for (size_t k = 0; k < *n_index; ++k)
        FFK_REQUIRE(g.index[k] >= 0 && g.index[k] < g.T, "index[%zu] = %d outside [0, %d)", k, g.index[k], g.T);
    return FFK_OK;
}

// Byte offsets of the table's arrays: the first member of every pass layout, at the start of its one H2D copy.
// `order` holds P int32 -- the sequences in the order the pass's kernels deal them out.
struct GateTableLayout {
    size_t offsets, index, order, tau, omega, basis, U, tab, host;
};
// `put(bytes)`: the caller's bump over its layout (returns where the array starts)
template <typename Put>
GateTableLayout gate_table_layout(Put&& put, int T, int P, size_t n_index, int n_host, int d, int A, int N, int W) {
    GateTableLayout L;
    const size_t dd = size_t(d)*d;
    L.offsets = put(4*(size_t(P) + 1));
    L.index = put(4*n_index);
    L.order = put(4*size_t(P));
    L.tau = put(8*size_t(T));
    L.omega = put(8*size_t(W));
    L.basis = put(16*size_t(N)*dd);
    L.U = put(16*size_t(T)*dd);
    L.tab = put(8*size_t(T));
    L.host = put(16*size_t(A)*N*W*size_t(n_host));
    return L;
}

// the sequences sorted by length, longest first, equal lengths in input order (the stable order, written as a total
// one): the rule kernels deal them out in this order
inline std::vector<int32_t> longest_first(const int32_t* offsets, int P) {
    std::vector<int32_t> order(P);
    for (int p = 0; p < P; ++p) order[p] = p;
    std::sort(order.begin(), order.end(), [offsets](int32_t a, int32_t b) {
        const int32_t la = offsets[a + 1] - offsets[a], lb = offsets[b + 1] - offsets[b];
        return la != lb ? la > lb : a < b;
    });
    return order;
}

// Control matrices that no handle holds (NULL in `at`) lie in consecutive rows from `table` on: returns how many.
inline size_t place_host_rows(std::vector<const unsigned char*>* at, const unsigned char* table, size_t row_bytes) {
    size_t n = 0;
    for (const unsigned char*& p : *at)
        if (!p) p = table + row_bytes*n++;
    return n;
}

// The table into the pinned block `hp`, laid out for the device block `dp`: the CSR arrays, `order` (P), the small
// arrays, the gates without a handle (rows of g.gate_table) and the pointer table `tab` -- as located, NULL for those
// gates, whose rows are placed here.
inline void stage_gate_table(const GateTable& g, const GateTableLayout& L, size_t n_index, const int32_t* order,
                             std::vector<const unsigned char*>* tab, unsigned char* hp, const unsigned char* dp) {
    const size_t dd = size_t(g.d)*g.d;
    std::memcpy(hp + L.offsets, g.offsets, 4*(size_t(g.P) + 1));
    std::memcpy(hp + L.index, g.index, 4*n_index);
    std::memcpy(hp + L.order, order, 4*size_t(g.P));
    std::memcpy(hp + L.tau, g.tau, 8*size_t(g.T));
    std::memcpy(hp + L.omega, g.omega, 8*size_t(g.W));
    std::memcpy(hp + L.basis, g.basis, 16*size_t(g.N)*dd);
    std::memcpy(hp + L.U, g.gate_propagators, 16*size_t(g.T)*dd);
    const size_t n_host = place_host_rows(tab, dp + L.host, g.row_bytes());
    std::memcpy(hp + L.tab, tab->data(), 8*size_t(g.T));
    if (n_host) std::memcpy(hp + L.host, g.gate_table, g.row_bytes()*n_host);
}

// the table's arrays in the device block, typed as the launchers take them
struct GateTableDevice {
    const int32_t *offsets, *index, *order;
    const double *tau, *omega;
    const cplx *basis, *U;
    const cplx* const* tab;
    GateTableDevice(const unsigned char* dp, const GateTableLayout& L)
        : offsets(reinterpret_cast<const int32_t*>(dp + L.offsets)),
          index(reinterpret_cast<const int32_t*>(dp + L.index)),
          order(reinterpret_cast<const int32_t*>(dp + L.order)),
          tau(reinterpret_cast<const double*>(dp + L.tau)),
          omega(reinterpret_cast<const double*>(dp + L.omega)),
          basis(reinterpret_cast<const cplx*>(dp + L.basis)),
          U(reinterpret_cast<const cplx*>(dp + L.U)),
          tab(reinterpret_cast<const cplx* const*>(dp + L.tab)) {}
};

// the front launch of the table's dimension: the gates' phases (T, W) and Liouville representations (T, N, N), every
// sequence's total propagator (P, d, d)
inline hipError_t launch_gate_table_front(const GateTable& g, const GateTableDevice& D, cplx* phases, double* Lpulse,
                                          cplx* Qtot, hipStream_t s) {
    return (g.d == 2 ? ffk::launch_sequences_front : ffk::launch_sequences4_front)(
        D.U, D.tau, D.omega, g.T, g.W, D.offsets, D.index, g.P, D.basis, phases, Lpulse, Qtot, s);
}

}  // namespace ffk_api

// prep.hip -- omega-independent operands of the control-matrix accumulation, one wavefront per
// segment, plus the two "cache_intermediates" side products that are cheap element-wise maps.
//
// Reference arithmetic restated here:
//   T_g = V_g^dag Q_g                         (_propagate_eigenvectors, numeric.py:93-95, :577)
//   Bbar_a^(g) = s_a(g) V_g^dag B_a V_g       (_transform_hamiltonian, numeric.py:98-141)
//   dE^(g)[m,n] = D_m - D_n                   (np.subtract.outer, numeric.py:155)
// packed per segment as ops[g] = (T_g, Bbar_0^(g), ..., Bbar_{A-1}^(g)), the block of operands the
// accumulate kernel stages in LDS for segment g.
#include "ffk_internal.h"
#include "ffk_mfma_util.h"

namespace ffk {
namespace {

// The prologue of one segment by one wavefront, in two halves around the propagator Q_g:
//   prologue_front  everything that needs only the eigensystem: the table row (dE, sin/cos of b, the threshold) and
//                   Bbar_a = s V^dag B_a V of every operator;
//   prologue_back   what needs Q_g: T = V^dag Q, Tc, the T block of ops, and (d = 4) the fold of the accumulate
//                   kernel's operand W_a.
// What either half reads from memory is asked for at the top of the block, in one go and before the first wait
// (prologue_front_loads; the fused kernel below adds the chunk totals and its two propagators): one trip to memory
// instead of one per array.  The matrices go straight into LDS (lds_dma16: no register holds them while they are on
// their way -- the kernel runs beside another pass's accumulate blocks on 56 registers); a lane's scalars wait in
// registers.  The products and sums are the ones the one-piece prologue made, operand by operand: the same bits.
// d <= 8 (one entry of a d x d matrix per lane); larger d reads everything where it is used, as ever.
template <int D>
constexpr bool kOneEntryPerLane = D*D <= 64;
// Operators per pass of the 64 lanes (d <= 8: lane = (operator q of the pass, entry e), like the prefix tree's
// products; larger d: one operator, several entries per lane) -- at d = 4 the B and the coefficients of up to four
// operators come in ONE trip to memory, and the two products take one pair of barriers for all of them.
template <int D>
constexpr int kOpsPerPass = D*D <= 64 ? 64/(D*D) : 1;

// The fold of the d = 4 operand needs every Bbar_a again once T is known.  Up to one pass of operators (four) they
// wait in LDS, in the place of the B they were made from (Bl is free once B V is out); with more operators each lane
// reads its entries back from `ops`.  No array of their own: with 2 KiB more the block was 10 KiB of LDS, and the
// kernel's launches beside another pass's accumulate blocks took 12.7 us on average instead of 9.9 (up to 48: blocks
// waiting for an accumulate block to retire), although a launch on its own was 2 us shorter.
template <int D>
__device__ __forceinline__ int bbar_kept(int A) { return A <= kOpsPerPass<D> ? A : 0; }

template <int D>
struct PrologueLoads {
    double em, en;                                  // D_m, D_n of the lane's entry (m, n)
    double dtg, tg;
    double s;                                       // coefficient of the lane's operator of the first pass
};

// B of the operators [a0, a0 + kOpsPerPass) into Bl by LDS-DMA, the lane's operator's coefficient for segment g
// into s (kOneEntryPerLane; lanes past the last operator: a clamped index, value unused).  The caller waits
// (lds_dma_wait) and synchronises before Bl is read.
template <int D>
__device__ __forceinline__ void operator_pass_loads(double& s, cplx (*Bl)[D][D], int a0, int lane,
                                                    const cplx* __restrict__ n_opers,
                                                    const double* __restrict__ n_coeffs, int G, int A, int g) {
    constexpr int DD = D*D, PER = kOpsPerPass<D>;
    if (lane < min(PER, A - a0)*DD) lds_dma16(n_opers + static_cast<size_t>(a0)*DD + lane, &Bl[0][0][0]);
    const int a = min(a0 + min(lane / DD, PER - 1), A - 1);
    s = n_coeffs ? n_coeffs[static_cast<size_t>(a)*G + g] : 1.0;   // NULL: unit
}

template <int D>
__device__ __forceinline__ void prologue_front_loads(PrologueLoads<D>& ld, cplx (*Bl)[D][D], int g, int lane,
                                                     const double* __restrict__ eigvals,
                                                     const double* __restrict__ dt, const double* __restrict__ t,
                                                     const cplx* __restrict__ n_opers,
                                                     const double* __restrict__ n_coeffs, int G, int A,
                                                     bool with_noise_ops) {
    const int e = min(lane, D*D - 1);                 // (lanes past the matrix: a clamped index, value unused)
    ld.em = eigvals[static_cast<size_t>(g)*D + e / D];
    ld.en = eigvals[static_cast<size_t>(g)*D + e % D];
    ld.dtg = dt[g];
    ld.tg = t[g];
    ld.s = 1.0;
    if constexpr (kOneEntryPerLane<D>) {
        if (with_noise_ops && A > 0) operator_pass_loads<D>(ld.s, Bl, 0, lane, n_opers, n_coeffs, G, A, g);
    }
}

// V and, for d <= 8, Bl (the first pass's operators) and ld are in place (prologue_front_loads, waited for and
// synchronised).  Bl, BV: [kOpsPerPass][D][D]; Bbar of the operators below bbar_kept stays in Bl.  Returns e^{i b_mn}
// of this lane's entry (d = 4: one entry per lane < 16).
template <int D>
__device__ __forceinline__ cplx prologue_front(const cplx (*V)[D], cplx (*Bl)[D][D], cplx (*BV)[D][D],
                                               int g, int lane, const PrologueLoads<D>& ld,
                                               const double* __restrict__ eigvals, const cplx* __restrict__ n_opers,
                                               const double* __restrict__ n_coeffs, int G, int A,
                                               double* __restrict__ segtab, cplx* __restrict__ ops,
                                               cplx* __restrict__ n_opers_transformed, bool with_noise_ops,
                                               bool fold) {
    constexpr int S = seg_stride(D);
    constexpr int DD = D*D, PER = kOpsPerPass<D>;
    double* st = segtab + static_cast<size_t>(g)*S;
    if (lane == 0) {
        st[0] = ld.dtg;
        st[1] = ld.tg;
    }
    cplx eb = {1.0, 0.0};                              // e^{i b_mn} of this lane's entry
    for (int e = lane; e < DD; e += 64) {
        double dE;
        if constexpr (kOneEntryPerLane<D>) dE = ld.em - ld.en;
        else dE = eigvals[static_cast<size_t>(g)*D + e / D] - eigvals[static_cast<size_t>(g)*D + e % D];
        double sb, cb;
        sincos_pi(0.5*(dE*ld.dtg), &sb, &cb);
        st[seg_rec(e)] = dE;
        st[seg_rec(e) + 1] = sb;
        st[seg_rec(e) + 2] = cb;
        st[seg_rec(e) + 3] = 0.0;
        eb = {cb, sb};
    }
    // [2]: the near-resonance threshold 2^-4/dt_g, phased_frequency()'s own expression (the d = 4 producers read
    // it with the head record instead of forming it per tile and lane, ctrl_pq.hip)
    if (lane == 0) st[2] = ld.dtg > 0.0 ? 0.0625*rcp(ld.dtg) : __builtin_huge_val();
    if (lane == 1) st[3] = 0.0;
    for (int e = 4 + 4*DD + lane; e < S; e += 64) st[e] = 0.0;

    if (!with_noise_ops) return eb;     // (large d: noise_ops_kernel, one block per operator)
    // Bbar = s V^dag BV, entry e of operator a (q: its place in the pass)
    auto bbar_entry = [&](int a, int q, int e, double s) {
        const int m = e / D, n = e % D;
        cplx acc = {0.0, 0.0};
#pragma unroll
        for (int k = 0; k < D; ++k) cmac_conj(acc, V[k][m], BV[q][k][n]);
        acc.re *= s;
        acc.im *= s;
        ops[(static_cast<size_t>(g)*(1 + A) + 1 + a)*DD + e] = acc;
        if (n_opers_transformed)
            n_opers_transformed[(static_cast<size_t>(a)*G + g)*DD + e] = acc;
        if (fold && a < bbar_kept<D>(A)) Bl[a][m][n] = acc;     // (one pass: a = q, and B V of the pass is out)
    };
    double s = ld.s;
    for (int a0 = 0; a0 < A; a0 += PER) {
        if constexpr (kOneEntryPerLane<D>) {
            if (a0 > 0) {
                // (every lane has its products of the pass before out of Bl: the barrier that ended it)
                operator_pass_loads<D>(s, Bl, a0, lane, n_opers, n_coeffs, G, A, g);
                lds_dma_wait();
                __syncthreads();
            }
            const int q = lane / DD, e = lane % DD, i = e / D, n = e % D;
            const bool act = q < PER && a0 + q < A;
            if (act) {                                  // BV = B V
                cplx acc = {0.0, 0.0};
#pragma unroll
                for (int k = 0; k < D; ++k) cmac(acc, Bl[q][i][k], V[k][n]);
                BV[q][i][n] = acc;
            }
            __syncthreads();
            if (act) bbar_entry(a0 + q, q, e, s);
            __syncthreads();
        } else {
            const cplx* B = n_opers + static_cast<size_t>(a0)*DD;
            s = n_coeffs ? n_coeffs[static_cast<size_t>(a0)*G + g] : 1.0;   // NULL: unit
            for (int e = lane; e < DD; e += 64) {       // BV = B V
                const int i = e / D, n = e % D;
                cplx acc = {0.0, 0.0};
#pragma unroll
                for (int k = 0; k < D; ++k) cmac(acc, B[i*D + k], V[k][n]);
                BV[0][i][n] = acc;
            }
            __syncthreads();
            for (int e = lane; e < DD; e += 64) bbar_entry(a0, 0, e, s);
            __syncthreads();
        }
    }
    return eb;
}

template <int D>
__device__ __forceinline__ void prologue_back(const cplx (*V)[D], cplx (*Q)[D], cplx (*T)[D], cplx (*BV)[D][D],
                                              const cplx (*Bl)[D][D], cplx eb, int g, int lane, int A,
                                              cplx* __restrict__ Tc, cplx* __restrict__ ops,
                                              cplx* __restrict__ eigvecs_propagated, bool fold,
                                              cplx* __restrict__ wfold) {
    // T = V^dag Q
    for (int e = lane; e < D*D; e += 64) {
        const int m = e / D, j = e % D;
        cplx acc = {0.0, 0.0};
#pragma unroll
        for (int k = 0; k < D; ++k) cmac_conj(acc, V[k][m], Q[k][j]);
        T[m][j] = acc;
        Tc[static_cast<size_t>(g)*D*D + e] = {acc.re, -acc.im};
        ops[static_cast<size_t>(g)*(1 + A)*D*D + e] = acc;
        // eigvecs_propagated = Q^dag V = T^dag:  [i][j] = conj(T[j][i])
        if (eigvecs_propagated)
            eigvecs_propagated[static_cast<size_t>(g)*D*D + j*D + m] = {acc.re, -acc.im};
    }
    __syncthreads();
    // d = 4 with a buffer for it (ffk_internal.h wfold): W_a[n][m][j] = Bbar_a[m][n] e^{i b_mn} T[n][j], the
    // operand the accumulate kernel's tiles hold, folded here once per segment.  Q is free by now: it keeps e^{ib}.
    if constexpr (D == 4) {
        if (!fold) return;
        if (lane < D*D) Q[lane / D][lane % D] = eb;
        __syncthreads();
        // lane = (m, n, j), the accumulate kernel's order of products: (e^{ib} T) first, then Bbar times that
        const int m = lane >> 4, n = (lane >> 2) & 3, j = lane & 3;
        const cplx et = cmul(Q[m][n], T[n][j]);
        for (int a = 0; a < A; ++a) {
            const bool kept = a < bbar_kept<D>(A);
            const cplx* bbar = &Bl[kept ? a : 0][m][n];
            if (!kept) {
                // (each lane reads back the entry of Bbar_a that it wrote itself: prologue_front's lane (q, e))
                if (lane / (D*D) == a % kOpsPerPass<D>) {
                    const int e = lane % (D*D);
                    BV[0][e / D][e % D] = ops[(static_cast<size_t>(g)*(1 + A) + 1 + a)*D*D + e];
                }
                __syncthreads();
                bbar = &BV[0][m][n];
            }
            const cplx w = cmul(*bbar, et);
            wfold[(static_cast<size_t>(g)*A + a)*64 + n*16 + m*4 + j] = w;
            if (!kept) __syncthreads();
        }
    }
}

// Prologue arithmetic for one segment by one wavefront; V (eigenvectors) and Q (propagator
// before the segment) already sit in LDS.
template <int D>
__device__ void prologue_segment(const cplx (*V)[D], cplx (*Q)[D], cplx (*T)[D],
                                 int g, int lane, const double* __restrict__ eigvals,
                                 const cplx* __restrict__ n_opers,
                                 const double* __restrict__ n_coeffs,
                                 const double* __restrict__ dt, const double* __restrict__ t, int G,
                                 int A, double* __restrict__ segtab, cplx* __restrict__ Tc,
                                 cplx* __restrict__ ops, cplx* __restrict__ n_opers_transformed,
                                 cplx* __restrict__ eigvecs_propagated, bool with_noise_ops = true,
                                 cplx* __restrict__ wfold = nullptr) {
    __shared__ __attribute__((aligned(16))) cplx Bl[kOpsPerPass<D>][D][D];
    __shared__ cplx BV[kOpsPerPass<D>][D][D];
    const bool fold = D == 4 && wfold != nullptr && with_noise_ops;
    PrologueLoads<D> ld;
    prologue_front_loads<D>(ld, Bl, g, lane, eigvals, dt, t, n_opers, n_coeffs, G, A, with_noise_ops);
    if constexpr (kOneEntryPerLane<D>) {
        lds_dma_wait();
        __syncthreads();
    }
    const cplx eb = prologue_front<D>(V, Bl, BV, g, lane, ld, eigvals, n_opers, n_coeffs, G, A, segtab, ops,
                                      n_opers_transformed, with_noise_ops, fold);
    prologue_back<D>(V, Q, T, BV, Bl, eb, g, lane, A, Tc, ops, eigvecs_propagated, fold, wfold);
}

template <int D>
__global__ __launch_bounds__(64) void prologue_kernel(
    const double* __restrict__ eigvals, const cplx* __restrict__ eigvecs,
    const cplx* __restrict__ propagators, const cplx* __restrict__ n_opers,
    const double* __restrict__ n_coeffs, const double* __restrict__ dt,
    const double* __restrict__ t, int G, int A, double* __restrict__ segtab,
    cplx* __restrict__ Tc, cplx* __restrict__ ops, cplx* __restrict__ n_opers_transformed,
    cplx* __restrict__ eigvecs_propagated, bool with_noise_ops, cplx* __restrict__ wfold) {
    __shared__ cplx V[D][D];
    __shared__ cplx Q[D][D];
    __shared__ cplx T[D][D];
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    for (int e = lane; e < D*D; e += 64) {
        V[e / D][e % D] = eigvecs[static_cast<size_t>(g)*D*D + e];
        Q[e / D][e % D] = propagators[static_cast<size_t>(g)*D*D + e];
    }
    __syncthreads();
    prologue_segment<D>(V, Q, T, g, lane, eigvals, n_opers, n_coeffs, dt, t, G, A, segtab, Tc,
                        ops, n_opers_transformed, eigvecs_propagated, with_noise_ops, wfold);
}

// Batched form of prologue_kernel: block (segment, pulse), every array pulse-major.
template <int D>
__global__ __launch_bounds__(64) void prologue_pulses_kernel(
    const double* __restrict__ eigvals, const cplx* __restrict__ eigvecs,
    const cplx* __restrict__ propagators, const cplx* __restrict__ n_opers,
    const double* __restrict__ n_coeffs, const double* __restrict__ dt,
    const double* __restrict__ t, int G, int A, double* __restrict__ segtab,
    cplx* __restrict__ Tc, cplx* __restrict__ ops, cplx* __restrict__ n_opers_transformed) {
    __shared__ cplx V[D][D];
    __shared__ cplx Q[D][D];
    __shared__ cplx T[D][D];
    constexpr size_t DD = D*D;
    const size_t p = blockIdx.y;
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    const cplx* Vp = eigvecs + p*G*DD;
    const cplx* Qp = propagators + p*(G + 1)*DD;
    for (int e = lane; e < D*D; e += 64) {
        V[e / D][e % D] = Vp[static_cast<size_t>(g)*DD + e];
        Q[e / D][e % D] = Qp[static_cast<size_t>(g)*DD + e];
    }
    __syncthreads();
    prologue_segment<D>(V, Q, T, g, lane, eigvals + p*G*D, n_opers + p*A*DD, n_coeffs + p*A*G, dt + p*G,
                        t + p*(G + 1), G, A, segtab + p*G*seg_stride(D), Tc + p*G*DD, ops + p*G*(1 + A)*DD,
                        n_opers_transformed + p*A*G*DD, nullptr, true, nullptr);
}

// Bbar_a^(g) = s_a(t_g) V_g^dag B_a V_g for one (segment, noise operator) per block.  For large d the
// two d^3 products per operator dominate the prologue (d = 16, 18 operators: 172 us for 13 blocks
// of one wavefront each); spread over G x A blocks they take as long as one operator.
template <int D>
__global__ __launch_bounds__(64) void noise_ops_kernel(const cplx* __restrict__ eigvecs,
                                                       const cplx* __restrict__ n_opers,
                                                       const double* __restrict__ n_coeffs, int G,
                                                       int A, cplx* __restrict__ ops,
                                                       cplx* __restrict__ n_opers_transformed) {
    __shared__ cplx V[D][D];
    __shared__ cplx BV[D][D];
    __builtin_amdgcn_s_setprio(3);     // see ffk_internal.h FFK_SMALL_KERNEL_PRIORITY
    const int g = blockIdx.x, a = blockIdx.y, lane = threadIdx.x;
    for (int e = lane; e < D*D; e += 64) V[e / D][e % D] = eigvecs[static_cast<size_t>(g)*D*D + e];
    __syncthreads();
    const cplx* B = n_opers + static_cast<size_t>(a)*D*D;
    const double s = n_coeffs ? n_coeffs[static_cast<size_t>(a)*G + g] : 1.0;   // NULL: unit
    for (int e = lane; e < D*D; e += 64) {
        const int i = e / D, n = e % D;
        cplx acc = {0.0, 0.0};
#pragma unroll
        for (int k = 0; k < D; ++k) cmac(acc, B[i*D + k], V[k][n]);
        BV[i][n] = acc;
    }
    __syncthreads();
    for (int e = lane; e < D*D; e += 64) {
        const int m = e / D, n = e % D;
        cplx acc = {0.0, 0.0};
#pragma unroll
        for (int k = 0; k < D; ++k) cmac_conj(acc, V[k][m], BV[k][n]);
        acc.re *= s;
        acc.im *= s;
        ops[(static_cast<size_t>(g)*(1 + A) + 1 + a)*D*D + e] = acc;
        if (n_opers_transformed)
            n_opers_transformed[(static_cast<size_t>(a)*G + g)*D*D + e] = acc;
    }
}

// noise operators by their own launch from this dimension on (and only with several of them)
constexpr int kNoiseOpsKernelMinD = 12;
inline bool split_noise_ops(int d, int A) { return d >= kNoiseOpsKernelMinD && A >= 2 && A <= 65535; }

// Fused scan fix-up + prologue, one wavefront per segment:
//   E_c = T_{c-1} ... T_0 rebuilt serially from the chunk totals (<= 63 small products, done
//   redundantly by every block instead of a third launch), Q[g+1] = Qloc[g+1] E_c written out,
//   Q[g] = Qloc[g] E_c kept in LDS and fed straight into the prologue.
// (segment g of one pulse; the kernels below pick g and the pulse)
template <int D>
__device__ __forceinline__ void apply_prologue_segment(
    const cplx* __restrict__ Qloc, const cplx* __restrict__ totals, int G, int L,
    cplx* __restrict__ Qout, const double* __restrict__ eigvals, const cplx* __restrict__ eigvecs,
    const cplx* __restrict__ n_opers, const double* __restrict__ n_coeffs,
    const double* __restrict__ dt, const double* __restrict__ t, int A,
    double* __restrict__ segtab, cplx* __restrict__ Tc, cplx* __restrict__ ops,
    bool with_noise_ops, cplx* __restrict__ wfold, const int g) {
    __builtin_amdgcn_s_setprio(3);     // see ffk_internal.h FFK_SMALL_KERNEL_PRIORITY
    __shared__ cplx E[2][D][D];
    __shared__ __attribute__((aligned(16))) cplx M[D][D];      // Qloc[g+1]
    __shared__ __attribute__((aligned(16))) cplx Mg[D][D];     // Qloc[g]
    __shared__ __attribute__((aligned(16))) cplx V[D][D];
    __shared__ __attribute__((aligned(16))) cplx Bl[kOpsPerPass<D>][D][D];
    __shared__ cplx Q[D][D];
    __shared__ cplx T[D][D];
    __shared__ cplx BV[kOpsPerPass<D>][D][D];
    constexpr int kBatch = 16;
    constexpr bool kTree = D <= 8;                 // a whole matrix fits one pass of the 64 lanes
    // the chunk totals: for the tree as many as the launch has chunks (dynamic LDS: 4 KiB at config 2;
    // a static array for the 64 chunks use_fused_front allows took 16 KiB, and a kernel with more
    // than 8 KiB of static LDS is not placed beside an accumulate block of another pass,
    // tools/corun.hip), else one batch
    extern __shared__ __attribute__((aligned(16))) unsigned char tot_raw[];
    cplx (*tot)[D][D] = reinterpret_cast<cplx (*)[D][D]>(tot_raw);
    const int lane = threadIdx.x;
    const int c = g / L;
    const bool prologue = segtab != nullptr;       // (nullptr: the scan fix-up alone)
    const bool fold = D == 4 && wfold != nullptr && with_noise_ops;
    // Every load of the block is issued here, before the first wait (d <= 8; see prologue_front): the matrices by
    // LDS-DMA -- eigenvectors, the first operators, the two local propagators, the chunk totals (lanes past an array's
    // end copy nothing) --, the lane's scalars into registers.
    constexpr int DD = D*D;
    PrologueLoads<D> ld;
    if constexpr (kOneEntryPerLane<D>) {
        if (prologue) {
            prologue_front_loads<D>(ld, Bl, g, lane, eigvals, dt, t, n_opers, n_coeffs, G, A, with_noise_ops);
            if (lane < DD) lds_dma16(eigvecs + static_cast<size_t>(g)*DD + lane, &V[0][0]);
        }
        if (lane < DD) {
            lds_dma16(Qloc + static_cast<size_t>(g + 1)*DD + lane, &M[0][0]);
            // (unused where g opens a chunk: Q_g is the prefix itself)
            lds_dma16(Qloc + static_cast<size_t>(g)*DD + lane, &Mg[0][0]);
        }
        for (int e0 = 0; e0 < c*DD; e0 += 64)
            if (e0 + lane < c*DD) lds_dma16(totals + e0 + lane, &tot[0][0][0] + e0);
        lds_dma_wait();
    } else {
        if (prologue) {
            prologue_front_loads<D>(ld, Bl, g, lane, eigvals, dt, t, n_opers, n_coeffs, G, A, with_noise_ops);
            for (int e = lane; e < DD; e += 64) V[e / D][e % D] = eigvecs[static_cast<size_t>(g)*DD + e];
        }
        for (int e = lane; e < DD; e += 64) {
            M[e / D][e % D] = Qloc[static_cast<size_t>(g + 1)*DD + e];
            Mg[e / D][e % D] = Qloc[static_cast<size_t>(g)*DD + e];
        }
    }
    for (int e = lane; e < DD; e += 64) E[0][e / D][e % D] = {(e / D == e % D) ? 1.0 : 0.0, 0.0};
    __syncthreads();
    cplx eb = {1.0, 0.0};
    if (prologue)
        eb = prologue_front<D>(V, Bl, BV, g, lane, ld, eigvals, n_opers, n_coeffs, G, A, segtab, ops, nullptr,
                               with_noise_ops, fold);
    int b = 0;
    if constexpr (kTree) {
        // exclusive prefix E_c = T_{c-1} ... T_0 of the chunk totals as an ordered pairwise tree
        // (newer factor on the left), several products per pass: ceil(log2 c) dependent levels
        // instead of c - 1 dependent products.  In place: pass j writes slot j after reading slots
        // 2j and 2j+1, which no later pass of the level reads.
        constexpr int PER = 64/DD;
        int n = c;                                  // (the totals: in `tot` since the top of the block)
        while (n > 1) {
            const int pairs = n >> 1;
            for (int j0 = 0; j0 < pairs; j0 += PER) {
                const int jj = j0 + lane/DD, e = lane % DD, i = e / D, k = e % D;
                const bool act = lane < PER*DD && jj < pairs;
                cplx acc = {0.0, 0.0};
                if (act) {
#pragma unroll
                    for (int x = 0; x < D; ++x) cmac(acc, tot[2*jj + 1][i][x], tot[2*jj][x][k]);
                }
                __syncthreads();
                if (act) tot[jj][i][k] = acc;
                __syncthreads();
            }
            if (n & 1) {                            // the newest factor moves up unpaired
                // (two doubles read by every lane from a clamped index: as a struct copy the value was kept in SCRATCH
                // memory across the barrier -- a trip to memory per odd level of the tree, in every pass; round 6)
                const cplx* from = &tot[n - 1][0][0] + (lane < DD ? lane : 0);
                const double carry_re = from->re, carry_im = from->im;      // (two doubles, not a struct copy)
                __syncthreads();
                if (lane < DD) (&tot[pairs][0][0])[lane] = {carry_re, carry_im};
                __syncthreads();
            }
            n = pairs + (n & 1);
        }
        if (c > 0) {
            for (int e = lane; e < DD; e += 64) E[0][e / D][e % D] = tot[0][e / D][e % D];
            __syncthreads();
        }
    } else {
    // exclusive prefix of the chunk totals; the totals are staged in batches of independent loads
    // (one dependent global load per step cost ~0.5 us each)
    for (int kb = 0; kb < c; kb += kBatch) {
        const int nb = min(kBatch, c - kb);
        __syncthreads();
        for (int e = lane; e < nb*D*D; e += 64)
            (&tot[0][0][0])[e] = totals[static_cast<size_t>(kb)*D*D + e];
        __syncthreads();
        for (int k = 0; k < nb; ++k) {
            for (int e = lane; e < D*D; e += 64) {
                const int i = e / D, j = e % D;
                cplx acc = {0.0, 0.0};
#pragma unroll
                for (int x = 0; x < D; ++x) cmac(acc, tot[k][i][x], E[b][x][j]);
                E[b ^ 1][i][j] = acc;
            }
            __syncthreads();
            b ^= 1;
        }
    }
    }
    // Q[g] (into LDS) and Q[g+1] (to memory)
    if (g == 0)
        for (int e = lane; e < D*D; e += 64) Qout[e] = {(e / D == e % D) ? 1.0 : 0.0, 0.0};
    __syncthreads();
    for (int e = lane; e < D*D; e += 64) {
        const int i = e / D, j = e % D;
        cplx acc = {0.0, 0.0};
#pragma unroll
        for (int x = 0; x < D; ++x) cmac(acc, M[i][x], E[b][x][j]);
        Qout[static_cast<size_t>(g + 1)*D*D + e] = acc;
    }
    if (!prologue) return;
    if (g % L == 0) {
        for (int e = lane; e < D*D; e += 64) Q[e / D][e % D] = E[b][e / D][e % D];
    } else {
        for (int e = lane; e < D*D; e += 64) {
            const int i = e / D, j = e % D;
            cplx acc = {0.0, 0.0};
#pragma unroll
            for (int x = 0; x < D; ++x) cmac(acc, Mg[i][x], E[b][x][j]);
            Q[i][j] = acc;
        }
    }
    __syncthreads();
    prologue_back<D>(V, Q, T, BV, Bl, eb, g, lane, A, Tc, ops, nullptr, fold, wfold);
}

template <int D>
__global__ __launch_bounds__(64) void apply_prologue_kernel(
    const cplx* __restrict__ Qloc, const cplx* __restrict__ totals, int G, int L,
    cplx* __restrict__ Qout, const double* __restrict__ eigvals, const cplx* __restrict__ eigvecs,
    const cplx* __restrict__ n_opers, const double* __restrict__ n_coeffs,
    const double* __restrict__ dt, const double* __restrict__ t, int A,
    double* __restrict__ segtab, cplx* __restrict__ Tc, cplx* __restrict__ ops,
    const cplx* __restrict__ basis, int* __restrict__ nnz, int* __restrict__ rows,
    cplx* __restrict__ vals, bool with_noise_ops, cplx* __restrict__ wfold) {
    // extra blocks (launch_apply_prologue_compact): basis compaction
    if (static_cast<int>(blockIdx.x) >= G) {
        basis_compact_one(basis, D, static_cast<int>(blockIdx.x) - G, threadIdx.x, nnz, rows, vals);
        return;
    }
    apply_prologue_segment<D>(Qloc, totals, G, L, Qout, eigvals, eigvecs, n_opers, n_coeffs, dt, t, A, segtab, Tc,
                              ops, with_noise_ops, wfold, blockIdx.x);
}

// Batched form: block (segment, pulse) over P pulses of G segments, every array pulse-major (t pulse-local,
// (P, G+1)); each block rebuilds the exclusive chunk prefix from its own pulse's totals.  The basis is compacted
// once per pass, by the extra blocks of pulse 0.  The noise operators always ride in this kernel (no split).
template <int D>
__global__ __launch_bounds__(64) void apply_prologue_pulses_kernel(
    const cplx* __restrict__ Qloc, const cplx* __restrict__ totals, int G, int L, int nchunks,
    cplx* __restrict__ Qout, const double* __restrict__ eigvals, const cplx* __restrict__ eigvecs,
    const cplx* __restrict__ n_opers, const double* __restrict__ n_coeffs,
    const double* __restrict__ dt, const double* __restrict__ t, int A,
    double* __restrict__ segtab, cplx* __restrict__ Tc, cplx* __restrict__ ops,
    const cplx* __restrict__ basis, int* __restrict__ nnz, int* __restrict__ rows,
    cplx* __restrict__ vals, cplx* __restrict__ wfold) {
    const size_t p = blockIdx.y;
    if (static_cast<int>(blockIdx.x) >= G) {
        if (p == 0) basis_compact_one(basis, D, static_cast<int>(blockIdx.x) - G, threadIdx.x, nnz, rows, vals);
        return;
    }
    constexpr size_t DD = D*D;
    apply_prologue_segment<D>(Qloc + p*(G + 1)*DD, totals + p*nchunks*DD, G, L, Qout + p*(G + 1)*DD,
                              eigvals + p*G*D, eigvecs + p*G*DD, n_opers + p*A*DD, n_coeffs + p*A*G, dt + p*G,
                              t + p*(G + 1), A, segtab + p*G*seg_stride(D), Tc + p*G*DD, ops + p*G*(1 + A)*DD,
                              true, wfold ? wfold + p*G*A*64 : nullptr, blockIdx.x);
}

// out[g,k] = T_g C_k T_g^dag with T_g = conj(Tc[g])   (= (Q^dag V)^dag C_k (Q^dag V))
template <int D>
__global__ __launch_bounds__(64) void basis_transformed_kernel(const cplx* __restrict__ Tc,
                                                               const cplx* __restrict__ basis,
                                                               int N, cplx* __restrict__ out) {
    __shared__ cplx T[D][D];
    __shared__ cplx C[D][D];
    __shared__ cplx TC[D][D];
    const int g = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;   // g on x: G may exceed 65535
    for (int e = lane; e < D*D; e += 64) {
        const cplx v = Tc[static_cast<size_t>(g)*D*D + e];
        T[e / D][e % D] = {v.re, -v.im};
        C[e / D][e % D] = basis[static_cast<size_t>(k)*D*D + e];
    }
    __syncthreads();
    for (int e = lane; e < D*D; e += 64) {
        const int i = e / D, j = e % D;
        cplx acc = {0.0, 0.0};
#pragma unroll
        for (int a = 0; a < D; ++a) cmac(acc, T[i][a], C[a][j]);
        TC[i][j] = acc;
    }
    __syncthreads();
    for (int e = lane; e < D*D; e += 64) {
        const int i = e / D, j = e % D;
        cplx acc = {0.0, 0.0};
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const cplx tj = T[j][a];  // (T^dag)[a][j] = conj(T[j][a])
            cmac_conj(acc, tj, TC[i][a]);
        }
        out[(static_cast<size_t>(g)*N + k)*D*D + e] = acc;
    }
}

// phase_factors[g,w] = exp(i w t_g); integral[g,w,m,n] per numeric.py:144-167
__global__ void phase_integral_kernel(const double* __restrict__ omega, int W,
                                      const double* __restrict__ segtab, int d, int S,
                                      cplx* __restrict__ phase_factors,
                                      cplx* __restrict__ integral) {
    const int g = blockIdx.x;   // segments on x: G may exceed 65535
    const int w = blockIdx.y*blockDim.x + threadIdx.x;
    if (w >= W) return;
    const double* st = segtab + static_cast<size_t>(g)*S;
    const double om = omega[w];
    if (phase_factors) phase_factors[static_cast<size_t>(g)*W + w] = cexp(om*st[1]);
    if (integral) {
        cplx* out = integral + (static_cast<size_t>(g)*W + w)*d*d;
        for (int e = 0; e < d*d; ++e) out[e] = first_order_integral(om, st[seg_rec(e)], st[0]);
    }
}

}  // namespace

// d = 8: W'_a[m][n][i] = Bbar_a[m][n] e^{i b_mn} conj(T[m][i]), the frequency-independent A operand of the accumulate
// kernel's first product (ctrl_pcr.hip), once per (segment, operator) instead of once per 64-frequency block: the
// kernel's producers then copy it into their tiles by LDS-DMA.  Thread l <-> (m, n) = (l >> 3, l & 7); the products,
// their order and the layout [(s, ng, ig)][consumer lane] are those of the producers' own fold (same bits).
__global__ __launch_bounds__(64) void fold_w8_kernel(const double* __restrict__ segtab, const cplx* __restrict__ ops,
                                                     int A, cplx* __restrict__ wfold) {
    constexpr int D = 8, DD = 64, S = seg_stride(8);
    const int g = blockIdx.x, a = blockIdx.y, lane = threadIdx.x;
    const cplx* src = ops + static_cast<size_t>(g)*(1 + A)*DD;
    const double* r = segtab + static_cast<size_t>(g)*S + seg_rec(lane);
    const cplx x = src[static_cast<size_t>(1 + a)*DD + lane];
    const double sb = r[1], cb = r[2];
    const int m = lane >> 3, n = lane & 7;
    const int base = ((m >> 2)*2 + (n >> 2))*2*64 + 4*(n & 3) + 16*(m & 3);
    const cplx bt = cmul(x, cplx{cb, sb});
    cplx* out = wfold + (static_cast<size_t>(g)*A + a)*512;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const cplx t = src[m*D + i];
        out[base + (i >> 2)*64 + (i & 3)] = cmul(bt, cplx{t.re, -t.im});
    }
}

hipError_t launch_fold_w8(const double* segtab, const cplx* ops, int G, int A, cplx* wfold, hipStream_t stream) {
    hipLaunchKernelGGL(fold_w8_kernel, dim3(G, A), dim3(64), 0, stream, segtab, ops, A, wfold);
    return hipGetLastError();
}

hipError_t launch_prologue(const double* eigvals, const cplx* eigvecs, const cplx* propagators,
                           const cplx* n_opers, const double* n_coeffs, const double* dt,
                           const double* t, int G, int d, int A, double* segtab, cplx* Tc,
                           cplx* ops, cplx* n_opers_transformed, cplx* eigvecs_propagated,
                           hipStream_t stream, cplx* wfold) {
    if (generic_dimension(d))
        return launch_prologue_generic(eigvals, eigvecs, propagators, n_opers, n_coeffs, dt, t, G, d, A, segtab,
                                       Tc, ops, n_opers_transformed, eigvecs_propagated, stream);
    switch (d) {
#define FFK_CASE(D)                                                                             \
    case D:                                                                                     \
        hipLaunchKernelGGL(prologue_kernel<D>, dim3(G), dim3(64), 0, stream, eigvals, eigvecs,  \
                           propagators, n_opers, n_coeffs, dt, t, G, A, segtab, Tc, ops,        \
                           n_opers_transformed, eigvecs_propagated, !split_noise_ops(D, A),     \
                           D == 4 ? wfold : nullptr);                                           \
        if (split_noise_ops(D, A))                                                              \
            hipLaunchKernelGGL(noise_ops_kernel<D>, dim3(G, A), dim3(64), 0, stream, eigvecs,   \
                               n_opers, n_coeffs, G, A, ops, n_opers_transformed);              \
        break;
        FFK_CASE(2) FFK_CASE(3) FFK_CASE(4) FFK_CASE(5) FFK_CASE(6) FFK_CASE(7) FFK_CASE(8)
        FFK_CASE(9) FFK_CASE(10) FFK_CASE(11) FFK_CASE(12) FFK_CASE(13) FFK_CASE(14)
        FFK_CASE(15) FFK_CASE(16)
#undef FFK_CASE
        default:
            return hipErrorInvalidValue;
    }
    if (d == 8 && wfold != nullptr) return launch_fold_w8(segtab, ops, G, A, wfold, stream);
    return hipGetLastError();
}

hipError_t launch_prologue_pulses(const double* eigvals, const cplx* eigvecs, const cplx* propagators,
                                  const cplx* n_opers, const double* n_coeffs, const double* dt, const double* t,
                                  int G, int P, int d, int A, double* segtab, cplx* Tc, cplx* ops,
                                  cplx* n_opers_transformed, hipStream_t stream) {
    if (P < 1 || P > 65535 || !n_opers_transformed || !n_coeffs) return hipErrorInvalidValue;
    switch (d) {
#define FFK_CASE(D)                                                                             \
    case D:                                                                                     \
        hipLaunchKernelGGL(prologue_pulses_kernel<D>, dim3(G, P), dim3(64), 0, stream, eigvals, \
                           eigvecs, propagators, n_opers, n_coeffs, dt, t, G, A, segtab, Tc,    \
                           ops, n_opers_transformed);                                           \
        break;
        // (d <= 8: from d = 9 on no tile of the matrix-core second-order kernel fits in LDS, and nothing else asks)
        FFK_CASE(2) FFK_CASE(3) FFK_CASE(4) FFK_CASE(5) FFK_CASE(6) FFK_CASE(7) FFK_CASE(8)
#undef FFK_CASE
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_apply_prologue_compact(const cplx* Qloc, const cplx* totals, int G, int d, cplx* Q,
                                         const double* eigvals, const cplx* eigvecs,
                                         const cplx* n_opers, const double* n_coeffs,
                                         const double* dt, const double* t, int A, double* segtab,
                                         cplx* Tc, cplx* ops, const cplx* basis, int N, void* ews,
                                         hipStream_t stream, cplx* wfold) {
    const int L = front_chunk(d);
    int* nnz = nullptr;
    int* rows = nullptr;
    cplx* vals = nullptr;
    int extra = 0;
    if (basis) {
        expand_workspace_slices(ews, N, d, &nnz, &rows, &vals);
        extra = N;
    }
    switch (d) {
#define FFK_CASE(D)                                                                              \
    case D:                                                                                      \
        if (D > 8) {   /* (static 7 D^2 + dynamic 16 D^2 complex numbers: beyond the default limit) */ \
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(apply_prologue_kernel<D>), \
                                               hipFuncAttributeMaxDynamicSharedMemorySize,       \
                                               static_cast<int>(sizeof(cplx)*D*D*16));           \
            if (e != hipSuccess) return e;                                                       \
        }                                                                                        \
        hipLaunchKernelGGL(apply_prologue_kernel<D>, dim3(G + extra), dim3(64),                  \
                           sizeof(cplx)*D*D*(D <= 8 ? (G + L - 1)/L : 16), stream, Qloc,         \
                           totals, G, L, Q, eigvals, eigvecs, n_opers, n_coeffs, dt, t, A,       \
                           segtab, Tc, ops, basis, nnz, rows, vals, !split_noise_ops(D, A),      \
                           D == 4 ? wfold : nullptr);                                            \
        if (split_noise_ops(D, A))                                                               \
            hipLaunchKernelGGL(noise_ops_kernel<D>, dim3(G, A), dim3(64), 0, stream, eigvecs,    \
                               n_opers, n_coeffs, G, A, ops, nullptr);                           \
        break;
        FFK_CASE(2) FFK_CASE(3) FFK_CASE(4) FFK_CASE(5) FFK_CASE(6) FFK_CASE(7) FFK_CASE(8)
        FFK_CASE(9) FFK_CASE(10) FFK_CASE(11) FFK_CASE(12) FFK_CASE(13) FFK_CASE(14)
        FFK_CASE(15) FFK_CASE(16)
#undef FFK_CASE
        default:
            return hipErrorInvalidValue;
    }
    if (d == 8 && wfold != nullptr) return launch_fold_w8(segtab, ops, G, A, wfold, stream);
    return hipGetLastError();
}

hipError_t launch_apply_prologue_compact_pulses(const cplx* Qloc, const cplx* totals, int G, int P, int d,
                                                cplx* Q, const double* eigvals, const cplx* eigvecs,
                                                const cplx* n_opers, const double* n_coeffs, const double* dt,
                                                const double* t, int A, double* segtab, cplx* Tc, cplx* ops,
                                                const cplx* basis, int N, void* ews, hipStream_t stream,
                                                cplx* wfold) {
    const int L = front_chunk(d);
    const int nchunks = (G + L - 1)/L;
    if (P < 1 || P > 65535 || !basis) return hipErrorInvalidValue;
    int* nnz = nullptr;
    int* rows = nullptr;
    cplx* vals = nullptr;
    expand_workspace_slices(ews, N, d, &nnz, &rows, &vals);
    switch (d) {
#define FFK_CASE(D)                                                                              \
    case D:                                                                                      \
        if (D > 8) {                                                                             \
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(apply_prologue_pulses_kernel<D>), \
                                               hipFuncAttributeMaxDynamicSharedMemorySize,       \
                                               static_cast<int>(sizeof(cplx)*D*D*16));           \
            if (e != hipSuccess) return e;                                                       \
        }                                                                                        \
        hipLaunchKernelGGL(apply_prologue_pulses_kernel<D>, dim3(G + N, P), dim3(64),            \
                           sizeof(cplx)*D*D*(D <= 8 ? nchunks : 16), stream, Qloc, totals, G, L, \
                           nchunks, Q, eigvals, eigvecs, n_opers, n_coeffs, dt, t, A, segtab, Tc, \
                           ops, basis, nnz, rows, vals, D == 4 ? wfold : nullptr);               \
        break;
        FFK_CASE(2) FFK_CASE(3) FFK_CASE(4) FFK_CASE(5) FFK_CASE(6) FFK_CASE(7) FFK_CASE(8)
        FFK_CASE(9) FFK_CASE(10) FFK_CASE(11) FFK_CASE(12) FFK_CASE(13) FFK_CASE(14)
        FFK_CASE(15) FFK_CASE(16)
#undef FFK_CASE
        default:
            return hipErrorInvalidValue;
    }
    // (d = 8: the fold reads only segtab and ops, per segment: the P G segments in one launch)
    if (d == 8 && wfold != nullptr) return launch_fold_w8(segtab, ops, P*G, A, wfold, stream);
    return hipGetLastError();
}

hipError_t launch_apply_prologue(const cplx* Qloc, const cplx* totals, int G, int d, cplx* Q,
                                 const double* eigvals, const cplx* eigvecs, const cplx* n_opers,
                                 const double* n_coeffs, const double* dt, const double* t, int A,
                                 double* segtab, cplx* Tc, cplx* ops, hipStream_t stream) {
    return launch_apply_prologue_compact(Qloc, totals, G, d, Q, eigvals, eigvecs, n_opers, n_coeffs,
                                         dt, t, A, segtab, Tc, ops, nullptr, 0, nullptr, stream);
}

hipError_t launch_basis_transformed(const cplx* Tc, const cplx* basis, int G, int N, int d,
                                    cplx* out, hipStream_t stream) {
    if (N > 65535) return hipErrorInvalidValue;
    switch (d) {
#define FFK_CASE(D)                                                                            \
    case D:                                                                                    \
        hipLaunchKernelGGL(basis_transformed_kernel<D>, dim3(G, N), dim3(64), 0, stream, Tc,   \
                           basis, N, out);                                                     \
        break;
        FFK_CASE(2) FFK_CASE(3) FFK_CASE(4) FFK_CASE(5) FFK_CASE(6) FFK_CASE(7) FFK_CASE(8)
        FFK_CASE(9) FFK_CASE(10) FFK_CASE(11) FFK_CASE(12) FFK_CASE(13) FFK_CASE(14)
        FFK_CASE(15) FFK_CASE(16)
#undef FFK_CASE
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_phase_and_integral(const double* omega, int W, const double* segtab, int G,
                                     int d, cplx* phase_factors, cplx* integral,
                                     hipStream_t stream) {
    if (!phase_factors && !integral) return hipSuccess;
    const int block = 128;
    if ((W + block - 1)/block > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(phase_integral_kernel, dim3(G, (W + block - 1)/block), dim3(block), 0,
                       stream, omega, W, segtab, d, seg_stride(d), phase_factors, integral);
    return hipGetLastError();
}

}  // namespace ffk

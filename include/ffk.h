/* ffk.h -- C ABI of libffk.so: the MI355X (gfx950) filter-function hot path.
 *
 * This is the drop-in boundary for the numeric hot path of qutech/filter_functions
 * (reference v1.2.1).  The reference has no FFI of its own: the path sits behind Python
 * free functions in filter_functions/numeric.py and superoperator.py.  Every entry point
 * below replaces exactly one of those functions; the citation names the reference
 * interface (file:line relative to the reference root) whose arguments, array layouts and
 * results it reproduces.  INTEGRATION.md shows the ctypes stub a reference maintainer
 * would add.
 *
 * Conventions
 *   - All arrays are C-contiguous.  "c128" is complex128 stored interleaved (re, im) as two
 *     doubles, identical to NumPy's layout; such arrays are passed as `const double*` /
 *     `double*` and have 2x the element count in doubles.
 *   - Plain pointers and sizes only.  No torch / numpy types.
 *   - Every function returns FFK_OK (0) or a negative FFK_E* code; ffk_last_error() returns
 *     a thread-local message for the last failure.
 *   - Two flavours per operation:
 *       ffk_<op>      host pointers in/out; the library stages through its own device
 *                     arena (H2D, kernels, D2H, synchronous).  This is what the NumPy-
 *                     facing Python front-end calls.
 *       ffk_<op>_dev  device pointers in/out, asynchronous on `stream` (a hipStream_t cast
 *                     to void*, NULL = default stream); scratch memory is supplied by the
 *                     caller (size from the matching *_workspace_bytes query).  No
 *                     allocation, no synchronisation: safe to capture in a hipGraph.  This
 *                     is what bench.py and the multi-GPU driver call with HBM-resident data.
 *   - d (Hilbert-space dimension) must satisfy 2 <= d <= FFK_MAX_D (64) for the path the reference's
 *     get_filter_function / infidelity / liouville_representation walk: ffk_diagonalize*,
 *     ffk_control_matrix* (control matrix and noise operators), ffk_filter_function*, ffk_infidelity*,
 *     ffk_decay_amplitudes*, ffk_cumulant_function*, ffk_expm_real, ffk_error_transfer_matrix_dev (the one
 *     `_dev` call that synchronises its stream, see there), ffk_control_matrix_from_atomic*, ffk_liouville*.  Up to
 *     FFK_MAX_D_TEMPLATED (16) the kernels are compiled per dimension (operands in registers or
 *     wave-private LDS); above it one runtime-d kernel set serves (csrc/generic.hip, workgroup-wide
 *     LDS tiles).  The remaining entry points (intermediates, second order, gradients, fused
 *     pipeline and resident passes, sequence concatenation in one call) accept
 *     d <= FFK_MAX_D_TEMPLATED only and return FFK_EINVAL above it.
 *   - Thread-safety: calls on one device are serialised by the caller; the library keeps one
 *     arena per process and device.
 */
#ifndef FFK_H
#define FFK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFK_VERSION 100 /* 0.1.0 */
#define FFK_MAX_D 64
#define FFK_MAX_D_TEMPLATED 16

#define FFK_OK 0
#define FFK_EINVAL -1   /* bad argument (shape, NULL, unsupported d) -> ValueError        */
#define FFK_EHIP -2     /* a HIP runtime call failed -> RuntimeError                       */
#define FFK_ENOMEM -3   /* device allocation failed / workspace too small -> MemoryError   */
#define FFK_ENOCONV -4  /* Jacobi eigensolver did not converge -> numpy.linalg.LinAlgError */
#define FFK_EKERNEL -5  /* a kernel reported an internal fault (a bounded wait between its       */
                        /* wavefronts ran out): the launch's results are invalid -> RuntimeError */

/* flags for ffk_control_matrix* */
#define FFK_WANT_NOISE_OPERATORS 0x1 /* also return B~(w) laid out (W, A, d, d)           */

/* which for ffk_filter_function* (numeric.py:1414 `which`) */
#define FFK_FF_FIDELITY 0
#define FFK_FF_GENERALIZED 1

/* ---- library / device management ------------------------------------------------------ */
const char* ffk_last_error(void);
int ffk_version(void);
int ffk_device_count(int* count);
int ffk_set_device(int device);
int ffk_get_device(int* device);
/* name (<= len-1 chars), compute units, total global memory bytes of the current device */
int ffk_device_info(char* name, int len, int* compute_units, size_t* global_mem_bytes);

/* ---- device memory, streams, events (so a host language without a HIP binding can keep
 *      data resident and time kernels on the stream they run on) --------------------------- */
int ffk_malloc(void** dptr, size_t bytes);
/* device memory that other agents (peer GPUs) may write while a local kernel polls it: fine-grained
 * coherence (hipExtMallocWithFlags).  FFK_EHIP if the runtime refuses: there is no silent
 * coarse-grained substitute (flag words polled by a running kernel would not be coherent) */
int ffk_malloc_finegrained(void** dptr, size_t bytes);
int ffk_free(void* dptr);
int ffk_memset(void* dptr, int value, size_t bytes, void* stream);
int ffk_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int ffk_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int ffk_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
int ffk_stream_create(void** stream);
int ffk_stream_destroy(void* stream);
int ffk_stream_synchronize(void* stream);
int ffk_device_synchronize(void);
int ffk_event_create(void** event);
int ffk_event_destroy(void* event);
int ffk_event_record(void* event, void* stream);
int ffk_event_synchronize(void* event);
int ffk_event_elapsed_ms(void* start, void* stop, float* ms);
/* release the library's cached device arena (host-pointer flavour) */
int ffk_release_arena(void);

/* ---- numeric.diagonalize (filter_functions/numeric.py:1886-1935; caller
 *      pulse_sequence.py:577-586) ----------------------------------------------------------
 * hamiltonian (G, d, d) c128 -- only the LOWER triangle is read (numpy.linalg.eigh default);
 * dt (G,) f64.
 * -> eigvals (G, d) f64 ascending; eigvecs (G, d, d) c128, columns are eigenvectors;
 *    propagators (G+1, d, d) c128 with propagators[0] = 1 and
 *    propagators[g+1] = V_g exp(-i D_g dt_g) V_g^dag propagators[g].                        */
int ffk_diagonalize(const double* hamiltonian, const double* dt, int G, int d,
                    double* eigvals, double* eigvecs, double* propagators);
size_t ffk_diagonalize_workspace_bytes(int G, int d);
int ffk_diagonalize_dev(const double* hamiltonian, const double* dt, int G, int d,
                        double* eigvals, double* eigvecs, double* propagators,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- numeric.calculate_control_matrix_from_scratch (numeric.py:707-881; callers
 *      pulse_sequence.py:625, 1843, 2595) and its Hilbert-space twin
 *      numeric.calculate_noise_operators_from_scratch (numeric.py:456-618) -----------------
 * eigvals (G, d) f64, eigvecs (G, d, d) c128, propagators (G+1, d, d) c128, omega (W,) f64,
 * basis (N, d, d) c128, n_opers (A, d, d) c128, n_coeffs (A, G) f64, dt (G,) f64,
 * t (G+1,) f64 (absolute segment times; t[0] is usually 0).
 * -> control_matrix (A, N, W) c128, omega fastest (may be NULL if only the noise operators
 *    are wanted); with FFK_WANT_NOISE_OPERATORS also noise_operators (W, A, d, d) c128,
 *    omega slowest -- both exactly the reference's layouts.                                */
int ffk_control_matrix(const double* eigvals, const double* eigvecs, const double* propagators,
                       const double* omega, int W, const double* basis, int N,
                       const double* n_opers, int A, const double* n_coeffs, const double* dt,
                       const double* t, int G, int d, unsigned flags, double* control_matrix,
                       double* noise_operators);
size_t ffk_control_matrix_workspace_bytes(int W, int N, int A, int G, int d);
int ffk_control_matrix_dev(const double* eigvals, const double* eigvecs,
                           const double* propagators, const double* omega, int W,
                           const double* basis, int N, const double* n_opers, int A,
                           const double* n_coeffs, const double* dt, const double* t, int G,
                           int d, unsigned flags, double* control_matrix,
                           double* noise_operators, void* workspace, size_t workspace_bytes,
                           void* stream);

/* The `cache_intermediates=True` products of numeric.py:828-833, 871-878 (materialising,
 * HBM-bound variant).  Any output pointer may be NULL to skip it.
 *   n_opers_transformed (A, G, d, d), eigvecs_propagated (G, d, d), basis_transformed
 *   (G, N, d, d), phase_factors (G, W), first_order_integral (G, W, d, d),
 *   control_matrix_step (G, A, N, W); all c128.  (control_matrix_step_cumulative is the
 *   running sum of control_matrix_step and is formed by the host wrapper.)                 */
int ffk_control_matrix_intermediates(
    const double* eigvals, const double* eigvecs, const double* propagators,
    const double* omega, int W, const double* basis, int N, const double* n_opers, int A,
    const double* n_coeffs, const double* dt, const double* t, int G, int d,
    double* n_opers_transformed, double* eigvecs_propagated, double* basis_transformed,
    double* phase_factors, double* first_order_integral, double* control_matrix_step);
/* The cache_intermediates products of calculate_noise_operators_from_scratch
 * (numeric.py:586-615): n_opers_transformed (A, G, d, d), phase_factors (G, W),
 * first_order_integral (G, W, d, d), noise_operators_step (G, W, A, d, d) c128 (any may be NULL). */
int ffk_noise_operators_intermediates(const double* eigvals, const double* eigvecs,
                                      const double* propagators, const double* omega, int W,
                                      const double* n_opers, int A, const double* n_coeffs,
                                      const double* dt, const double* t, int G, int d,
                                      double* n_opers_transformed, double* phase_factors,
                                      double* first_order_integral, double* noise_operators_step);

/* ---- numeric.calculate_control_matrix_from_atomic (numeric.py:621-704; caller
 *      pulse_sequence.concatenate pulse_sequence.py:1858) -- the concatenation rule -----------
 * phases (G-1, W) c128 cumulated total phase factors; control_matrix_atomic (G, A, N, W) c128;
 * propagators_liouville (G-1, N, N), f64 if l_is_complex == 0 else c128.
 * which 0 ('total'): out (A, N, W) = R^(0) + sum_g phases[g-1] R^(g) L^(g-1);
 * which 1 ('correlations'): out (G, A, N, W), every summand.                                */
int ffk_control_matrix_from_atomic(const double* phases, const double* control_matrix_atomic,
                                   const double* propagators_liouville, int l_is_complex, int G,
                                   int A, int N, int W, int which, double* out);
size_t ffk_control_matrix_from_atomic_workspace_bytes(int G, int A, int N, int W);
int ffk_control_matrix_from_atomic_dev(const double* phases, const double* control_matrix_atomic,
                                       const double* propagators_liouville, int l_is_complex,
                                       int G, int A, int N, int W, int which, double* out,
                                       void* workspace, size_t workspace_bytes, void* stream);

/* The same rule for sequences drawn from T distinct pulses (pulse_sequence.concatenate called with
 * repeated PulseSequence objects, e.g. examples/randomized_benchmarking.py:76-81):
 * total_phases (T, W) c128 = exp(i omega tau) of every distinct pulse, control_matrix_table
 * (T, A, N, W) c128, index (G,) int32 = which distinct pulse sits at position g.  The cumulated
 * phases of pulse_sequence.py:1824 are formed in the kernel.                                   */
int ffk_control_matrix_from_atomic_indexed(const double* total_phases,
                                           const double* control_matrix_table,
                                           const int32_t* index,
                                           const double* propagators_liouville, int l_is_complex,
                                           int T, int G, int A, int N, int W, int which,
                                           double* out);
int ffk_control_matrix_from_atomic_indexed_dev(const double* total_phases,
                                               const double* control_matrix_table,
                                               const int32_t* index,
                                               const double* propagators_liouville,
                                               int l_is_complex, int T, int G, int A, int N, int W,
                                               int which, double* out, void* workspace,
                                               size_t workspace_bytes, void* stream);

/* ---- pulse_sequence.concatenate (pulse_sequence.py:1668-1887) for a sequence of G positions drawn
 * from T distinct pulses, the whole rule in one call: total_propagators (T, d, d) c128 of the
 * distinct pulses, their total_phases (T, W) c128 and control_matrix_table (T, A, N, W) c128,
 * index (G,) int32, basis (N, d, d) c128.  The cumulative propagators (util.adot, :1812), their
 * Liouville representations (:1827), the cumulative phases (:1824) and the sum (:1836,
 * numeric.calculate_control_matrix_from_atomic) all run on the device.  Returns the control matrix
 * ((A, N, W); (G, A, N, W) for which = 1), the total propagator (d, d) and, if
 * propagators_liouville is not NULL, the (G - 1, N, N) cumulative Liouville propagators (f64 if
 * hermitian_basis, else c128); if filter_function is not NULL (which = 0 only), also the fidelity
 * filter function (A, A, W) of the result (numeric.calculate_filter_function).                    */
int ffk_concatenate_sequence(const double* total_propagators, const double* total_phases,
                             const double* control_matrix_table, const int32_t* index,
                             const double* basis, int hermitian_basis, int T, int G, int d, int A,
                             int N, int W, int which, double* control_matrix,
                             double* total_propagator, double* propagators_liouville,
                             double* filter_function);

/* The same for distinct pulses whose control matrices are still resident in HBM (each evaluated by
 * ffk_resident_filter_function[_from_controls] on the same frequency grid, same device): handles
 * (T,), tau (T,) f64 total durations (the total phases exp(i omega tau) are formed on the device
 * from the resident grid), index (G,) int32, basis (N, d, d) c128.  The table of control matrices
 * is assembled by device-to-device copies; shapes come from the handles.  With `result` (another
 * handle; which = 0 and filter_function required, control_matrix may be NULL) the summed control
 * matrix, its filter function and the grid stay resident in it: ffk_resident_control_matrix and
 * ffk_resident_infidelity serve the concatenated pulse, and it can be an input of a further call. */
struct ffk_resident;
int ffk_concatenate_sequence_resident(struct ffk_resident* const* pulses, const double* tau,
                                      const int32_t* index, const double* basis, int hermitian_basis,
                                      int T, int G, int which, double* control_matrix,
                                      double* total_propagator, double* propagators_liouville,
                                      double* filter_function, struct ffk_resident* result);

/* ---- numeric.calculate_control_matrix_periodic (numeric.py:886-954) ----------------------
 * phases (W,) c128 = exp(i omega T) of one period, control_matrix (A, N, W) c128 of one period,
 * total_propagator_liouville (N, N) f64 (or c128 if l_is_complex) of one period -> the control
 * matrix (A, N, W) c128 of `repeats` periods.  The reference evaluates the geometric series in
 * closed form (one inverse per frequency, with a term-by-term fallback where it is ill
 * conditioned); here it is summed by doubling in ~2 log2(repeats) streaming passes, no inverse. */
int ffk_control_matrix_periodic(const double* phases, const double* control_matrix,
                                const double* total_propagator_liouville, int l_is_complex, int repeats,
                                int A, int N, int W, double* out);
size_t ffk_control_matrix_periodic_workspace_bytes(int A, int N, int W);
int ffk_control_matrix_periodic_dev(const double* phases, const double* control_matrix,
                                    const double* total_propagator_liouville, int l_is_complex,
                                    int repeats, int A, int N, int W, double* out, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* ---- numeric.calculate_filter_function (numeric.py:1413-1467) --------------------------
 * control_matrix (A, N, W) c128 -> fidelity: (A, A, W) c128,
 *                                  generalized: (A, A, N, N, W) c128.                       */
int ffk_filter_function(const double* control_matrix, int A, int N, int W, int which,
                        double* filter_function);
int ffk_filter_function_dev(const double* control_matrix, int A, int N, int W, int which,
                            double* filter_function, void* stream);

/* The filter function of a basis that is not traceless (numeric.py:2295-2305):
 * F[a,b,w] = scale * sum_kl conj(R[a,k,w]) M[k,l] R[b,l,w], weights M (N, N) c128 built by the
 * caller from the four-element traces of the basis, scale = 1/d.                               */
int ffk_filter_function_weighted(const double* control_matrix, int A, int N, int W,
                                 const double* weights, double scale, double* filter_function);
int ffk_filter_function_weighted_dev(const double* control_matrix, int A, int N, int W,
                                     const double* weights, double scale, double* filter_function,
                                     void* stream);

/* ---- numeric.infidelity, filter-function branch (numeric.py:2307-2320 with _get_integrand
 *      :323-325, :351-352, :374 and util.integrate util.py:880-906) ------------------------
 * filter_function (A, A, W) c128; omega (W,) f64; idx (n_idx,) int32 noise-operator indices;
 * spectrum c128 with s_ndim in {1, 2, 3}: (W,), (n_idx, W) or (n_idx, n_idx, W) (already
 * validated / broadcast by the caller as util.parse_spectrum util.py:214-227 does).
 * -> infid f64: (n_idx,) for s_ndim 1 or 2, (n_idx, n_idx) for s_ndim 3:
 *    Re-part trapezoid of S*F over omega, divided by 2 pi d.                                 */
int ffk_infidelity(const double* filter_function, int A, int W, const double* spectrum,
                   int s_ndim, const double* omega, const int32_t* idx, int n_idx, int d,
                   double* infid);
size_t ffk_infidelity_workspace_bytes(int W, int n_idx, int s_ndim);
int ffk_infidelity_dev(const double* filter_function, int A, int W, const double* spectrum,
                       int s_ndim, const double* omega, const int32_t* idx, int n_idx, int d,
                       double* infid, void* workspace, size_t workspace_bytes, void* stream);

/* The same integral on the raw buffer of an all-gather over omega blocks: filter_function_shards
 * (n_shards, A, A, shard_width) c128, block r holding frequencies [r, r+1) * shard_width of the
 * global grid omega (n_shards * shard_width,).  Saves the re-layout pass on the multi-GPU path. */
int ffk_infidelity_sharded_dev(const double* filter_function_shards, int n_shards, int shard_width,
                               int A, const double* spectrum, int s_ndim, const double* omega,
                               const int32_t* idx, int n_idx, int d, double* infid, void* stream);

/* ---- numeric.calculate_noise_operators_from_atomic (numeric.py:377-453) -------------------
 * phases (G-1, W) c128, noise_operators_atomic (G, W, A, d, d) c128, propagators (G-1, d, d) c128
 * -> noise_operators (W, A, d, d):  B = B^(0) + sum_{g>=1} phases[g-1] P_{g-1}^dag B^(g) P_{g-1}. */
int ffk_noise_operators_from_atomic(const double* phases, const double* noise_operators_atomic,
                                    const double* propagators, int G, int W, int A, int d,
                                    double* noise_operators);

/* ---- numeric.calculate_decay_amplitudes (numeric.py:1194-1337; integrand _get_integrand
 *      :310-374 'generalized' with the control matrix; util.integrate util.py:880-906) -------
 * control_matrix (n_pulses, A, N, W) c128: n_pulses = 1 is the total control matrix
 * (which='total'), n_pulses = G the pulse-correlation control matrix (which='correlations').
 * spectrum / s_ndim / idx / n_idx as in ffk_infidelity.
 * -> decay_amplitudes f64: (n_pulses, n_pulses, n_idx, N, N) for s_ndim 1 or 2,
 *    (n_pulses, n_pulses, n_idx, n_idx, N, N) for s_ndim 3:
 *    Gamma[g,h,a,b,k,l] = int dw/2pi Re(R*[g,a,k,w] S_ab(w) R[h,b,l,w])  (trapezoid).          */
size_t ffk_decay_amplitudes_workspace_bytes(int n_pulses, int N, int W, int n_idx, int s_ndim);
int ffk_decay_amplitudes_dev(const double* control_matrix, int n_pulses, int A, int N, int W,
                             const double* spectrum, int s_ndim, const double* omega,
                             const int32_t* idx, int n_idx, double* decay_amplitudes,
                             void* workspace, size_t workspace_bytes, void* stream);
int ffk_decay_amplitudes(const double* control_matrix, int n_pulses, int A, int N, int W,
                         const double* spectrum, int s_ndim, const double* omega,
                         const int32_t* idx, int n_idx, double* decay_amplitudes);
/* The contribution of one frequency block to the same integral (multi-GPU path):
 * control_matrix (n_pulses, A, N, W_block) and spectrum ([[n_idx,] n_idx,] W_block) hold the
 * frequencies [w_offset, w_offset + W_block) of the global grid omega (W,); the trapezoid
 * weights are those of the global grid, so the blocks' results add up to ffk_decay_amplitudes
 * of the whole grid.                                                                           */
int ffk_decay_amplitudes_shard_dev(const double* control_matrix, int n_pulses, int A, int N,
                                   int W_block, const double* spectrum, int s_ndim,
                                   const double* omega, int W, int w_offset, const int32_t* idx,
                                   int n_idx, double* decay_amplitudes, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ---- numeric.calculate_cumulant_function, first order (numeric.py:957-1191) ----------------
 * decay_amplitudes (batch, N, N) f64 (any leading axes flattened into batch), basis (N, d, d)
 * c128 -> cumulant_function (batch, N, N) f64,
 *    K_ij = -1/2 sum_kl Gamma_kl (T_klji - T_kjli - T_kilj + T_kijl),  T = Basis.four_element_traces
 * (basis.py:330-348), evaluated without forming T.  single_qubit != 0 selects the simplified
 * expression the reference uses for d = 2 with a Pauli or GGM basis (:1119-1141).             */
size_t ffk_cumulant_function_workspace_bytes(int batch, int N, int d);
int ffk_cumulant_function_dev(const double* decay_amplitudes, int batch, int N, int d,
                              const double* basis, int single_qubit, double* cumulant_function,
                              void* workspace, size_t workspace_bytes, void* stream);
int ffk_cumulant_function(const double* decay_amplitudes, int batch, int N, int d,
                          const double* basis, int single_qubit, double* cumulant_function);

/* ---- second order: numeric.calculate_second_order_filter_function_from_scratch
 *      (numeric.py:1470-1699, nested integral :170-256), numeric.calculate_frequency_shifts
 *      (:1340-1410) and the frequency-shift terms of calculate_cumulant_function (:1139-1141,
 *      :1166-1190) ---------------------------------------------------------------------------
 * Inputs as ffk_control_matrix.  filter_function_2 (A, A, N, N, W) c128, omega fastest.        */
int ffk_second_order_filter_function(const double* eigvals, const double* eigvecs,
                                     const double* propagators, const double* omega, int W,
                                     const double* basis, int N, const double* n_opers, int A,
                                     const double* n_coeffs, const double* dt, const double* t, int G,
                                     int d, double* filter_function_2);
/* numeric.calculate_second_order_filter_function_from_atomic (numeric.py:1702-1818), the
 * concatenation rule: filter_function_atomic (G, A, A, N, N, W) c128 = each pulse's own F2,
 * control_matrix_step (G, A, N, W) c128 = the summands of the sequence's control matrix
 * (ffk_control_matrix_from_atomic with correlations != 0), propagators_liouville (G-1, N, N) f64
 * (Hermitian basis) -> filter_function_2 (A, A, N, N, W).                                       */
int ffk_second_order_filter_function_from_atomic(const double* filter_function_atomic,
                                                 const double* control_matrix_step,
                                                 const double* propagators_liouville, int G, int A,
                                                 int N, int W, double* filter_function_2);
/* Delta = int dw/2pi Re(S F2): spectrum/s_ndim/idx as in ffk_decay_amplitudes; frequency_shifts
 * (n_idx, N, N) f64 for s_ndim 1, 2 and (n_idx, n_idx, N, N) for s_ndim 3.                      */
int ffk_frequency_shifts(const double* filter_function_2, int A, int N, int W, const double* spectrum,
                         int s_ndim, const double* omega, const int32_t* idx, int n_idx,
                         double* frequency_shifts);
/* Both in one device-resident pass (F2 never crosses PCIe unless filter_function_2 != NULL, in
 * which case it is returned as well, for the caller's cache).                                   */
int ffk_frequency_shifts_from_scratch(const double* eigvals, const double* eigvecs,
                                      const double* propagators, const double* omega, int W,
                                      const double* basis, int N, const double* n_opers, int A,
                                      const double* n_coeffs, const double* dt, const double* t, int G,
                                      int d, const double* spectrum, int s_ndim, const int32_t* idx,
                                      int n_idx, double* filter_function_2, double* frequency_shifts);
/* cumulant_function (batch, N, N) f64, IN/OUT: the first-order result of ffk_cumulant_function, to
 * which -1/2 sum_kl Delta_kl (T_klji - T_lkji - T_klij + T_lkij) is added, evaluated as the
 * commutator -1/2 Re tr(C_i [X, C_j]), X = sum_kl (Delta_kl - Delta_lk) C_k C_l (which is also the
 * reference's single-qubit expression -(Delta - Delta^T) on the traceless block).              */
int ffk_cumulant_function_second_order(const double* frequency_shifts, int batch, int N, int d,
                                       const double* basis, double* cumulant_function);

/* Device-resident flavours (device pointers, caller-provided workspace, asynchronous on `stream`);
 * ffk_frequency_shifts_shard_dev integrates the frequency block [w_offset, w_offset + W_block) of
 * the global grid omega (W,) with the global trapezoid weights (multi-GPU: the per-rank results
 * add up to the unsharded integral).                                                            */
size_t ffk_second_order_workspace_bytes(int W, int N, int A, int G, int d);
int ffk_second_order_filter_function_dev(const double* eigvals, const double* eigvecs,
                                         const double* propagators, const double* omega, int W,
                                         const double* basis, int N, const double* n_opers, int A,
                                         const double* n_coeffs, const double* dt, const double* t,
                                         int G, int d, double* filter_function_2, void* workspace,
                                         size_t workspace_bytes, void* stream);
size_t ffk_frequency_shifts_workspace_bytes(int W, int n_idx, int s_ndim);
int ffk_frequency_shifts_shard_dev(const double* filter_function_2, int A, int N, int W_block,
                                   const double* spectrum, int s_ndim, const double* omega, int W,
                                   int w_offset, const int32_t* idx, int n_idx,
                                   double* frequency_shifts, void* workspace, size_t workspace_bytes,
                                   void* stream);
size_t ffk_cumulant_function_second_order_workspace_bytes(int batch, int N, int d);
int ffk_cumulant_function_second_order_dev(const double* frequency_shifts, int batch, int N, int d,
                                           const double* basis, double* cumulant_function,
                                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- gradient (filter_functions/gradient.py; PulseSequence.get_filter_function_derivative,
 *      pulse_sequence.py:977-1054; gradient.infidelity_derivative, gradient.py:559-676) ----------
 * Derivative of the fidelity filter function of each noise operator with respect to the amplitude
 * of control operator h during segment s: filter_function_derivative (A, G, H, W) f64 (the
 * reference's (n_nops, n_dt, n_ctrl, n_omega)); infidelity_derivative (A, G, H) f64 =
 * int dw/(2 pi d) S_a(w) dF_a/du_h(t_s) for a spectrum (W,) or (A, W) c128 (s_ndim 1, 2).  Either
 * output may be NULL.  c_opers (H, d, d) c128: the control operators to differentiate by (the
 * eigensystem is that of the full control Hamiltonian); n_coeffs_ratio (A, H, G) f64 or NULL:
 * (d n_coeffs[a, s] / d u_h(t_s)) / n_coeffs[a, s], the explicit dependence of the noise
 * sensitivities on the controls (gradient.py:376-379).  Supports 2 <= d <= 8.                  */
int ffk_filter_function_derivative(const double* eigvals, const double* eigvecs,
                                   const double* propagators, const double* omega, int W,
                                   const double* n_opers, int A, const double* n_coeffs,
                                   const double* c_opers, int H, const double* n_coeffs_ratio,
                                   const double* dt, const double* t, int G, int d,
                                   const double* spectrum, int s_ndim,
                                   double* filter_function_derivative,
                                   double* infidelity_derivative);

/* The two tensor-level gradient functions of the reference.
 * ffk_control_matrix_derivative: gradient.calculate_derivative_of_control_matrix_from_scratch
 * (gradient.py:384-523): control_matrix_derivative (H, W, G, A, N) c128 = d R_ak(w) / d u_h(t_s)
 * [the reference's (n_ctrl, n_omega, n_dt, n_nops, d**2)]; basis (N, d, d) c128; the other arguments
 * as for ffk_filter_function_derivative.  2 <= d <= 8.
 * ffk_filter_function_derivative_from_control_matrix: gradient.calculate_filter_function_derivative
 * (gradient.py:526-556): (A, G, H, W) f64 = 2 Re sum_k conj(R[a,k,w]) dR[h,w,s,a,k] from
 * control_matrix (A, N, W) c128 and control_matrix_derivative (H, W, G, A, N) c128.              */
int ffk_control_matrix_derivative(const double* eigvals, const double* eigvecs, const double* propagators,
                                  const double* omega, int W, const double* basis, int N,
                                  const double* n_opers, int A, const double* n_coeffs,
                                  const double* c_opers, int H, const double* n_coeffs_ratio,
                                  const double* dt, const double* t, int G, int d,
                                  double* control_matrix_derivative);
int ffk_filter_function_derivative_from_control_matrix(const double* control_matrix,
                                                       const double* control_matrix_derivative, int A,
                                                       int N, int W, int G, int H,
                                                       double* filter_function_derivative);

/* Device-resident flavour on one block [w_offset, w_offset + W_block) of the global grid omega (W,):
 * omega_block (W_block,) are the block's frequencies, spectrum (W_block,) or (A, W_block) its part of
 * the spectrum; the trapezoid weights are those of the global grid, so the per-rank
 * infidelity_derivative results add up to the unsharded one (multi-GPU).
 * filter_function_derivative (A, G, H, W_block) is required (device scratch if not wanted).       */
size_t ffk_filter_function_derivative_workspace_bytes(int W, int A, int H, int G, int d);
int ffk_filter_function_derivative_shard_dev(const double* eigvals, const double* eigvecs,
                                             const double* propagators, const double* omega_block,
                                             int W_block, const double* n_opers, int A,
                                             const double* n_coeffs, const double* c_opers, int H,
                                             const double* n_coeffs_ratio, const double* dt,
                                             const double* t, int G, int d, const double* spectrum,
                                             int s_ndim, const double* omega, int W, int w_offset,
                                             double* filter_function_derivative,
                                             double* infidelity_derivative, void* workspace,
                                             size_t workspace_bytes, void* stream);

/* ---- exp of the summed cumulant function (numeric.error_transfer_matrix, numeric.py:2049-2053;
 *      the reference calls scipy.linalg.expm) ---------------------------------------------------
 * matrix (N, N) f64 row-major -> result (N, N) = exp(matrix): scaling and squaring with a Taylor
 * polynomial of degree 18, every product on v_mfma_f64_16x16x4.                                */
int ffk_expm_real(const double* matrix, int N, double* result);

/* The same for a cumulant function that is already in HBM (round 6): cumulant_function (batch, N, N) f64 is summed
 * over its leading axis in order (numeric.py:2049: `cumulant_function.sum(axis=...)`), the 1-norm that sizes the
 * scaling is taken on the device (16 bytes cross to the host, one stream synchronisation: the number of squarings
 * decides how many products are enqueued), result (N, N) f64 stays in HBM.  NaN / Inf in the sum: FFK_EINVAL.  */
size_t ffk_error_transfer_matrix_workspace_bytes(int N);
int ffk_error_transfer_matrix_dev(const double* cumulant_function, int batch, int N, double* result,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- exp of MANY small matrices at once (ff.exponentiate_cumulant_functions, the error transfer matrices after
 *      every gate of ff.sequence_prefix_error_transfer_matrices) ---------------------------------------------------
 * tiles (count, rows, N, N) f64 row-major, 1 <= N <= 16 -> result (count, N, N) f64: matrix i is the sum of its
 * `rows` tiles, added in order (as NumPy's sum over the leading axes), and result[i] its exponential by the plan of
 * ffk_expm_real -- 1-norm, halvings until it is at most 1/2, Taylor polynomial of degree 18 (B^2, B^3, B^4 once, then
 * Horner in B^4), squarings -- with the number of squarings chosen on the device, per matrix.  One launch whatever
 * count: N = 4 runs one matrix per lane in registers, every other N one matrix per wavefront on v_mfma_f64_16x16x4.
 * The sums inside the products are ordered differently from ffk_expm_real's, so the results are close to, not the
 * bits of, that call; a matrix's result is the same bits at every count, at every place among the others and in
 * every split.  not_finite (count,) int32: 1 where the sum holds a NaN or Inf -- that matrix's result tile is then not
 * written --, else 0.
 *   ffk_expm_real_batch_dev: device pointers; launches only -- no copy, no synchronisation, no allocation, no
 *     workspace (unlike ffk_error_transfer_matrix_dev it is legal during stream capture).
 *   ffk_expm_real_batch: host pointers; chunks of what the staging arena's budget of 1 GiB takes, each one H2D copy,
 *     one launch and the D2H copies of its results and flags (a chunk's results come back whole: the HOST tile of a
 *     flagged matrix holds no meaningful value afterwards).
 *   ffk_expm_real_batch_workspace_bytes: the device bytes the host-pointer call stages for `count` matrices (tiles,
 *     results, flags); needs no GPU; 0 for a shape that is not supported.
 * NULL pointers, count < 0, rows < 1 and N outside [1, 16] are FFK_EINVAL before anything touches the device;
 * count == 0 succeeds and does nothing.                                                                         */
size_t ffk_expm_real_batch_workspace_bytes(long count, int rows, int N);
int ffk_expm_real_batch_dev(const double* tiles, long count, int rows, int N, double* result, int32_t* not_finite,
                            void* stream);
int ffk_expm_real_batch(const double* tiles, long count, int rows, int N, double* result, int32_t* not_finite);

/* ---- superoperator.liouville_representation (superoperator.py:51-84 + Basis.expand
 *      basis.py:350-371, 650-698) --------------------------------------------------------
 * U (batch, d, d) c128, basis (N, d, d) c128 -> liouville (batch, N, N):
 * L_ij = tr(U^dag C_i U C_j), written as f64 (real part) if `hermitian_basis` != 0 (the
 * reference casts to real iff basis.isherm), else c128.                                     */
int ffk_liouville(const double* U, int batch, int d, const double* basis, int N,
                  int hermitian_basis, double* liouville);
size_t ffk_liouville_workspace_bytes(int batch, int d, int N);
int ffk_liouville_dev(const double* U, int batch, int d, const double* basis, int N,
                      int hermitian_basis, double* liouville, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- fused path: PulseSequence.get_filter_function + infidelity in one device-resident
 *      pass (pulse_sequence.py:577-586, 588-636, 691-902 and numeric.py:2062-2334) ---------
 * hamiltonian (G, d, d) c128 (lower triangle), dt (G,), omega (W,), basis (N, d, d),
 * n_opers (A, d, d), n_coeffs (A, G); spectrum/idx/s_ndim as in ffk_infidelity (spectrum
 * may be NULL: no infidelity).  Outputs (any may be NULL): eigvals, eigvecs, propagators,
 * control_matrix (A, N, W), filter_function (A, A, W), infid.
 * `t` is formed on the host by the caller (t = [0, cumsum(dt)]) exactly like the reference
 * (pulse_sequence.py:534) so the phase arguments omega*t_g round identically.               */
size_t ffk_pipeline_workspace_bytes(int W, int N, int A, int G, int d, int n_idx, int s_ndim);
int ffk_pipeline_dev(const double* hamiltonian, const double* dt, const double* t, int G, int d,
                     const double* omega, int W, const double* basis, int N,
                     const double* n_opers, int A, const double* n_coeffs,
                     const double* spectrum, int s_ndim, const int32_t* idx, int n_idx,
                     double* eigvals, double* eigvecs, double* propagators,
                     double* control_matrix, double* filter_function, double* infid,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Number of segments whose eigensolver iteration did not converge (or met NaN/Inf) in the last
 * ffk_diagonalize_dev / ffk_pipeline_dev run that used `workspace`, written to the device integer
 * `n_failed` on `stream`: the device-resident counterpart of the FFK_ENOCONV return of
 * ffk_diagonalize (numpy.linalg.LinAlgError of numeric.py:1919).                               */
int ffk_eigensolver_status_dev(const void* workspace, size_t workspace_bytes, int G, int d,
                               int32_t* n_failed, void* stream);

/* ---- batched path: P pulses of one shape (d, G, n_cops, A, N) in ONE pass, the pulse a grid axis of every stage
 *      (ff.get_filter_functions / ff.infidelities) -----------------------------------------------------------
 * Per pulse, pulse-major: c_opers (P, n_cops, d, d) c128, c_coeffs (P, n_cops, G), dt (P, G), t (P, G+1) -- formed
 * on the host per pulse exactly as for ffk_pipeline_dev --, n_opers (P, A, d, d), n_coeffs (P, A, G).  Shared by
 * all pulses: omega (W,), basis (N, d, d), spectrum / s_ndim / idx as in ffk_pipeline_dev (may be NULL).  Outputs
 * carry a leading P axis, any may be NULL: eigvals (P, G, d), eigvecs (P, G, d, d), propagators (P, G+1, d, d),
 * control_matrix (P, A, N, W), filter_function (P, A, A, W), infid (P, n_idx[, n_idx]).  1 <= P <= 65535.
 * Where the fused front applies (G <= 1024 for d <= 8, G <= 512 for d <= 16) and A N is small enough for the
 * expansion kernel that also forms F (A (N + d^2) 256 B of LDS <= 128 KiB), each stage is one launch for all P
 * pulses and the accumulate launch is the single-pulse kernel of the dimension over the P G segments laid end to
 * end.  Every other shape with 2 <= d <= 16 runs P single passes of ffk_pipeline_dev on `stream` inside the call
 * (same results; the integral is still one launch).                                                          */
size_t ffk_pipeline_batch_workspace_bytes(int P, int W, int N, int A, int G, int d, int n_idx, int s_ndim);
int ffk_pipeline_batch_dev(int P, const double* c_opers, int n_cops, const double* c_coeffs, const double* dt,
                           const double* t, int G, int d, const double* omega, int W, const double* basis, int N,
                           const double* n_opers, int A, const double* n_coeffs, const double* spectrum, int s_ndim,
                           const int32_t* idx, int n_idx, double* eigvals, double* eigvecs, double* propagators,
                           double* control_matrix, double* filter_function, double* infid, void* workspace,
                           size_t workspace_bytes, void* stream);
/* n_failed (P,) int32 on the device: flagged segments per pulse of the last ffk_pipeline_batch_dev run that used
 * `workspace` (every word written).                                                                            */
int ffk_eigensolver_status_batch_dev(const void* workspace, size_t workspace_bytes, int P, int G, int d,
                                     int32_t* n_failed, void* stream);

/* ---- batched gradient: P pulses of one shape (d, G, A, H) in ONE pass (ff.infidelity_derivatives /
 *      ff.filter_function_derivatives) --------------------------------------------------------------------------
 * ffk_filter_function_derivative for P pulses at once, 2 <= d <= 4, A <= 4, H <= 8, 1 <= P <= 65535.  Every per-pulse
 * array is pulse-major with a leading axis P: eigvals (P, G, d), eigvecs (P, G, d, d), propagators (P, G+1, d, d),
 * n_opers (P, A, d, d), n_coeffs (P, A, G), c_opers (P, H, d, d), n_coeffs_ratio (P, A, H, G) or NULL, dt (P, G),
 * t (P, G+1).  Shared by all pulses: omega (W,) and spectrum (W,) or (A, W) c128 (s_ndim 1, 2).  Outputs, either may
 * be NULL but not both: filter_function_derivative (P, A, G, H, W) f64, infidelity_derivative (P, A, G, H) f64.
 * The inputs cross in one copy from a pinned staging block, the results in one copy per requested output, nothing
 * synchronises in between, and the number of launches and copies does not depend on P.  The running sums of the
 * interaction-picture noise operators (G, A, d, d, W per pulse on the single path) are never formed: the pass keeps
 * the sums of chunks of L = ffk_batch_filter_function_derivative_chunk(G, d, W) segments, ceil(G/L) <= 16 per pulse,
 * and the gradient kernel rebuilds the running sum in registers as it walks a chunk.  L depends on the shape only,
 * never on P: a pulse's result is the same bits in every batch.  With only the infidelity derivative requested the
 * filter-function derivative is never stored either.
 * The two queries run without a GPU.  ..._workspace_bytes: device bytes of a pass (exactly linear in P; 0 for a
 * shape the pass does not take); the call reserves them in the library's arena itself.                           */
size_t ffk_batch_filter_function_derivative_workspace_bytes(int P, int W, int A, int H, int G, int d, int want_dF);
int ffk_batch_filter_function_derivative_chunk(int G, int d, int W);
int ffk_batch_filter_function_derivative(int P, const double* eigvals, const double* eigvecs,
                                         const double* propagators, const double* omega, int W,
                                         const double* n_opers, int A, const double* n_coeffs,
                                         const double* c_opers, int H, const double* n_coeffs_ratio,
                                         const double* dt, const double* t, int G, int d, const double* spectrum,
                                         int s_ndim, double* filter_function_derivative,
                                         double* infidelity_derivative);

/* ---- sequence gradient: P gate sequences, index arrays into ONE gate set, in ONE pass
 *      (ff.sequence_infidelity_derivatives / ff.sequence_filter_function_derivatives / ff.gate_infidelity_derivatives)
 * The derivatives of the filter function / infidelity of the concatenated sequences by the amplitudes of every
 * segment that stands in them, 2 <= d <= 4, A <= 4, H <= 8, T, P, Gmax <= 65535.  The gate set: T gates with the same
 * noise operators n_opers (A, d, d) and control operators c_opers (H, d, d), gate k with gate_segments[k] <= Gmax
 * segments, every per-gate array gate-major and padded to Gmax segments of ZERO duration: eigvals (T, Gmax, d) (0),
 * eigvecs (T, Gmax, d, d) (identity), propagators (T, Gmax + 1, d, d) (the last one repeated: row Gmax is the gate's
 * total propagator), n_coeffs (T, A, Gmax) (0), dt (T, Gmax) (0).  The sequences in CSR form: offsets (P + 1) int32
 * from 0, strictly increasing, index (offsets[P]) int32 in [0, T).  omega (W,), spectrum (W,) or (A, W) c128
 * (s_ndim 1, 2).  Sequence p has G_p = sum of gate_segments over its positions segments, and S_p = sum of G_q, q < p,
 * stand before it.  Outputs, any may be NULL but not all:
 *   filter_function_derivative  sequence p at S_p A H W doubles: (A, G_p, H, W)
 *   infidelity_derivative       sequence p at S_p A H doubles: (A, G_p, H)
 *   gate_infidelity_derivative  (T, A, Gmax, H), IN and out: to what entry [k] holds the call adds, over the occurrences
 *                               of gate k -- occ_offsets (T + 1) int32, then per occurrence occ_sequence and
 *                               occ_position, int32, every position named once under its gate --, one after the other
 *                               in list order, weights[p] times the position's (A, G_k, H) slice of sequence p's
 *                               infidelity derivative (consecutive passes thus give one sequential sum); rows past
 *                               gate_segments[k] are kept.  One thread per entry, no atomics; the sequences'
 *                               derivatives stay on the device.
 * The kernels work in the frame of the current position, in which one record per gate segment serves every position
 * and sequence (csrc/sequence_gradient.hip); nothing of the size of a sequence is formed, and with only infidelity
 * derivatives requested the filter-function derivative is never stored.  One H2D copy from a pinned staging block, a
 * fixed number of launches whatever P, one D2H copy per requested output.  A sequence's result is the same bits
 * whatever else is in the pass.  Bad arguments (an index outside [0, T), an empty sequence, W < 1, s_ndim not 1 or 2
 * with an infidelity output, ...) return FFK_EINVAL before anything touches the device.
 * ..._workspace_bytes runs without a GPU: device bytes of a pass over n_index positions and n_segments walked
 * segments in all (exactly linear in n_segments, an upper bound; 0 for a shape the pass does not take); the call
 * reserves them in the library's arena itself.                                                                  */
size_t ffk_sequence_infidelity_derivatives_workspace_bytes(int T, int Gmax, int P, long long n_index,
                                                           long long n_segments, int W, int A, int H, int d,
                                                           int want_dF);
int ffk_sequence_infidelity_derivatives(int T, int Gmax, const int32_t* gate_segments, const double* eigvals,
                                        const double* eigvecs, const double* propagators, const double* n_opers,
                                        int A, const double* n_coeffs, const double* c_opers, int H, const double* dt,
                                        int d, const int32_t* offsets, const int32_t* index, int P,
                                        const double* omega, int W, const double* spectrum, int s_ndim,
                                        const int32_t* occ_offsets, const int32_t* occ_sequence,
                                        const int32_t* occ_position, const double* weights,
                                        double* filter_function_derivative, double* infidelity_derivative,
                                        double* gate_infidelity_derivative);

/* ffk_frequency_shifts_from_scratch for P pulses of one shape at once, 1 <= P <= 65535, without the second-order
 * filter function in memory.  Per-pulse arrays are pulse-major with a leading axis P, as in
 * ffk_batch_filter_function_derivative; omega (W,), basis (N, d, d), spectrum ((W,), (n_idx, W) or (n_idx, n_idx, W)
 * c128) and idx (n_idx distinct noise operators) are shared.  frequency_shifts (P, n_idx, N, N) f64, or
 * (P, n_idx, n_idx, N, N) for s_ndim 3.  Shapes: those for which the single pass runs its matrix-core kernel (a square
 * wave tile whose operands fit in LDS twice per CU); others are refused, ..._workspace_bytes and ..._chunk return 0.
 * The pass runs that kernel's segment loop and integrates each frequency's accumulators against the weighted
 * spectrum in its epilogue; only the tiles of the (A N) x (A N) output that hold a selected operator pair are
 * launched.  A block walks ffk_batch_frequency_shifts_chunk(W, N, A, G, d) frequencies and writes one partial; a
 * second kernel adds a pulse's partials in ascending order, without atomics.  The chunk depends on the shape only,
 * never on P: a pulse's result is the same bits in every batch and at every slot.  Every input array crosses in one
 * copy, the result in one copy, nothing synchronises in between, and the number of launches and copies does not
 * depend on P.  The two queries run without a GPU; ..._workspace_bytes is exactly linear in P.                    */
size_t ffk_batch_frequency_shifts_workspace_bytes(int P, int W, int N, int A, int G, int d, int n_idx, int s_ndim);
int ffk_batch_frequency_shifts_chunk(int W, int N, int A, int G, int d);
int ffk_batch_frequency_shifts(int P, const double* eigvals, const double* eigvecs, const double* propagators,
                               const double* omega, int W, const double* basis, int N, const double* n_opers, int A,
                               const double* n_coeffs, const double* dt, const double* t, int G, int d,
                               const double* spectrum, int s_ndim, const int32_t* idx, int n_idx,
                               double* frequency_shifts);

/* Fault word of the kernels whose wavefronts hand tiles to one another through flags in LDS (the d = 4
 * accumulation behind ffk_control_matrix*, ffk_pipeline_dev and the resident passes; reference loop
 * numeric.py:846-869).  Their waits are bounded; a wait that runs out stores a non-zero code in a word of mapped
 * host memory that the launcher hands the kernel as an ARGUMENT (so it is right on whichever device the launch goes
 * to), and the launch's results are invalid.  ONE WORD PER HOST THREAD: a thread sees the faults of the launches it
 * enqueued itself, and only those (a captured graph reports to the thread that captured it).  The host-pointer
 * entry points read the calling thread's word after their own synchronisation and return FFK_EKERNEL; a fault that
 * an EARLIER, never checked asynchronous launch of the thread left behind is reported by them on entry, as such,
 * before anything runs.  Callers of the `_dev` flavour call this AFTER synchronising the stream, on the thread that
 * enqueued: *word = 0 means every launch of this thread since the last clearing was sound.  Sticky until read with
 * clear != 0.                                                                                                    */
int ffk_kernel_fault_status(int32_t* word, int clear);

/* ---- resident evaluation: the user-facing call PulseSequence.get_filter_function(omega)
 *      followed by ff.infidelity(pulse, S, omega) (pulse_sequence.py:691-805, 577-677;
 *      numeric.py:2062-2334) on host arrays with the minimum of PCIe traffic ------------------
 * ffk_resident_filter_function stages all inputs (same arrays as ffk_pipeline_dev, host pointers)
 * through one pinned block with ONE H2D copy, runs the fused pass, and returns the small results
 * -- eigvals (G, d), eigvecs (G, d, d), propagators (G+1, d, d), filter_function (A, A, W) -- by ONE
 * D2H copy as pointers into pinned host memory owned by the handle (valid until the handle runs
 * another pass or is destroyed; the binding wraps them as arrays without copying).  The control
 * matrix (A, N, W) -- 5x the bytes of F at config 2 -- stays in HBM and is fetched only when the
 * caller asks for it (ffk_resident_control_matrix), which is what the reference's cache
 * (`pulse._frequency_data['control_matrix']`) needs it for.  ffk_resident_infidelity integrates
 * the resident F against a host spectrum ((W,), (n_idx, W) or (n_idx, n_idx, W); real f64 if
 * spectrum_is_real, else c128) on the resident frequency grid, normalised by 1/(2 pi d) with the
 * caller's d (pulse.d, which a user may override: tests/test_precision.py:300).  Returns FFK_ENOCONV like
 * ffk_diagonalize.  Device and pinned blocks come from grow-only pools
 * (ffk_resident_release_pools frees what is idle).                                             */
typedef struct ffk_resident ffk_resident;
int ffk_resident_create(ffk_resident** handle);
int ffk_resident_destroy(ffk_resident* handle);
int ffk_resident_release_pools(void);
int ffk_resident_filter_function(ffk_resident* handle, const double* hamiltonian, const double* dt,
                                 const double* t, int G, int d, const double* omega, int W,
                                 const double* basis, int N, const double* n_opers, int A,
                                 const double* n_coeffs, double** eigvals, double** eigvecs,
                                 double** propagators, double** filter_function);
/* The same pass with the control Hamiltonian given as PulseSequence holds it -- c_opers
 * (n_cops, d, d) c128 and c_coeffs (n_cops, G) f64 -- instead of the summed (G, d, d) array of
 * numeric.diagonalize (pulse_sequence.py:1300-1302, einsum 'ijk,il->ljk'): the sum runs on the
 * device, 8 n_cops bytes per segment cross PCIe instead of 16 d^2.                               */
int ffk_resident_filter_function_from_controls(ffk_resident* handle, const double* c_opers, int n_cops,
                                               const double* c_coeffs, const double* dt,
                                               const double* t, int G, int d, const double* omega,
                                               int W, const double* basis, int N,
                                               const double* n_opers, int A, const double* n_coeffs,
                                               double** eigvals, double** eigvecs,
                                               double** propagators, double** filter_function);
/* The same pass with the infidelity integral of numeric.infidelity (numeric.py:2063-2334, `which='total'`,
 * traceless basis) riding in it: `ff.infidelity(pulse, S, omega)` on a pulse with nothing cached is one
 * round trip to the device instead of two.  spectrum: (W,), (n_idx, W) or (n_idx, n_idx, W), f64 if
 * spectrum_is_real else c128, already validated (util.parse_spectrum, util.py:214-227); idx: the noise
 * operators' indices; d_infidelity: the dimension in 1/(2 pi d); infidelity: (n_idx,) resp. (n_idx, n_idx). */
int ffk_resident_filter_function_infidelity(ffk_resident* handle, const double* c_opers, int n_cops,
                                            const double* c_coeffs, const double* dt, const double* t,
                                            int G, int d, const double* omega, int W, const double* basis,
                                            int N, const double* n_opers, int A, const double* n_coeffs,
                                            const double* spectrum, int s_ndim, int spectrum_is_real,
                                            const int32_t* idx, int n_idx, int d_infidelity,
                                            double** eigvals, double** eigvecs, double** propagators,
                                            double** filter_function, double* infidelity);
/* host-clock seconds of the last pass: [0] packing the inputs into the pinned block, [1] enqueueing
 * the H2D copy, the kernels and the D2H copy, [2] waiting for the stream                         */
int ffk_resident_timing(ffk_resident* handle, double* seconds);
int ffk_resident_control_matrix(ffk_resident* handle, double* control_matrix);
/* device pointers of the resident control matrix, filter function and frequencies (any may be NULL) */
int ffk_resident_control_matrix_dev(ffk_resident* handle, const double** control_matrix,
                                    const double** filter_function, const double** omega);
int ffk_resident_infidelity(ffk_resident* handle, const double* spectrum, int s_ndim,
                            int spectrum_is_real, const int32_t* idx, int n_idx, int d,
                            double* infid);
/* The batch counterpart of ffk_resident_filter_function_infidelity: P pulses (arrays as for ffk_pipeline_batch_dev,
 * host pointers) staged with ONE H2D copy, one batched pass, ONE D2H copy of eigvals (P, G, d), eigvecs, propagators
 * and filter_function (P, A, A, W) into the handle's pinned block.  spectrum may be NULL (no integral); else it is
 * shared by all pulses as in ffk_resident_filter_function_infidelity and infidelity is (P, n_idx[, n_idx]).
 * n_failed (P,) int32 host: flagged segments per pulse; any non-zero entry returns FFK_ENOCONV naming the first such
 * pulse, and the results are then not valid.  The control matrices (P, A, N, W) stay in HBM:
 * ffk_resident_batch_control_matrix copies pulse `pulse`'s (A, N, W) out.                                      */
int ffk_resident_batch_filter_function_infidelity(ffk_resident* handle, int P, const double* c_opers, int n_cops,
                                                  const double* c_coeffs, const double* dt, const double* t, int G,
                                                  int d, const double* omega, int W, const double* basis, int N,
                                                  const double* n_opers, int A, const double* n_coeffs,
                                                  const double* spectrum, int s_ndim, int spectrum_is_real,
                                                  const int32_t* idx, int n_idx, int d_infidelity, double** eigvals,
                                                  double** eigvecs, double** propagators, double** filter_function,
                                                  double* infidelity, int32_t* n_failed);
int ffk_resident_batch_control_matrix(ffk_resident* handle, int pulse, double* control_matrix);

/* ---- many gate sequences from one table of distinct gates in ONE pass (ff.concatenate_sequences) ----
 * P sequences as a CSR list: offsets (P + 1) int32 host, offsets[0] = 0 and strictly increasing, index
 * (offsets[P]) int32 host, each entry in [0, T).  The T gates: gates[k] an ffk_resident* whose control matrix
 * (A, N, W) is read in place -- slots[k] < 0 for a single resident result, slots[k] >= 0 for member slots[k] of a
 * batched or sequence pass -- or NULL: the gate's control matrix is the next row of gate_table (n_host, A, N, W)
 * c128 host, in gate order.  gate_propagators (T, d, d) c128 and tau (T,) f64 host: the gates' total propagators
 * and durations; omega (W,) f64, basis (N, d, d) c128.  Supported: d = 2, N = 4, 1 <= A <= 4, Hermitian basis.
 * Results stay in `result` (not one of the gates): the control matrices (P, A, N, W) in HBM
 * (ffk_resident_batch_control_matrix copies member p's out), the filter functions (P, A, A, W) in HBM and in
 * pinned host memory (*filter_function points there until the handle is reused or destroyed); the total
 * propagators (P, d, d) c128 go to the caller's array.  Optional (spectrum != NULL): the infidelities (P, n_idx
 * [, n_idx]) of every sequence on a shared spectrum, as in ffk_resident_batch_filter_function_infidelity.
 * A sequence's results do not depend on the other sequences of the pass.  Bad arguments: FFK_EINVAL. */
size_t ffk_concatenate_sequences_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A, int N, int W,
                                                 int n_idx, int s_ndim);
int ffk_concatenate_sequences_resident(ffk_resident* result, ffk_resident* const* gates, const int32_t* slots,
                                       const double* gate_table, const double* gate_propagators, const double* tau,
                                       int T, const int32_t* offsets, const int32_t* index, int P,
                                       const double* omega, int W, const double* basis, int hermitian_basis, int d,
                                       int A, int N, const double* spectrum, int s_ndim, int spectrum_is_real,
                                       const int32_t* idx, int n_idx, int d_infidelity, double* total_propagators,
                                       double** filter_function, double* infidelity);
/* The infidelities (n_members, n_idx[, n_idx]) of members (n_members,) int32 of a batched or sequence pass on their
 * resident filter functions, ONE launch of the pulse-axis integral; spectrum, idx and d as in
 * ffk_resident_infidelity.  Needs W >= 2 and n_members <= 65535. */
int ffk_resident_batch_infidelity(ffk_resident* handle, const int32_t* members, int n_members, const double* spectrum,
                                  int s_ndim, int spectrum_is_real, const int32_t* idx, int n_idx, int d,
                                  double* infidelity);

/* ---- pulse-correlation infidelities of many gate sequences in ONE pass (ff.correlation_infidelities) ----
 * I[g, h, a] of sequence p, the contribution of its gate pair (g, h) to its infidelity on noise operator idx[a]:
 * (1 / 2 pi d_infidelity) times the trapezoid integral of S_a(w) Re sum_k conj(X_g[a, k, w]) X_h[a, k, w] over the
 * summands X_g = e^{i w t_{g-1}} v_{k_g} Q^{(g-1)} of the concatenation rule.  Sequences, gates, gate_table,
 * gate_propagators, tau, omega and basis as for ffk_concatenate_sequences_resident (d = 2, N = 4, 1 <= A <= 4,
 * Hermitian basis); every sequence has 1 ... 256 positions.  spectrum (W,) (s_ndim = 1) or (n_idx, W) (s_ndim = 2),
 * f64 if spectrum_is_real, else c128 with a zero imaginary part; cross-spectra (s_ndim = 3) are FFK_EINVAL.  idx
 * (n_idx,) int32 in [0, A); W >= 2.  out_offsets (P + 1) int64 host: the prefix sums of G_p^2; infidelity
 * (out_offsets[P], n_idx) f64 host: sequence p's (G_p, G_p, n_idx) array starts at row out_offsets[p].  There is no
 * result handle: one H2D copy, five to eight launches whatever P (one Gram launch per class of lengths that has
 * members: up to 32, 64, 128, 256 positions), one D2H copy.  Neither the summands nor the pulse-correlation filter function (G, G, A, A, W) are formed: each
 * block generates the summands of a few frequencies in LDS and accumulates the real Gram matrix of the positions on
 * the FP64 matrix cores; the frequency axis is cut into slabs that depend on W alone and are added in index order,
 * the lower triangle is the mirror of the upper.  A sequence's result is the same bits whatever else is in the pass.
 * The workspace query needs no GPU; it bounds the arena bytes of any lengths (0: unsupported shape).  Bad arguments:
 * FFK_EINVAL before anything touches the device. */
size_t ffk_sequence_correlation_infidelities_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A,
                                                             int N, int W, int n_idx, int s_ndim);
int ffk_sequence_correlation_infidelities(ffk_resident* const* gates, const int32_t* slots, const double* gate_table,
                                          const double* gate_propagators, const double* tau, int T,
                                          const int32_t* offsets, const int32_t* index, int P, const double* omega,
                                          int W, const double* basis, int hermitian_basis, int d, int A, int N,
                                          const double* spectrum, int s_ndim, int spectrum_is_real, const int32_t* idx,
                                          int n_idx, int d_infidelity, const int64_t* out_offsets, double* infidelity);

/* ---- the same for two-qubit gates (ff.sequence_correlation_infidelities) ----
 * ffk_sequence_correlation_infidelities for (d, N) = (4, 16), 1 <= A <= 4, Hermitian basis: the same arguments and
 * conventions -- CSR offsets / index, every sequence 1 ... 256 positions, out_offsets the prefix sums of G_p^2, the
 * ragged (out_offsets[P], n_idx) output, spectra of one or two dimensions without an imaginary part, W >= 2 --, arena
 * workspace, one H2D copy, one D2H copy, no result handle, five to eight launches whatever P: phases, Liouville
 * representations (T, 16, 16) and total propagators; the propagator accumulated before every position, (n_index, 16,
 * 16) f64, one block per sequence; the spectral weights; one Gram launch per class of lengths that has members (up
 * to 32, 64, 128, 256 positions); the slab reduction.  A Gram block generates the summands of 8, 4, 2 or 1
 * frequencies in LDS with vector FMAs and accumulates the real Gram matrix of the positions on the FP64 matrix
 * cores, eight K-steps per tile pair and frequency.  A sequence's result is the same bits whatever else is in the
 * pass, and exactly symmetric.  Any other (d, N), the single-qubit shape included, is FFK_EINVAL here and 0 from the
 * workspace query, which needs no GPU.  Bad arguments: FFK_EINVAL before anything touches the device. */
size_t ffk_sequence_correlation_infidelities4_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A,
                                                              int N, int W, int n_idx, int s_ndim);
int ffk_sequence_correlation_infidelities4(ffk_resident* const* gates, const int32_t* slots, const double* gate_table,
                                           const double* gate_propagators, const double* tau, int T,
                                           const int32_t* offsets, const int32_t* index, int P, const double* omega,
                                           int W, const double* basis, int hermitian_basis, int d, int A, int N,
                                           const double* spectrum, int s_ndim, int spectrum_is_real, const int32_t* idx,
                                           int n_idx, int d_infidelity, const int64_t* out_offsets,
                                           double* infidelity);

/* ---- infidelities of many gate sequences from one gate set in ONE pass (ff.sequence_infidelities) ----
 * infidelity (P, n_idx) f64 host, or (P, n_idx, n_idx) for s_ndim = 3: what ffk_concatenate_sequences_resident
 * returns as `infidelity`, without a result handle and without the sequences' control matrices, which this entry
 * never writes to memory; the filter functions (P, A, A, W) exist in the arena workspace only.  Sequences, gates,
 * slots, gate_table, gate_propagators, tau, omega, basis, spectrum, idx and d_infidelity as there (Hermitian basis;
 * with a spectrum W >= 2 and P <= 65535).  Supported: (d, N) = (2, 4) and (4, 16), 1 <= A <= 4.  Optional outputs, each
 * may be NULL: total_propagators (P, d, d) c128 host, filter_function (P, A, A, W) c128 host (owned by the caller);
 * spectrum may be NULL if one of them is asked for (infidelity is then not written).  One H2D copy, three launches
 * whatever P -- phases, Liouville propagators and total propagators; the rule with the filter function; the
 * integral --, one D2H copy.  d = 2 runs the kernels and the arithmetic of ffk_concatenate_sequences_resident; d = 4
 * runs the 16 x 16 product of the recurrence on the FP64 matrix cores.  A sequence's result is the same bits
 * whatever else is in the pass and whatever its place.  The workspace query needs no GPU (0: unsupported shape; s_ndim
 * = 0: no spectrum).  Bad arguments: FFK_EINVAL before anything touches the device. */
size_t ffk_sequence_infidelities_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A, int N, int W,
                                                 int n_idx, int s_ndim);
int ffk_sequence_infidelities(ffk_resident* const* gates, const int32_t* slots, const double* gate_table,
                              const double* gate_propagators, const double* tau, int T, const int32_t* offsets,
                              const int32_t* index, int P, const double* omega, int W, const double* basis,
                              int hermitian_basis, int d, int A, int N, const double* spectrum, int s_ndim,
                              int spectrum_is_real, const int32_t* idx, int n_idx, int d_infidelity,
                              double* infidelity, double* total_propagators, double* filter_function);

/* ---- decay amplitudes, cumulant functions and error transfer matrices of P independent pulses in ONE pass
 *      (ff.decay_amplitudes, ff.cumulant_functions, ff.error_transfer_matrices) ----
 * The control matrix (A, N, W) of pulse p is read in place: pulses[p] an ffk_resident* with slots[p] < 0 for a
 * single resident result, slots[p] >= 0 for member slots[p] of a batched or sequence pass -- or NULL: the next row
 * of control_matrices (n_host, A, N, W) c128 host, in pulse order (may be NULL if no pulse is NULL).  omega (W,)
 * f64, basis (N, d, d) c128, spectrum c128 (W,), (n_idx, W) or (n_idx, n_idx, W) and idx (n_idx,) int32 as for
 * ffk_decay_amplitudes, all host.  Supported: N <= 16, N <= d^2, 2 <= d <= FFK_MAX_D_TEMPLATED, 1 <= P <= 65535
 * (and P * pairs <= 65535 cumulant functions unless single_qubit; pairs = n_idx, or n_idx^2 for s_ndim = 3).
 * Outputs, host, each may be NULL (only the stages a requested output needs are run): decay_amplitudes and
 * cumulant_function (P, n_idx[, n_idx], N, N) f64 -- a pulse's values are those of ffk_decay_amplitudes with
 * n_pulses = 1 up to the order of the sum over the frequencies, and of ffk_cumulant_function (single_qubit as
 * there) --, error_transfer_matrix (P, N, N) f64 = exp of the cumulant function summed over the noise operators,
 * with the arithmetic of ffk_expm_real and the number of squarings chosen on the device.  not_finite (P,) int32
 * (required with error_transfer_matrix): 1 where that sum holds a NaN or Inf; the pulse's error transfer matrix
 * is then not written.  A pulse's results do not depend on the other pulses of the pass.  One H2D copy of the small
 * inputs and the host rows, one D2H copy of the requested outputs, no synchronisation in between.  Bad
 * arguments: FFK_EINVAL.  The query returns the device bytes a pass with all three outputs holds (0: unsupported). */
size_t ffk_resident_batch_processes_workspace_bytes(int P, int n_host, int A, int N, int W, int d, int n_idx,
                                                    int s_ndim);
int ffk_resident_batch_processes(ffk_resident* const* pulses, const int32_t* slots, const double* control_matrices,
                                 int P, int A, int N, int W, int d, const double* omega, const double* basis,
                                 int single_qubit, const double* spectrum, int s_ndim, const int32_t* idx, int n_idx,
                                 double* decay_amplitudes, double* cumulant_function, double* error_transfer_matrix,
                                 int32_t* not_finite);

/* ---- periodic driving: P pulses at K repeat counts in ONE pass (ff.periodic_filter_functions,
 *      ff.periodic_infidelities, ff.periodic_decay_amplitudes) ----
 * Pulse p is one period: its control matrix (A, N = d^2, W) on the grid omega (W,), the eigensystem of its total
 * propagator U = V diag(e^{i phi}) V^dag -- eigvecs (P, d, d) c128 with UNITARY V also where phases coincide,
 * phase_differences (P, d, d, 2) f64: phi_j - phi_k as an unevaluated sum hi + lo of two doubles (lo may be 0) -- and
 * its duration periods (P,) f64.  basis (N, d, d) c128: complete, orthonormal, Hermitian.  repeats
 * (K,) int32 >= 1 is shared by all pulses.  In U's eigenbasis the control matrix of n periods is that of one period
 * times sum_{g<n} e^{i g theta_jk}, theta_jk = fl(omega T) - (phi_j - phi_k): the repeat count enters as the argument
 * of a sine, evaluated as sin(n theta/2)/sin(theta/2) on the angle reduced to [-pi, pi] (n where the sine vanishes).
 * stage selects `out`: 1 the fidelity filter functions' diagonal (P, K, n_idx, W) f64 (no spectrum needed), 2 the
 * infidelities (P, K, n_idx) f64 = sum_w weight(w) F(w) / d_infidelity, 3 the decay amplitudes (P, K, n_idx, N, N)
 * f64, symmetric bit for bit.  spectrum c128 (W,) for s_ndim = 1 or (n_idx, W) for s_ndim = 2 (its real part is
 * used; cross-spectra are not taken), idx (n_idx,) int32 the selected noise operators, W >= 2 at stage 2 and 3.
 * A result does not depend on what else is in the pass, nor on its place in it.  One launch per stage (two with
 * the weights) whatever P and K.  Supported: 2 <= d <= 4, 1 <= P, K <= 65535, 1 <= n_idx <= A.
 *   ffk_periodic_dev: device pointers (control_matrices: P device pointers in device memory); launches only.
 *     workspace: 16 * rows * W bytes (rows = 1 or n_idx) at stage 2 and 3, none at stage 1.
 *   ffk_resident_periodic: host pointers; pulses[p] an ffk_resident* with slots[p] as for
 *     ffk_resident_batch_processes, or NULL: the next row of control_matrices (n_host, A, N, W) c128 host.  One
 *     staged call through the arena: the inputs up, the kernels, `out` back.  Bad arguments (a repeat count below 1
 *     among them): FFK_EINVAL before anything touches the device.
 *   ffk_periodic_workspace_bytes: the device bytes that call stages (0: unsupported shape). */
size_t ffk_periodic_workspace_bytes(int P, int K, int n_host, int A, int W, int d, int n_idx, int s_ndim, int stage);
int ffk_periodic_dev(const void* const* control_matrices, int P, int A, int W, int d, const double* omega,
                     const double* basis, const double* eigvecs, const double* phase_differences, const double* periods,
                     const int32_t* repeats, int K, const double* spectrum, int s_ndim, const int32_t* idx,
                     int n_idx, int d_infidelity, int stage, double* out, void* workspace, size_t workspace_bytes,
                     void* stream);
int ffk_resident_periodic(ffk_resident* const* pulses, const int32_t* slots, const double* control_matrices, int P,
                          int A, int W, int d, const double* omega, const double* basis, const double* eigvecs,
                          const double* phase_differences, const double* periods, const int32_t* repeats, int K,
                          const double* spectrum, int s_ndim, const int32_t* idx, int n_idx, int d_infidelity,
                          int stage, double* out);

/* ---- periodic driving, second order: the frequency shifts of P pulses at K repeat counts in ONE pass
 *      (ff.periodic_frequency_shifts) ----
 * Pulses, eigensystems, periods, basis, omega, spectrum, idx, handles and slots as for ffk_resident_periodic (W >= 2,
 * s_ndim 1 or 2).  The counts are reached by period doubling: with Q_m the Liouville matrix of U^m and R_n the
 * control matrix of n periods,
 *     Delta_{m+m'} = Delta_m + Q_m^T Delta_{m'} Q_m + X(m, m'),
 *     X(m, m')[k,l] = sum_w weight(w) Re( conj( e^{i w m T} (R_{m'} Q_m)[k,w] ) R_m[l,w] ),
 * both operands element-wise in U's eigenbasis (sines of m theta/2 and m' theta/2 over sin(theta/2), and the phase
 * e^{i m theta}).  steps (S, 4) int32 is the plan: per step (m, m', slot of Delta_m, slot of Delta_m'); the result of
 * step s lies in slot s + 1 and slot 0 is delta1 (P, n_idx, N, N) f64, the pulses' own frequency shifts; a step reads
 * slots <= s only.  count_slots (K,) int32 names the slot of each row of out (P, K, n_idx, N, N) f64.  With S = 0
 * (steps may be NULL) every row is delta1 bit for bit.  A result depends on its own steps alone, not on what else is
 * in the pass.  At most three launches whatever P, K and S: the weights, X of every step (grid: operator, step,
 * pulse; d = 4 on the FP64 matrix cores), the serial walk (grid: operator, pulse).  Supported: 2 <= d <= 4,
 * 1 <= P, K <= 65535, 0 <= S <= 65535, 1 <= n_idx <= A.
 *   ffk_periodic_shifts_dev: device pointers; launches only.  workspace: align256(16 rows W) + align256(t S) +
 *     align256(t (S + 1)) bytes with rows = 1 or n_idx and t = 8 P n_idx N^2.
 *   ffk_resident_periodic_shifts: host pointers, one staged call.  Bad arguments (a step that reads a slot not yet
 *     written among them): FFK_EINVAL before anything touches the device.
 *   ffk_periodic_shifts_workspace_bytes: the device bytes that call stages (0: unsupported shape). */
size_t ffk_periodic_shifts_workspace_bytes(int P, int K, int S, int n_host, int A, int W, int d, int n_idx,
                                           int s_ndim);
int ffk_periodic_shifts_dev(const void* const* control_matrices, int P, int A, int W, int d, const double* omega,
                            const double* basis, const double* eigvecs, const double* phase_differences,
                            const double* periods, const int32_t* steps, int S, const int32_t* count_slots, int K,
                            const double* spectrum, int s_ndim, const int32_t* idx, int n_idx, const double* delta1,
                            double* out, void* workspace, size_t workspace_bytes, void* stream);
int ffk_resident_periodic_shifts(ffk_resident* const* pulses, const int32_t* slots, const double* control_matrices,
                                 int P, int A, int W, int d, const double* omega, const double* basis,
                                 const double* eigvecs, const double* phase_differences, const double* periods,
                                 const int32_t* steps, int S, const int32_t* count_slots, int K,
                                 const double* spectrum, int s_ndim, const int32_t* idx, int n_idx,
                                 const double* delta1, double* out);

/* ---- decay amplitudes, cumulant functions and error transfer matrices of many gate sequences from one gate set in
 *      ONE pass, under any number of spectra (ff.sequence_decay_amplitudes, ff.sequence_cumulant_functions,
 *      ff.sequence_error_transfer_matrices) ----
 * Sequences, gates, slots, gate_table, gate_propagators, tau, omega, basis and idx as for ffk_sequence_infidelities
 * (Hermitian basis; (d, N) = (2, 4) or (4, 16), 1 <= A <= 4; W >= 2).  spectrum (n_spectra, W) for s_ndim = 1 or
 * (n_spectra, n_idx, W) for s_ndim = 2, f64 host: real weights only, cross-spectra are not taken.  stage selects what
 * `out` receives: 1 the decay amplitudes (n_spectra, P, n_idx, N, N) f64, 2 the cumulant functions of the same shape
 * (single_qubit as for ffk_cumulant_function), 3 the error transfer matrices (n_spectra, P, N, N), the exponential of
 * the cumulant function summed over the selected operators.  not_finite (n_spectra, P) int32: at stage 3, 1 where
 * that sum holds a NaN or Inf (the matrix is then not written); 0 at the other stages.  total_propagators (P, d, d)
 * c128 host may be NULL.  The decay amplitudes are formed from the registers of the concatenation rule at the end of
 * each sequence: the sequences' control matrices are never written to memory, and every spectrum beyond the first
 * costs one more epilogue, not one more walk.  One H2D copy, a fixed number of launches whatever P and n_spectra --
 * the front, the weights, the rule with Gamma, the sum of the frequency blocks' partial tiles in block order, then
 * the cumulant functions and the exponentials as ffk_resident_batch_processes runs them --, one D2H copy.  Arena
 * workspace, no result handle.  Gamma of one operator is symmetric bit for bit, and a sequence's result is the same
 * bits whatever else is in the pass, whatever its place and however many spectra the call carries.  At stage 2 and 3
 * without single_qubit n_spectra * P * n_idx <= 65535.  Bad arguments: FFK_EINVAL before anything touches the
 * device.  The workspace query needs no GPU (0: unsupported shape). */
size_t ffk_sequence_processes_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A, int N, int W,
                                              int n_idx, int s_ndim, int n_spectra, int stage);
int ffk_sequence_processes(ffk_resident* const* gates, const int32_t* slots, const double* gate_table,
                           const double* gate_propagators, const double* tau, int T, const int32_t* offsets,
                           const int32_t* index, int P, const double* omega, int W, const double* basis,
                           int hermitian_basis, int d, int A, int N, int single_qubit, const double* spectrum,
                           int s_ndim, int n_spectra, const int32_t* idx, int n_idx, int stage, double* out,
                           int32_t* not_finite, double* total_propagators);

/* ---- frequency shifts (second order) of many gate sequences from one gate set in ONE pass, under any number of
 *      spectra (ff.sequence_frequency_shifts) ----
 * Sequences, gates, slots, gate_table, gate_propagators, tau, omega, basis, spectrum, s_ndim, n_spectra and idx as for
 * ffk_sequence_processes (Hermitian basis; (d, N) = (2, 4) or (4, 16), 1 <= A <= 4; W >= 2; real weights of one or
 * two dimensions); the operators in idx must be distinct.  gate_shifts (n_spectra, T, n_idx, N, N) f64 host: the
 * gates' own frequency shifts under each spectrum (ffk_batch_frequency_shifts, ff.frequency_shifts).  out
 * (n_spectra, P, n_idx, N, N) f64 host: the frequency shifts of the sequences, i.e. the integral of the rotated
 * concatenation rule of the second-order filter function,
 *     sum_g [ Lam_g^T gate_shifts[k_g] Lam_g + sum_w c_w S(w) Re(conj(Rs_g[k, w]) Cum_{g-1}[l, w]) ],
 * Lam_g the Liouville matrix of the propagator before position g, Rs_g the first-order rule's summand and Cum its
 * running sum.  Neither a second-order filter function nor a sequence's control matrix is written to memory.
 * not_finite (n_spectra, P) int32: 1 where a sequence's tiles under a spectrum hold a NaN or Inf.  total_propagators
 * (P, d, d) c128 host may be NULL.  One H2D copy, a fixed number of launches whatever P and n_spectra -- the front,
 * the weights, one forward walk of the sequences (two spectra share a walk, grid z carries the further pairs), the sum
 * of the frequency blocks' partial tiles in block order --, one D2H copy.  Arena workspace, no result handle.  A
 * sequence's result is the same bits whatever else is in the pass, whatever its place and however many spectra the
 * call carries; a sequence of one gate returns that gate's row of gate_shifts.  Bad arguments: FFK_EINVAL before
 * anything touches the device.  The workspace query needs no GPU (0: unsupported shape). */
size_t ffk_sequence_frequency_shifts_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A, int N, int W,
                                                     int n_idx, int s_ndim, int n_spectra);
int ffk_sequence_frequency_shifts(ffk_resident* const* gates, const int32_t* slots, const double* gate_table,
                                  const double* gate_propagators, const double* tau, int T, const int32_t* offsets,
                                  const int32_t* index, int P, const double* omega, int W, const double* basis,
                                  int hermitian_basis, int d, int A, int N, const double* spectrum, int s_ndim,
                                  int n_spectra, const int32_t* idx, int n_idx, const double* gate_shifts, double* out,
                                  int32_t* not_finite, double* total_propagators);

/* ---- infidelities or decay amplitudes of every PREFIX of many gate sequences from one gate set in ONE pass, under
 *      any number of spectra (ff.sequence_prefix_infidelities, ff.sequence_prefix_decay_amplitudes) ----
 * Sequences, gates, slots, gate_table, gate_propagators, tau, omega, basis, spectrum, s_ndim, n_spectra and idx as for
 * ffk_sequence_frequency_shifts (Hermitian basis; (d, N) = (2, 4) or (4, 16), 1 <= A <= 4; W >= 2; real weights of
 * one or two dimensions; distinct operators in idx).  closing (n_index,) int32 host or NULL: closing[offsets[p] + g]
 * is the table row, in [0, T), of the gate appended behind the first g + 1 gates of sequence p.  The result of global
 * position offsets[p] + g is that of the sequence index[offsets[p] : offsets[p] + g + 1] (with its closing gate):
 * mode 0 the infidelities, out (n_spectra, n_index, n_idx) f64 host, the trace of the decay amplitudes over d; mode 1
 * the diagonal of the decay amplitudes, out (n_spectra, n_index, n_idx, N); mode 2 the decay amplitudes, out
 * (n_spectra, n_index, n_idx, N, N).  The control matrix of a prefix is the partial sum of the concatenation rule,
 * which a forward walk holds in registers at every position: each sequence is walked once, G positions instead of
 * the G (G + 1) / 2 of its prefixes taken as sequences, with one epilogue per position.  One H2D copy, four launches
 * whatever P, n_index and n_spectra -- the front, the weights, the walk (two spectra share a walk, grid z carries the
 * further pairs), the sum of the frequency blocks' partial results in block order --, one D2H copy.  Arena workspace,
 * no result handle.  A position's result is the same bits whatever else is in the pass, whatever lies behind it in
 * its sequence and however many spectra the call carries; decay amplitudes are symmetric bit for bit.  Bad arguments
 * (a closing entry outside [0, T) among them): FFK_EINVAL before anything touches the device.  The workspace query
 * needs no GPU (0: unsupported shape). */
size_t ffk_sequence_prefix_processes_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A, int N, int W,
                                                     int n_idx, int s_ndim, int n_spectra, int mode, int has_closing);
int ffk_sequence_prefix_processes(ffk_resident* const* gates, const int32_t* slots, const double* gate_table,
                                  const double* gate_propagators, const double* tau, int T, const int32_t* offsets,
                                  const int32_t* index, int P, const double* omega, int W, const double* basis,
                                  int hermitian_basis, int d, int A, int N, const int32_t* closing,
                                  const double* spectrum, int s_ndim, int n_spectra, const int32_t* idx, int n_idx,
                                  int mode, double* out);

/* ---- frequency shifts (second order) of every PREFIX of many gate sequences from one gate set in ONE pass, under
 *      any number of spectra (ff.sequence_prefix_frequency_shifts) ----
 * The arguments of ffk_sequence_prefix_processes without mode (closing (n_index,) int32 host or NULL among them), and
 * gate_shifts (n_spectra, T, n_idx, N, N) f64 host as for ffk_sequence_frequency_shifts: the gates' own frequency
 * shifts under each spectrum.  out (n_spectra, n_index, n_idx, N, N) f64 host: the result of global position
 * offsets[p] + g is the frequency shift of the sequence index[offsets[p] : offsets[p] + g + 1], with the gate
 * closing[offsets[p] + g] appended if closing is given.  The forward walk of ffk_sequence_frequency_shifts holds the
 * frequency shift of the first m gates in its accumulators after position m; a closing gate c adds one more summand
 * of the same form from the state the walk holds,
 *     Lam_{m+1}^T gate_shifts[c] Lam_{m+1} + sum_w c_w S(w) Re(conj((R_c Lam_{m+1})[k, w]) C_m[l, w]),
 * so each sequence is walked once, G positions instead of the G (G + 1) / 2 of its prefixes taken as sequences, with
 * one epilogue per position on copies of the accumulators.  One H2D copy, four launches whatever P, n_index and
 * n_spectra -- the front, the weights, the walk (one or two spectra share a walk, a function of d, A and whether
 * closing is given; grid z carries the further ones), the sum of the frequency blocks' partial tiles in block order
 * --, one D2H copy.  Arena workspace, no result handle.  A position's result is the same bits whatever else is in the
 * pass, whatever lies behind it in its sequence and however many spectra the call carries; without closing, position
 * 0 of a sequence returns that gate's row of gate_shifts.  Bad arguments (a closing entry outside [0, T) among them):
 * FFK_EINVAL before anything touches the device.  The workspace query needs no GPU (0: unsupported shape). */
size_t ffk_sequence_prefix_frequency_shifts_workspace_bytes(int T, int P, int n_index, int n_host, int d, int A, int N,
                                                            int W, int n_idx, int s_ndim, int n_spectra,
                                                            int has_closing);
int ffk_sequence_prefix_frequency_shifts(ffk_resident* const* gates, const int32_t* slots, const double* gate_table,
                                         const double* gate_propagators, const double* tau, int T,
                                         const int32_t* offsets, const int32_t* index, int P, const double* omega,
                                         int W, const double* basis, int hermitian_basis, int d, int A, int N,
                                         const int32_t* closing, const double* spectrum, int s_ndim, int n_spectra,
                                         const int32_t* idx, int n_idx, const double* gate_shifts, double* out);

/* ---- one-sided all-gather of the F blocks over xGMI (frequency-sharded step; the
 *      reference has no multi-device path: numeric.py:846-869 is embarrassingly parallel in omega
 *      and this is the exchange that reassembles F(omega) for util.integrate, util.py:880-906) ----
 * Every rank pushes its block into slot `rank` of a gather buffer on every rank through pointers
 * obtained with ffk_ipc_open_handle, with a copy kernel that needs no LDS (it shares the CUs with
 * the accumulate kernel, which an RCCL all-gather kernel cannot), and completion travels as
 * sequence numbers in 64-bit flag words polled with a timeout (error word, sticky -- the first
 * failure stays: 1 = acknowledgement timed out in push, the copy to that peer was skipped; 2 =
 * signal timed out in wait; 3 = a peer published the poison value).  A rank whose error word is set
 * signals the poison value (-1) instead of sequence numbers from then on, so that no peer
 * integrates a slot that was never filled: the failure reaches every rank within one step.  dst / flags / acks are DEVICE arrays of
 * `world` device pointers (addresses on rank p of: the slot of this rank in the buffer set, the flag
 * word of this rank, the acknowledgement word of this rank); `acks` / `flags` of push / wait are
 * this rank's own words, one per peer.  filter_functions_amd/parallel.py holds the protocol.     */
#define FFK_IPC_HANDLE_BYTES 64
int ffk_ipc_get_handle(const void* dptr, void* handle);
int ffk_ipc_open_handle(const void* handle, void** dptr);
int ffk_ipc_close_handle(void* dptr);
int ffk_peer_push_dev(const double* src, size_t bytes, void* const* dst, const int64_t* acks,
                      int64_t need_ack, int world, int rank, int32_t* error, void* stream);
int ffk_peer_signal_dev(void* const* flags, void* const* acks, int world, int64_t seq,
                        int64_t consumed, const int32_t* error, void* stream);
/* timeout of every poll of the protocol (default 2000 ms, or the environment variable
 * FFK_PEER_TIMEOUT_MS); legitimate host stalls on a peer (first-launch compilation, a profiler, a
 * garbage collection) must fit into it */
int ffk_peer_set_timeout_ms(double ms);
int ffk_peer_wait_dev(const int64_t* flags, int world, int64_t seq, int32_t* error, void* stream);
/* the three of step `step` in one call: push (after acknowledgements >= need_ack), signal
 * (flags = step + 1, acknowledging `step` buffers consumed), wait (flags of every peer >= step + 1) */
int ffk_peer_step_dev(const double* src, size_t bytes, void* const* dst, const int64_t* own_acks,
                      int64_t need_ack, void* const* flag_at, void* const* ack_at,
                      const int64_t* own_flags, int world, int rank, int64_t step, int32_t* error,
                      void* stream);

/* ---- hipGraph capture of device-pointer calls ------------------------------------------------
 * The reference's user-facing call (PulseSequence.get_filter_function, pulse_sequence.py:691-805 ->
 * numeric.calculate_control_matrix_from_scratch, numeric.py:707-881) is one Python call; here a
 * pass is 6 kernel launches whose host-side enqueue cost rivals their device time.  Any sequence
 * of `_dev` calls issued on `stream` between ffk_graph_capture_begin and ffk_graph_capture_end is
 * recorded instead of executed and comes back as one graph; ffk_graph_launch replays it on any
 * stream with a single runtime call.  Work forked onto other streams inside the capture
 * (ffk_event_record on the captured stream, a wait for that event on the other stream) is captured
 * too, provided it is joined back the same way before the end.  Arguments are frozen at capture:
 * every buffer a captured call names (inputs, outputs, workspace) must stay allocated and in place
 * while the graph lives; their CONTENTS may change between replays.  `stream` must be a created
 * stream (ffk_stream_create or any hipStream_t), not the null stream.  ffk_graph_capture_abort
 * leaves capture mode after a failed call. */
typedef struct ffk_graph ffk_graph;
int ffk_graph_capture_begin(void* stream);
int ffk_graph_capture_end(void* stream, ffk_graph** graph);
int ffk_graph_capture_abort(void* stream);
int ffk_graph_launch(ffk_graph* graph, void* stream);
int ffk_graph_node_count(const ffk_graph* graph, int* nodes);
int ffk_graph_destroy(ffk_graph* graph);
int ffk_stream_wait_event(void* stream, void* event);

/* ---- tuning / introspection ------------------------------------------------------------ */
/* Number of segment chunks the control-matrix kernel splits G into (0 = automatic).        */
int ffk_set_segment_chunks(int chunks);
/* Kernel variant of the control-matrix accumulation: 0 = default (multi-wave blocks sharing the
 * generated integral through LDS), 1 = one-wave-per-block variant for d <= 4 (kept for tuning;
 * measured slower on MI355X because its 48 accumulators per lane spill into AGPRs),
 * 2 = default kernel without the in-block segment split (tuning), 3 = never use the matrix-core
 * kernel (d >= 12 use it by default), 4 = use the matrix-core kernel wherever it exists (d = 8 too). */
int ffk_set_accumulate_variant(int variant);
/* Per-call statistics of the last ffk_control_matrix*_dev launch on this thread:
 * algorithmic FP64 flops of the accumulate kernel, its grid/block geometry, chunks used.
 * A batched pass (ffk_pipeline_batch_dev) on its fused route records its one accumulate launch over
 * the P G segments: chunks = grid_z = P x (chunks per pulse), accumulate_flops = 0 (not modelled);
 * where it runs P single passes it leaves the last of them.                                  */
typedef struct ffk_stats {
    double accumulate_flops;   /* FMA-counted real flops ffk::ctrl_accumulate executes      */
    double accumulate_bytes;   /* HBM bytes it must move (inputs + partial sums)            */
    int chunks;                /* segment chunks                                            */
    int grid_x, grid_y, grid_z, block;
    int lds_bytes;
} ffk_stats;
int ffk_get_stats(ffk_stats* out);
/* Profiling hook: when both are non-NULL hipEvent_t handles, the next ffk_control_matrix_dev /
 * ffk_pipeline_dev calls on this thread record `start` immediately before and `stop`
 * immediately after the accumulate kernel, on the stream it is launched on (so that a caller
 * can time the dominant kernel inside its own timed region); the concatenation entry points
 * (ffk_concatenate_sequence*) do the same around their rule kernel.  Pass NULLs to switch off. */
int ffk_set_accumulate_events(void* start, void* stop);
/* With several passes in flight on several streams, the accumulate kernel of one pass waits for the
 * blocks of the other pass's to retire, and a start event recorded on its own stream would include
 * that wait.  `event` (recorded on another stream; NULL = none) is waited for on the launch stream
 * right before `start` is recorded; it applies to the calls that follow until reset, and
 * ffk_set_accumulate_events resets it.                                                          */
int ffk_set_accumulate_gate(void* event);

#ifdef __cplusplus
}
#endif
#endif /* FFK_H */

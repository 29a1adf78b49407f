/*
 * mspmv.h -- C-ABI of the MI355X-native merge-path CSR SpMV/SpMM + CG library (libmspmv.so).
 *
 * This is the drop-in boundary for the reference's hot path
 * (YuyaW-0118/Sparse-Matrix-Linear-Equations).  Each entry point names the reference
 * interface it replaces (file:line in the reference checkout).  Plain pointers and sizes
 * only; no C++ or torch types.  The header-only C++ facade in mspmv.hpp re-exposes the
 * reference's own template names (CsrMatrix, OmpMergeCsrmv, OmpMergeCsrmm, CGSolveSingle,
 * CGSolveMultiple) on top of these.
 *
 * Types: values fp64, indices int32 -- CsrMatrix<double,int> (sparse_matrix.h:633-653).
 * Dense multi-vector panels are ROW-MAJOR n x L (X[c*L + j]), the layout of
 * OmpMergeCsrmm / CGSolveMultiple (merge_based.hpp:97-100, utils_multiple.hpp:17).
 *
 * Threading: one handle per host thread.  Work is enqueued on the handle's own HIP
 * stream; *_dev calls are asynchronous with respect to the host (use mspmv_sync);
 * host-pointer calls copy in, compute, copy out and return synchronously.  There is no
 * global mutable state except the thread-local last-error string.
 *
 * Errors: every call returns an mspmv_status; nothing calls exit() (unlike
 * sparse_matrix.h:232,297,305).  mspmv_last_error() describes the last failure on the
 * calling thread.
 */
#ifndef MSPMV_H
#define MSPMV_H

#include <stddef.h>

#ifndef MSPMV_API
#define MSPMV_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mspmv_status {
    MSPMV_OK = 0,
    MSPMV_ERR_INVALID = 1,       /* bad argument / shape */
    MSPMV_ERR_HIP = 2,           /* a HIP runtime call failed */
    MSPMV_ERR_OOM = 3,           /* device allocation failed */
    MSPMV_ERR_BREAKDOWN = 4,     /* CG: p.Ap <= 0 or non-finite (the reference has no guard) */
    MSPMV_ERR_RCCL = 5,          /* a collective failed */
    MSPMV_ERR_UNSUPPORTED = 6,   /* e.g. L outside the compiled set */
    MSPMV_ERR_IO = 7,            /* MatrixMarket read/parse failure */
    MSPMV_ERR_STALL = 8,         /* IC(0) / ILU(0) apply: a triangular-solve dependency never became ready
                                    (the solve stopped; X is not a solution) */
    MSPMV_ERR_FAULT = 9          /* a cross-workgroup fold ticket drew past its group: its array was
                                    not zero when the launch began, so a fold summed partials not yet
                                    written or never ran (results invalid; a CG solve stops) */
} mspmv_status;

/* Mirror of CsrMatrix<double,int> fields, sparse_matrix.h:648-653.  row_offsets has
 * num_rows+1 entries; column indices sorted within each row as CsrMatrix::Init leaves
 * them (stable_sort by (row,col), sparse_matrix.h:680); duplicates allowed. */
typedef struct mspmv_csr_d {
    int num_rows;
    int num_cols;
    int num_nonzeros;
    const int *row_offsets;
    const int *column_indices;
    const double *values;
} mspmv_csr_d;

typedef struct mspmv_handle_s *mspmv_handle;
/* An IC(0) factor resident on a device (mspmv_ic0_create). */
typedef struct mspmv_ic0_s *mspmv_ic0;
/* An ILU(0) factor resident on a device (mspmv_ilu0_create).  A type of its own: a nonsymmetric
 * factor cannot be handed to the PCG. */
typedef struct mspmv_ilu0_s *mspmv_ilu0;

/* Merge-path coordinate (CUB CoordinateT / the reference's int2, types.hpp:3-7). */
typedef struct mspmv_coord {
    int x; /* row index (merge list A = row end offsets) */
    int y; /* nonzero index (merge list B = 0..nnz-1) */
} mspmv_coord;

/* SpmmKernel (work_2025/types.hpp:11-16).  Accepted for signature compatibility; the GPU
 * always runs its merge-path kernel. */
typedef enum mspmv_spmm_kernel { MSPMV_SIMPLE = 0, MSPMV_MERGE = 1, MSPMV_NONZERO_SPLIT = 2 } mspmv_spmm_kernel;

/* ---- library / errors -------------------------------------------------------------- */
MSPMV_API const char *mspmv_last_error(void);
MSPMV_API const char *mspmv_version(void);
/* Number of visible HIP devices (0 when none; never an error). */
MSPMV_API int mspmv_device_count(void);

/* ---- matrix handle ------------------------------------------------------------------ */
/* Upload the CSR once to HBM on `device` and build its merge-path tile plans.  Replaces
 * the per-call partitioning of OmpMergeCsrmv (cpu_spmv.cpp:379-389) and CUB's
 * DeviceSpmvSearchKernel (dispatch_spmv_orig.cuh:99-143): the matrix's pattern is fixed for the
 * handle's life, so the partition is computed once (its values can be replaced:
 * mspmv_csr_update_values).  `host` arrays are only read during the call. */
MSPMV_API mspmv_status mspmv_csr_create(const mspmv_csr_d *host, int device, mspmv_handle *out);
/* Same, from arrays already resident in HBM (copied device-to-device). */
MSPMV_API mspmv_status mspmv_csr_create_dev(const mspmv_csr_d *dev, int device, mspmv_handle *out);
MSPMV_API mspmv_status mspmv_destroy(mspmv_handle h);
MSPMV_API mspmv_status mspmv_shape(mspmv_handle h, int *num_rows, int *num_cols, int *num_nonzeros);
/* Milliseconds spent in mspmv_csr_create (upload + partition), the reference's setup_ms
 * (cpu_spmv.cpp:715-742). */
MSPMV_API double mspmv_setup_ms(mspmv_handle h);
/* Replace the values of h's matrix; the pattern (row offsets, columns) is unchanged.  values[k] is
 * entry k of the CSR the handle was created from, same order, num_nonzeros entries.  The loop this
 * is for: create once, update per time step / Newton iteration / load case, solve.
 *  - Stream order.  The _dev form is enqueued on the handle's stream and returns without a host
 *    sync: products and solves enqueued earlier see the old values, everything enqueued later the new
 *    ones, on every plan.  d_values must stay valid and unchanged until the stream has passed the
 *    update (mspmv_sync).  The host form copies in, updates, synchronises and records
 *    mspmv_update_ms.  (A handle's first update uploads the source maps of the reordered plans it
 *    holds: a blocking copy on the host side, not a wait for the stream.)  A preconditioner handle
 *    of mspmv_dpcg_spai_multi runs its products on A's stream: synchronise its update before that solve.
 *  - What is refreshed: the CSR values and every derived copy of every plan built so far, for every
 *    width (the offset windows' panels and remainder, the column-slab / sliced-ELL / slab-SpMM value
 *    streams, the register-resident CG's layout).  Plans built later read the new values.
 *  - What is kept: every plan decision, tile boundary, record, column stream, dictionary, ticket and
 *    the fault word; the kernel-name and plan queries and mspmv_setup_ms answer as before; cached
 *    solver graphs stay valid (every buffer they bake in is updated in place).
 *  - The values are not read on the host and not checked: Inf and NaN are legal, as at create.
 *    Padding slots of every layout keep their zeros.
 *  - MSPMV_ERR_INVALID: null handle, or null pointer with num_nonzeros > 0.  num_nonzeros == 0:
 *    MSPMV_OK, nothing enqueued.  MSPMV_ERR_UNSUPPORTED: a handle whose values belong to another
 *    handle (a row-range view) or that such views were cut from -- the local matrices inside the
 *    sharded mspmv_dist_* objects.  A rejected call enqueues nothing.
 *  - Not refreshed: mspmv_ic0 / mspmv_ilu0 factors (their values come from a host factorisation of
 *    the caller's matrix: recreate them) and the mspmv_dist_* objects.
 * A handle that is never updated holds no more device memory and launches nothing else than
 * before this entry existed. */
MSPMV_API mspmv_status mspmv_csr_update_values(mspmv_handle h, const double *values);       /* host pointer, synchronous */
MSPMV_API mspmv_status mspmv_csr_update_values_dev(mspmv_handle h, const double *d_values); /* device pointer, asynchronous */
/* Wall milliseconds of the last host-pointer update (0 before any), as mspmv_setup_ms. */
MSPMV_API double mspmv_update_ms(mspmv_handle h);
/* Block until all work enqueued on the handle's stream has finished. */
MSPMV_API mspmv_status mspmv_sync(mspmv_handle h);
/* Confine the handle's work to num_cus compute units (spread evenly over the device's CUs, so
 * over its XCDs), or to all of them when num_cus <= 0 or >= the device's count: the handle's
 * stream is replaced by a CU-masked one (hipExtStreamCreateWithCUMask) and launch sizing follows
 * the new count.  The GPU counterpart of the thread count that OpenMP runs take
 * (parallel_efficiency.cpp:67-113 sets omp_set_num_threads per point); tools/parallel_efficiency.py
 * sweeps it, one CU count per process.  One masked stream per (device, count) is created per
 * process and shared by all handles limited to that count (a masked stream holds a hardware
 * queue of its own; a process has few).  Synchronizes the handle first. */
MSPMV_API mspmv_status mspmv_set_cu_limit(mspmv_handle h, int num_cus);

/* ---- Stream pool ------------------------------------------------------------------------ */
/* Every device has a pool of four non-blocking streams, created back to back by the first mspmv_csr_create
 * on it and never destroyed, so that each sits on a hardware queue of its own (a process opens four by
 * default).  mspmv_csr_create{,_dev} leases the lowest free slot and runs the handle on that slot's stream;
 * with every slot taken it creates a private stream, which shares a queue with some other.  The lease is
 * exclusive and returned by mspmv_destroy, and by mspmv_set_cu_limit when it moves the handle to a CU-masked
 * stream (back on all CUs the handle takes a free slot again, if there is one).  Independent products of a
 * batch (mspmv_spmm_batch_dev) overlap fully only on distinct queues: keep at most four pooled handles per
 * device alive where that matters.  MSPMV_STREAM_POOL=0 in the environment, read by every create, gives
 * every handle a private stream as before the pool. */
/* *slot = the pool slot whose stream h runs on (0..3), or -1: a private, caller's or CU-masked stream. */
MSPMV_API mspmv_status mspmv_stream_slot(mspmv_handle h, int *slot);
/* *slots = the slots of `device`'s pool, *leased = how many are held.  Either pointer may be NULL. */
MSPMV_API mspmv_status mspmv_stream_pool_stats(int device, int *slots, int *leased);
/* The slot ledger itself, host only (the handles' calls; exposed for tests): take puts the lowest free slot
 * of `device` into *slot and holds it, or -1 with every slot held; give returns a held slot and refuses
 * (MSPMV_ERR_INVALID) one that is not held.  Neither needs a device. */
MSPMV_API mspmv_status mspmv_stream_slot_take(int device, int *slot);
MSPMV_API mspmv_status mspmv_stream_slot_give(int device, int slot);

/* ---- Infinity-Cache leases ------------------------------------------------------------ */
/* Every product kernel exists in two forms: one reads the matrix's own arrays (values, columns,
 * records, panels) with default-policy loads, so their lines stay in the 256 MiB Infinity Cache for
 * the next product on the same matrix; the other reads them nontemporal, so a matrix that cannot stay
 * anyway does not evict x / X or another matrix's lines.  Which form a handle runs is decided from the
 * bytes one product on it streams from those arrays (the largest over the plans the handle has built;
 * x, y and solver vectors are not counted) against a budget the handles alive on one device share:
 *   - a stream of at most the floor (32 MiB, the eight L2s together) keeps default-policy loads and
 *     books nothing;
 *   - otherwise the handle asks the device's ledger for a lease of that size when its plain product's
 *     plan is decided (at creation) and again when a later plan streams more: granted while the live
 *     leases plus the request stay within the budget (default loads), refused otherwise (nontemporal
 *     loads, and the handle holds no lease).  First come, first served; returned at mspmv_destroy.
 * mspmv_set_cache_policy overrides the decision for one handle: MSPMV_CACHE_RESIDENT books the
 * stream whatever the budget says (later handles see it), MSPMV_CACHE_STREAM returns the lease,
 * MSPMV_CACHE_AUTO asks again.  It synchronizes the handle and drops its cached solver graphs (a
 * captured graph holds one instantiation); mspmv_spmv_kernel_name and mspmv_cg_kernel_name follow.
 * The handles inside a sharded object (mspmv_dist_create*) take no lease: under MSPMV_CACHE_AUTO they read
 * nontemporal when 12 nnz + 4 m of the rank's block exceeds 128 MiB, as every handle did before the ledger.
 * Results do not depend on the policy: both forms compute the same bits. */
enum { MSPMV_CACHE_AUTO = 0, MSPMV_CACHE_STREAM = 1, MSPMV_CACHE_RESIDENT = 2 };
MSPMV_API mspmv_status mspmv_set_cache_policy(mspmv_handle h, int policy);
/* *resident = 1 when h's products read the matrix with default-policy loads; *bytes = what one plain
 * single-RHS product streams from the matrix's arrays on its plan (the lease covers the largest plan built,
 * which may be another: a solver's, a wider product's).  Either pointer may be NULL. */
MSPMV_API mspmv_status mspmv_cache_info(mspmv_handle h, int *resident, long long *bytes);
/* The budget of `device`'s ledger in bytes (built-in default, or MSPMV_CACHE_MIB read once per
 * process); bytes < 0 queries only; *old (may be NULL) takes the value before the call.  Decisions
 * already made stay as they are.  mspmv_cache_floor: the same for the floor below which nothing is
 * booked.  Neither needs a device. */
MSPMV_API mspmv_status mspmv_cache_budget(int device, long long bytes, long long *old);
MSPMV_API mspmv_status mspmv_cache_floor(int device, long long bytes, long long *old);
/* The ledger itself, host only (the handles' calls; exposed for tests): exchanges a lease of `held`
 * bytes (0: none) on `device` for one of `want` bytes under `policy`.  *granted = the bytes booked
 * after the call (0: no lease), *resident = the load policy that follows.  mspmv_cache_leased: the sum
 * of the live leases. */
MSPMV_API mspmv_status mspmv_cache_lease(int device, long long held, long long want, int policy,
                                         long long *granted, int *resident);
MSPMV_API mspmv_status mspmv_cache_leased(int device, long long *bytes);

/* ---- merge-path partition ----------------------------------------------------------- */
/* Coordinates of the num_parts+1 partition boundaries exactly as OmpMergeCsrmv computes
 * them: diagonal_t = min(ceil((m+nnz)/P) * t, m+nnz), MergePathSearch over
 * (row_offsets+1, 0..nnz-1) (cpu_spmv.cpp:208-235, :379-389).  Computed on the GPU, one
 * lane per diagonal; bit-exact with the reference.  `coords` has num_parts+1 entries. */
MSPMV_API mspmv_status mspmv_merge_coords(mspmv_handle h, int num_parts, mspmv_coord *coords);

/* ---- SpMV / SpMM -------------------------------------------------------------------- */
/* y = A x   (OmpMergeCsrmv, cpu_spmv.cpp:357-421; cub::DeviceSpmv::CsrMV with alpha=1,
 * beta=0, device_spmv.cuh:129-164).  Host pointers: x[num_cols], y[num_rows]. */
MSPMV_API mspmv_status mspmv_dspmv(mspmv_handle h, const double *x, double *y);
/* Device pointers, asynchronous on the handle's stream. */
MSPMV_API mspmv_status mspmv_dspmv_dev(mspmv_handle h, const double *d_x, double *d_y);
/* Y = A X for L right-hand sides, row-major panels (OmpMergeCsrmm, merge_based.hpp:46-153).
 * Any L >= 1: the tile kernels run widths 1, 2, 4, 8, 16; other even L run as column chunks of
 * those widths over the same panels (stride L), odd L > 1 through a copy padded to L + 1
 * columns.  Even-L panels must be 16-byte aligned. */
MSPMV_API mspmv_status mspmv_dspmm(mspmv_handle h, const double *X, double *Y, int L);
MSPMV_API mspmv_status mspmv_dspmm_dev(mspmv_handle h, const double *d_X, double *d_Y, int L);
/* Batched product: d_Y[i] = A_i d_X[i] for `count` handles on one device, L in {1, 2, 4, 8, 16} (panels
 * 16-byte aligned for L > 1).  Product i is enqueued on hs[i]'s own stream by the launch path of
 * mspmv_dspmm_dev (same kernel, plan and order of sums) and the call returns without a host sync, with no
 * events and no waits between streams: work issued earlier on handle i precedes its product, work issued
 * later follows it, and products of different handles are unordered and may run at the same time.  A handle
 * listed twice is legal; its products run in order.  So that no overlap is a race, the y ranges
 * [d_Y[i], +8 m_i L) must be pairwise disjoint and disjoint from every x range [d_X[j], +8 n_j L), j = i
 * included (a shared x is fine): otherwise MSPMV_ERR_INVALID, naming the two products, and nothing is
 * launched.  No reference counterpart. */
MSPMV_API mspmv_status mspmv_spmm_batch_dev(int count, const mspmv_handle *hs, const double *const *d_X,
                                            double *const *d_Y, int L);
/* Block until every listed handle's stream has drained and run mspmv_check_faults on each (all of them,
 * even after one reports): MSPMV_ERR_FAULT, naming the first such product, if a ticket fault was raised. */
MSPMV_API mspmv_status mspmv_sync_batch(int count, const mspmv_handle *hs);

/* ---- initial guess (warm start) and the true residual --------------------------------------- */
/* Every solver below starts from x0 = 0 (the reference's behaviour, MSPMV_X0_ZERO, the default) unless the matrix's
 * handle is set to MSPMV_X0_CALLER: then every solver called with `h` as the matrix reads X on entry as X0 -- the
 * host- and device-pointer forms of mspmv_dcg_single, mspmv_dcg_multi, mspmv_dpcg_spai_multi, mspmv_dpcg_ic0_multi
 * (natural and multi-colour factors), mspmv_dbicgstab_multi, mspmv_dpbicgstab_ilu0_multi and mspmv_dbcg_multi; the
 * host-pointer forms upload X as well as B.  The setting is sticky on the handle, like mspmv_set_cu_limit and
 * mspmv_set_cache_policy; *old (may be NULL) takes the mode before the call.  MSPMV_ERR_INVALID for a null handle
 * or an unknown mode.  mspmv_dist_cg_dev (mspmv_dist.h) is out of scope: the sharded CG keeps x0 = 0.
 * A warm solve is the cold recurrence continued from X0, with the stop test still relative to ||B||:
 *   - R0 = B - A X0 (one product on the path the solver's own products take, one fused pass); the per-column
 *     scalars start from R0.R0, and Z = M R, Rhat = P = R, H = R^T R follow on R0 unchanged;
 *   - b_norm_j = ||B_j|| (0 -> 1): stop tests and history entries stay relative to ||B||; iterations count from
 *     the warm start;
 *   - entry test (warm only): a column with ||R0_j|| / b_norm_j < tolerance is marked converged by the init and
 *     its X column is returned as given (every update of it is x + 0 p with p = 0, which keeps every value's bits but
 *     a -0.0 entry's sign); when every column is, the solver returns *iters = 0 and MSPMV_OK and writes no history
 *     entry.  (The cold path keeps the reference's behaviour, a zero column's
 *     breakdown included.)
 *   - a non-finite X0 or B: no new rule -- the column breaks down and freezes as a non-finite B does, X as given;
 *   - block CG: its columns are coupled, so it needs a full-rank block of initial residuals: all columns converged
 *     at entry returns 0 iterations and MSPMV_OK, otherwise a rank-deficient R0 (one exact column, say) is the
 *     Cholesky-pivot MSPMV_ERR_BREAKDOWN at the init, X left as given;
 *   - single-RHS CG runs the split iteration at L = 1 (the form MSPMV_CG_SPLIT=1 selects; mspmv_cg_kernel_name
 *     reports it), not the resident or pipelined kernels, whose first iteration derives ||b|| from r.r;
 *   - widths outside {1, 2, 4, 8, 16}: X0's columns travel with B's into each column group;
 *   - X0 = 0 with tolerance < 1 and no zero column in B: X, *iters, the history and the status are bit for bit
 *     the cold solve's (single-RHS: the cold split form's). */
enum { MSPMV_X0_ZERO = 0, MSPMV_X0_CALLER = 1 };
MSPMV_API mspmv_status mspmv_set_initial_guess(mspmv_handle h, int mode, int *old);
/* R = B - A X on the handle's plain product, with its column norms from the same pass: norms[j] = ||B_j||_2 and
 * norms[L + j] = ||R_j||_2 (2 L values, on the host).  Any L >= 1 (native widths 1, 2, 4, 8, 16; any other as
 * column groups of those); square or rectangular handles: B and R are m x L, X is n x L, row-major.  d_R may be
 * NULL when only the norms are wanted.  Synchronizes (the norms come back to the host) and checks the fault word
 * as mspmv_dspmm does.  The check a caller makes of a solution: a solver's recurrence residual drifts from this
 * one.  Device panels must be 16-byte aligned at the native widths.  mspmv_dresidual: host pointers. */
MSPMV_API mspmv_status mspmv_dresidual_dev(mspmv_handle h, const double *d_B, const double *d_X, double *d_R, int L,
                                           double *norms);
MSPMV_API mspmv_status mspmv_dresidual(mspmv_handle h, const double *B, const double *X, double *R, int L,
                                       double *norms);

/* ---- CG ----------------------------------------------------------------------------- */
/* Single-RHS CG, CGSolveSingle (work_2025/main/single_strategy.hpp:102-170): x0 = 0 (unless
 * mspmv_set_initial_guess says MSPMV_X0_CALLER, above),
 * r = p = b; stop after the update of r when sqrt(r.r)/||b|| < tolerance, counting that
 * iteration; ||b|| == 0 -> 1.  `tolerance` has the reference's meaning (callers such as
 * cpu_singlecg.cpp:92,101 pass tol*||b||; that quirk is the caller's).  Returns the
 * iteration count in *iters.  resid_hist (optional, capacity hist_cap) receives
 * sqrt(r.r)/||b|| per iteration.  Host pointers b[n], x[n]. */
MSPMV_API mspmv_status mspmv_dcg_single(mspmv_handle h, const double *b, double *x, int max_iters, double tolerance,
                              int *iters, double *resid_hist, int hist_cap);
MSPMV_API mspmv_status mspmv_dcg_single_dev(mspmv_handle h, const double *d_b, double *d_x, int max_iters, double tolerance,
                                  int *iters, double *resid_hist, int hist_cap);
/* Diagnostic (measurement of configs[3]'s kernel): one register-resident single-RHS solve, as
 * mspmv_dcg_single_dev on device vectors, that also records wall_clock64() (a constant 100 MHz
 * clock) at five phase boundaries of every workgroup's iterations k < stamp_iters:
 * stamps[(k * G + w) * 5 + i], i = 0 iteration start, 1 the workgroup's rows of Ap done, 2 the
 * p.Ap total received, 3 the workgroup's r update done, 4 the r.r total received (entries of
 * iterations not run stay 0).  stamps holds stamp_iters * G * 5 values; *workgroups = G.
 * MSPMV_ERR_UNSUPPORTED when the matrix does not take the resident path.  No reference
 * counterpart (CGSolveSingle has no instrumentation). */
MSPMV_API mspmv_status mspmv_cg_resident_stamps(mspmv_handle h, const double *d_b, double *d_x, int max_iters,
                                                double tolerance, int *iters, unsigned long long *stamps,
                                                int stamp_iters, int *workgroups);
/* Block multi-RHS CG, CGSolveMultiple (work_2025/main/no_pretreatment.hpp:32-197): L
 * lock-step recurrences on interleaved n x L panels, per-column converged masks
 * (alpha = beta = 0 once converged), stop when all columns converged.  Breakdown is per
 * column: a column whose p.Ap gives a non-finite alpha (e.g. a zero RHS column, 0/0) is frozen
 * at its last finite iterate and left out of the history (the reference's column turns NaN and
 * never converges); the other columns keep iterating, and the call returns
 * MSPMV_ERR_BREAKDOWN with X holding every column's result.  max_err_hist
 * (optional) receives the per-iteration max over ALL columns of sqrt(r.r)/||b||
 * (:132-155).  Any L >= 1: widths outside {1, 2, 4, 8, 16} are solved as independent column
 * groups of those widths (the recurrences are per column), iteration count = the groups'
 * maximum, history = the max over groups with finished groups frozen, as the reference's. */
MSPMV_API mspmv_status mspmv_dcg_multi(mspmv_handle h, const double *B, double *X, int L, int max_iters, double tolerance,
                             mspmv_spmm_kernel kernel, int *iters, double *max_err_hist, int hist_cap);
MSPMV_API mspmv_status mspmv_dcg_multi_dev(mspmv_handle h, const double *d_B, double *d_X, int L, int max_iters,
                                 double tolerance, mspmv_spmm_kernel kernel, int *iters, double *max_err_hist,
                                 int hist_cap);

/* ---- BiCGSTAB (nonsymmetric systems) -------------------------------------------------- */
/* Multi-RHS BiCGSTAB for a square matrix that need not be symmetric or definite (van der
 * Vorst's recurrence, unpreconditioned -- mspmv_dpbicgstab_ilu0_multi below is the preconditioned
 * form -- shadow residual rhat = b); only A X is needed, no
 * transpose.  No reference counterpart (every solver of the reference is a CG).  Per column j of
 * the interleaved n x L panels: X = 0, R = P = B, rho = B.B; per iteration V = A P,
 * alpha = rho / (rhat.V), s = R - alpha V, X += alpha P, T = A s, omega = T.s / T.T (T.T == 0:
 * s is exactly 0 and omega = 0, not a breakdown), X += omega s, R = s - omega T, stop test on
 * sqrt(R.R)/||B_j|| < tolerance with per-column converged masks (alpha = omega = beta = 0 once
 * converged; ||B_j|| == 0 -> 1), rho' = rhat.R, beta = (rho'/rho)(alpha/omega), rho = rho',
 * P = R + beta (P - omega V).  Returns the iteration count in *iters (max_iters when not every
 * column converged); max_err_hist (optional, capacity hist_cap) receives the per-iteration max
 * over the columns of sqrt(R.R)/||B_j||.  Breakdown is per column, by mspmv_dcg_multi's rule: a
 * non-finite alpha, omega or beta (a zero RHS column; rho = 0 or omega = 0 on a column still
 * iterating) freezes the column at its last finite iterate and leaves it out of the history, the
 * other columns keep iterating, and the call returns MSPMV_ERR_BREAKDOWN with X holding every
 * column's result.  Any L >= 1 (column groups as mspmv_dcg_multi).  MSPMV_ERR_INVALID for a
 * non-square matrix, max_iters < 0, null vectors, or device vectors not 16-byte aligned. */
MSPMV_API mspmv_status mspmv_dbicgstab_multi(mspmv_handle h, const double *B, double *X, int L, int max_iters,
                                             double tolerance, int *iters, double *max_err_hist, int hist_cap);
MSPMV_API mspmv_status mspmv_dbicgstab_multi_dev(mspmv_handle h, const double *d_B, double *d_X, int L,
                                                 int max_iters, double tolerance, int *iters, double *max_err_hist,
                                                 int hist_cap);

/* ---- block CG (SPD systems, one Krylov space for all right-hand sides) ------------------ */
/* Block conjugate gradient in Dubrulle's BCGrQ form of O'Leary's method, for a symmetric positive
 * definite matrix.  Unlike every other multi-RHS solver here -- L lock-step recurrences that share
 * the matrix read and nothing else -- the L columns share ONE Krylov space: each iterate minimises
 * over the sum of the columns' spaces, so the iteration count falls as L grows -- by much where the
 * system is small or has few slow modes against L, by little on large smooth ones, while an
 * iteration costs more than the lock-step CG's (measured: DESIGN.md 4.4d).  No reference
 * counterpart (its CGSolveMultiple is the lock-step form).  With the interleaved n x L panels as
 * matrices, all small matrices L x L, and chol(G) the upper factor zeta with G = zeta^T zeta:
 *     init:  X = 0;  H = B^T B;  zeta = chol(H);  C = zeta;  W = B zeta^-1;  S = W;
 *            bnorm_j = ||C e_j||_2 (= ||B_j||; 0 -> 1)
 *     iter:  Q = A S
 *            G = S^T Q;  xi = G^-1 (by chol(G));  T = xi C
 *            X += S T;  V = W - Q xi;  H = V^T V
 *            zeta = chol(H);  C <- zeta C;  rel_j = ||C e_j||_2 / bnorm_j
 *            history[k] = max_j rel_j;  stop when every rel_j < tolerance, counting this iteration
 *            W = V zeta^-1;  S = W + S zeta^T
 * W is an orthonormal basis of the residual block R = W C, so ||R e_j|| = ||C e_j|| and columns that
 * converge at different speeds do not drive G or H singular.  An iteration is one product and three
 * streaming passes; the two Gram matrices fold in a fixed order, so a solve repeats bit for bit.
 * max_err_hist (optional) receives the per-iteration max over the columns of rel_j, as
 * mspmv_dcg_multi's; *iters the iterations completed (an iteration is complete once X and the
 * residual norms are updated).  The columns are coupled: there are no per-column masks and no
 * per-column freeze, and breakdown is one rule -- a Cholesky pivot of H or G that is <= 0 or
 * non-finite (a zero or linearly dependent right-hand-side column at the init; an exactly converged
 * direction later) ends the solve with MSPMV_ERR_BREAKDOWN.  X then holds the iterate of the last
 * completed iteration (0 when the init broke, *iters = 0), and the error text names the matrix, the
 * pivot index and the iteration: solve such a block with mspmv_dcg_multi, whose columns are
 * independent (deflation is not implemented).  L must be 1, 2, 4, 8 or 16: column groups would
 * uncouple the block, so any other width is MSPMV_ERR_UNSUPPORTED.  MSPMV_ERR_INVALID for a
 * non-square matrix, max_iters < 0, null vectors, or device vectors not 16-byte aligned.
 * mspmv_cg_kernel_name then reads "BlockCG-rQ (1 SpMM + 3 passes)", and
 * mspmv_solver_product_kernel_name names the product's kernel as for BiCGSTAB. */
MSPMV_API mspmv_status mspmv_dbcg_multi(mspmv_handle h, const double *B, double *X, int L, int max_iters,
                                        double tolerance, int *iters, double *max_err_hist, int hist_cap);
MSPMV_API mspmv_status mspmv_dbcg_multi_dev(mspmv_handle h, const double *d_B, double *d_X, int L, int max_iters,
                                            double tolerance, int *iters, double *max_err_hist, int hist_cap);

/* ---- SPAI-preconditioned block CG ---------------------------------------------------- */
/* SPAI preconditioner M with A's own pattern, SparseApproximateInversion
 * (work_2025/cg/sparse_approximate_inversion.hpp:40-321): column k of M minimises
 * ||A(I,J) m - e_k(I)||_2 (J = rows of A's column k, I = rows those columns touch; Householder
 * QR where the reference calls LAPACKE_dgels; a rank-deficient column gives zeros, as the
 * reference's info != 0 fallback), then M = (M + M^T)/2 over the pattern.  Host setup
 * (OpenMP), like the reference's; m_values[num_nonzeros] receives M's values in A's CSR order,
 * so M's CSR is (A.row_offsets, A.column_indices, m_values).  Square A only. */
MSPMV_API mspmv_status mspmv_spai_values(const mspmv_csr_d *a, double *m_values);
/* SPAISolveMultiple (work_2025/main/sparse_approximate_inverse.hpp:30-230) on the GPU: X = 0,
 * R = B, Z = M R, P = Z, rs_old = R.Z; per iteration AP = A P, alpha = rs_old/P.AP (0 when
 * converged or P.AP == 0), X += alpha P, R -= alpha AP, stop test on sqrt(R.R)/||B_j|| with the
 * per-column masks and the max-over-columns history, Z = M R, beta = R.Z/rs_old (0 when converged
 * or rs_old == 0), P = Z + beta P.  `m` is M's handle (same shape and device as `a`); both SpMMs
 * are merge-path tile kernels.  Any L >= 1 (column groups as mspmv_dcg_multi); interleaved
 * n x L panels. */
MSPMV_API mspmv_status mspmv_dpcg_spai_multi(mspmv_handle a, mspmv_handle m, const double *B, double *X, int L,
                                             int max_iters, double tolerance, mspmv_spmm_kernel kernel, int *iters,
                                             double *max_err_hist, int hist_cap);
MSPMV_API mspmv_status mspmv_dpcg_spai_multi_dev(mspmv_handle a, mspmv_handle m, const double *d_B, double *d_X,
                                                 int L, int max_iters, double tolerance, mspmv_spmm_kernel kernel,
                                                 int *iters, double *max_err_hist, int hist_cap);

/* ---- IC(0)-preconditioned block CG --------------------------------------------------- */
/* IncompleteCholesky (work_2025/cg/incomplete_cholesky_decomp.hpp:84-201) on the host, as in the
 * reference: L has A's lower-triangle pattern (diagonal included, A's CSR order); on a
 * non-positive pivot the factorization restarts with the diagonal shifted by 1e-3, x10 per
 * attempt, 20 attempts (MSPMV_ERR_BREAKDOWN after that).  mspmv_ic0_nnz gives L's nonzero count;
 * l_row_offsets[n+1], l_cols / l_vals[nnz_l] receive L; *shift (nullable) the shift used.
 * Precondition, checked by mspmv_ic0_factor: in every row of A the entries with column <= row
 * are strictly ascending and end in the diagonal (sorted columns, no duplicates, every diagonal
 * present) -- the recurrence merges rows in that order and takes a row's last lower entry as its
 * diagonal.  Anything else is MSPMV_ERR_INVALID, the message naming the first such row. */
MSPMV_API mspmv_status mspmv_ic0_nnz(const mspmv_csr_d *a, int *nnz_l);
MSPMV_API mspmv_status mspmv_ic0_factor(const mspmv_csr_d *a, int *l_row_offsets, int *l_cols, double *l_vals,
                                        double *shift);
/* TransposeCsr (work_2025/cg/incomplete_cholesky_decomp.hpp:11-78) on the host: out_row_offsets
 * [num_cols+1], out_cols / out_vals [num_nonzeros] receive A^T in CSR, each row's entries in
 * ascending column order (the reference's counting sort). */
MSPMV_API mspmv_status mspmv_csr_transpose(const mspmv_csr_d *in, int *out_row_offsets, int *out_cols,
                                           double *out_vals);
/* Upload L and its transpose (TransposeCsr, :11-78) for the GPU triangular solves. */
MSPMV_API mspmv_status mspmv_ic0_create(const mspmv_csr_d *l, int device, mspmv_ic0 *out);
MSPMV_API mspmv_status mspmv_ic0_destroy(mspmv_ic0 m);
/* PCGSolveMultiple (work_2025/main/incomplete_cholesky.hpp:33-199) on the GPU: Z = L^-T L^-1 R by
 * two sync-free triangular solves per application (one wave per row in dependency-level order;
 * the output panel starts filled with a pending pattern and a consumer polls the value it needs),
 * merge-path SpMM for A P, the reference's masks and max-residual history.  A stalled solve
 * (a dependency never ready) stops the iteration and is reported as MSPMV_ERR_STALL, never a
 * hang.  mspmv_ic0_create rejects a factor with an entry above the diagonal or a row without
 * its diagonal (either would make a solve wait forever). */
MSPMV_API mspmv_status mspmv_dpcg_ic0_multi(mspmv_handle a, mspmv_ic0 m, const double *B, double *X, int L,
                                            int max_iters, double tolerance, mspmv_spmm_kernel kernel, int *iters,
                                            double *max_err_hist, int hist_cap);
MSPMV_API mspmv_status mspmv_dpcg_ic0_multi_dev(mspmv_handle a, mspmv_ic0 m, const double *d_B, double *d_X, int L,
                                                int max_iters, double tolerance, mspmv_spmm_kernel kernel,
                                                int *iters, double *max_err_hist, int hist_cap);
/* One triangular solve with the factor: transpose = 0 solves L X = B, 1 solves L^T X = B.
 * Device panels n x L row-major, 16-byte aligned, L in {1,2,4,8,16}; B and X must not overlap
 * (X is pre-filled with the pending pattern).  Runs on a's stream with a's control block,
 * synchronises; MSPMV_ERR_STALL exactly as the PCG reports it.  MSPMV_ERR_INVALID (X untouched)
 * for a factor of another shape or device, a null or misaligned panel, overlapping panels;
 * MSPMV_ERR_UNSUPPORTED for another L. */
MSPMV_API mspmv_status mspmv_ic0_solve_dev(mspmv_handle a, mspmv_ic0 m, int transpose, const double *d_B,
                                           double *d_X, int L);

/* ---- ILU(0)-preconditioned BiCGSTAB (nonsymmetric systems) ---------------------------- */
/* ILU(0) on the host, in A's own pattern, row by row in IKJ order: for each entry (i, k) of row i
 * with k < i, ascending, l = w(k) / U(k,k), w(k) = l, w(j) -= l U(k,j) for every j > k held by
 * both rows' patterns (every l * u and the subtraction round separately).  lu_values[num_nonzeros]
 * receives the factors in A's CSR order, like mspmv_spai_values: entries with column < row hold L's
 * multipliers (unit diagonal implied), entries with column >= row hold U.  Sequential, like
 * mspmv_ic0_factor.  No reference counterpart (the reference has no ILU), so no diagonal shifting:
 * a zero or non-finite pivot is MSPMV_ERR_BREAKDOWN, the message naming the row.
 * Precondition, checked first: A is square and every row's columns ascend strictly (sorted, no
 * duplicates) and hold the diagonal.  Anything else is MSPMV_ERR_INVALID, the message naming the
 * first such row. */
MSPMV_API mspmv_status mspmv_ilu0_values(const mspmv_csr_d *a, double *lu_values);
/* Upload the factor for the GPU triangular solves: `lu` is A's pattern with mspmv_ilu0_values'
 * values, split into L (the strictly lower entries and a stored 1.0 diagonal, last in its row) and
 * U (the diagonal first, then the upper entries), each with its dependency-level order.  The row
 * checks of mspmv_ilu0_values apply; a zero or non-finite diagonal is MSPMV_ERR_INVALID (a solve
 * must never divide by it).  All of that is checked before the device is touched. */
MSPMV_API mspmv_status mspmv_ilu0_create(const mspmv_csr_d *lu, int device, mspmv_ilu0 *out);
MSPMV_API mspmv_status mspmv_ilu0_destroy(mspmv_ilu0 m);
/* One triangular solve with the factor: upper = 0 solves L X = B (unit diagonal), 1 solves
 * U X = B.  The contract of mspmv_ic0_solve_dev, check for check: device panels n x L row-major,
 * 16-byte aligned, not overlapping, L in {1,2,4,8,16} (MSPMV_ERR_UNSUPPORTED otherwise); a factor of
 * another shape or device is MSPMV_ERR_INVALID; MSPMV_ERR_STALL as the solver reports it; X is
 * untouched on a rejected call. */
MSPMV_API mspmv_status mspmv_ilu0_solve_dev(mspmv_handle a, mspmv_ilu0 m, int upper, const double *d_B,
                                            double *d_X, int L);

/* ---- multi-colour ILU(0): the factor whose solves are one parallel sweep per colour ------- */
/* Greedy colouring of the graph of A + A^T's off-diagonal pattern (stored zeros count as entries):
 * rows 0..n-1 in turn take the smallest colour that no already-coloured neighbour holds.  Sequential
 * and deterministic.  colors[n] receives the colours, *num_colors their number, at most the largest
 * degree of the symmetrised pattern + 1.  A must pass mspmv_ilu0_values' row checks
 * (MSPMV_ERR_INVALID otherwise). */
MSPMV_API mspmv_status mspmv_color_greedy(const mspmv_csr_d *a, int *colors, int *num_colors);
/* Ap = P A P^T for a square CSR A: row i of Ap is row perm[i] of A, its columns renumbered by the
 * inverse permutation and sorted ascending.  ro[n + 1], ci[nnz], va[nnz] receive Ap.
 * MSPMV_ERR_INVALID when perm is not a permutation of 0..n-1 (an index out of range or repeated). */
MSPMV_API mspmv_status mspmv_csr_permute_sym(const mspmv_csr_d *a, const int *perm, int *ro, int *ci, double *va);
/* The multi-colour ILU(0) factor of A itself (not of a factor): rows that share a colour share no
 * entry, perm orders the rows stably by colour (ascending within a colour), and the factor is
 * mspmv_ilu0_values run on Ap = P A P^T, so it has at most as many dependency levels as colours and
 * a triangular solve is one launch per colour.  colors == NULL: mspmv_color_greedy's.  Colours the
 * caller supplies (a block or any other colouring) must lie in [0, n), use every colour of 0..C-1,
 * and give no two rows joined by an entry (i, j), i != j, of A the same colour: MSPMV_ERR_INVALID
 * otherwise, the message naming the first offending row.  A's row checks are mspmv_ilu0_values';
 * a zero or non-finite pivot of the permuted factorisation is MSPMV_ERR_BREAKDOWN (the row named in
 * the colour ordering).  All of that happens before the device is touched.  Uploaded: L's strictly
 * lower entries (unit diagonal implied), U with the diagonal first, perm and the colour offsets.
 * The result is an ordinary mspmv_ilu0: mspmv_dpbicgstab_ilu0_multi[_dev] takes it unchanged
 * (mspmv_cg_kernel_name then reads "MC-ILU0-BiCGSTAB (2 SpMM + 4 sweeps of C colours + 5 passes)"
 * and MSPMV_ERR_STALL cannot occur), mspmv_ilu0_destroy frees it.
 * Summation order of a solve's row: the first product plus numpy's pairwise sum of the rest (in
 * CSR order; sequential up to 7 further products, eight interleaved running sums beyond, halves
 * beyond 128) -- the order np.add.reduceat gives, so a solve is reproducible against it bit for
 * bit.  A long row is summed by max(1, L / 2) lanes alone: the known cost of that exactness. */
MSPMV_API mspmv_status mspmv_ilu0_create_colored(const mspmv_csr_d *a, const int *colors, int device,
                                                 mspmv_ilu0 *out);
/* *num_colors: the factor's colours, 0 for a natural-order factor (mspmv_ilu0_create); perm (null,
 * or n entries): row i of the permuted matrix is row perm[i] of A (untouched for 0 colours).
 * On a multi-colour factor mspmv_ilu0_solve_dev solves one triangle of Ap's factor, B and X in the
 * colour ordering, under the same argument contract. */
MSPMV_API mspmv_status mspmv_ilu0_colors(mspmv_ilu0 m, int *num_colors, int *perm);
/* X = M^-1 B = U^-1 L^-1 B in A's own ordering, for either kind of factor, on a's stream,
 * synchronised: the two tagged solves through the factor's intermediate (natural order), or the
 * colour sweeps, which gather by perm on the way in and scatter on the way out (no pass of their
 * own).  mspmv_ilu0_solve_dev's argument contract without `upper`; X is untouched on a rejected
 * call. */
MSPMV_API mspmv_status mspmv_ilu0_apply_dev(mspmv_handle a, mspmv_ilu0 m, const double *d_B, double *d_X, int L);
/* Right-preconditioned multi-RHS BiCGSTAB with M = L U.  The residual is the original system's, so
 * the stop test and the history mean what they mean in mspmv_dbicgstab_multi.  Per column, X = 0,
 * R = Rhat = P = B, rho = B.B; per iteration Phat = U^-1 L^-1 P, V = A Phat, alpha = rho / (Rhat.V),
 * s = R - alpha V, X += alpha Phat, Shat = U^-1 L^-1 s, T = A Shat, omega = T.s / T.T (T.T == 0:
 * omega = 0, not a breakdown), X += omega Shat, R = s - omega T, stop test on sqrt(R.R)/||B_j||,
 * rho' = Rhat.R, beta = (rho'/rho)(alpha/omega), P = R + beta (P - omega V).  Masks, the per-column
 * freeze (MSPMV_ERR_BREAKDOWN with the other columns solved), ||B_j|| == 0 -> 1, the history, the
 * iteration count and any L >= 1 are mspmv_dbicgstab_multi's.  An iteration is two products, four
 * sync-free triangular solves (as mspmv_dpcg_ic0_multi's) and five streaming passes; a stalled
 * triangular solve stops the iteration and is reported as MSPMV_ERR_STALL, never a hang.
 * MSPMV_ERR_INVALID for a null factor, a factor of another shape or device, a non-square matrix,
 * max_iters < 0, null vectors, or device vectors not 16-byte aligned.  No reference counterpart. */
MSPMV_API mspmv_status mspmv_dpbicgstab_ilu0_multi(mspmv_handle a, mspmv_ilu0 m, const double *B, double *X, int L,
                                                   int max_iters, double tolerance, int *iters,
                                                   double *max_err_hist, int hist_cap);
MSPMV_API mspmv_status mspmv_dpbicgstab_ilu0_multi_dev(mspmv_handle a, mspmv_ilu0 m, const double *d_B, double *d_X,
                                                       int L, int max_iters, double tolerance, int *iters,
                                                       double *max_err_hist, int hist_cap);

/* ---- multi-colour IC(0): the same ordering for the block PCG -------------------------- */
/* The multi-colour IC(0) factor of A itself (not of a factor).  colors == NULL: mspmv_color_greedy's;
 * colours the caller supplies pass mspmv_ilu0_create_colored's checks (in [0, n), every colour of
 * 0..C-1 in use, no entry (i, j), i != j, joining two rows of one colour: MSPMV_ERR_INVALID otherwise,
 * the message naming the first offending row).  Then perm orders the rows stably by colour,
 * Ap = P A P^T (mspmv_csr_permute_sym), and L is mspmv_ic0_factor of Ap -- with its row checks (a row
 * without its diagonal is MSPMV_ERR_INVALID, the row named in the colour ordering) and its
 * diagonal-shift retries (*shift, nullable, receives the shift used; MSPMV_ERR_BREAKDOWN after 20
 * attempts) -- and L^T is mspmv_csr_transpose of it.  A's own structure is checked as mspmv_ic0_nnz
 * checks it (square, consistent offsets, columns in range).  All of that happens before the device
 * is touched.  Uploaded: L (diagonal last in its row), L^T (diagonal first), perm, the colour offsets.
 * The result is an ordinary mspmv_ic0: mspmv_dpcg_ic0_multi[_dev] takes it unchanged
 * (mspmv_cg_kernel_name then reads "MC-IC0-PCG (split, S sweeps of C colours)", S = 2 C - 1, and
 * MSPMV_ERR_STALL cannot occur), mspmv_ic0_destroy frees it.  An apply Z = P^T L^-T L^-1 P R is one
 * launch per colour and triangle, in stream order; the last colour's rows of L^T hold the diagonal
 * alone, so its forward launch divides twice (y = (r - s) / d, z = y / d, each rounded) and the
 * backward sweeps start at colour C - 2: 2 C - 1 launches.  A row's sum runs over the entries before
 * the diagonal in mspmv_ilu0_create_colored's summation order, so a solve is reproducible against
 * np.add.reduceat bit for bit.  No reference counterpart; red-black orderings cost iterations. */
MSPMV_API mspmv_status mspmv_ic0_create_colored(const mspmv_csr_d *a, const int *colors, int device, double *shift,
                                                mspmv_ic0 *out);
/* *num_colors: the factor's colours, 0 for a natural-order factor (mspmv_ic0_create); perm (null,
 * or n entries): row i of the permuted matrix is row perm[i] of A (untouched for 0 colours).
 * On a multi-colour factor mspmv_ic0_solve_dev solves one triangle of Ap's factor, B and X in the
 * colour ordering (colours ascending for L, descending for L^T; no pending-pattern fill, no
 * polling), under the same argument contract. */
MSPMV_API mspmv_status mspmv_ic0_colors(mspmv_ic0 m, int *num_colors, int *perm);
/* X = L^-T L^-1 B in A's own ordering, for either kind of factor, on a's stream, synchronised: the
 * two tagged solves through the factor's intermediate (natural order), or the colour sweeps, which
 * gather by perm on the way in and scatter on the way out.  mspmv_ilu0_apply_dev's argument
 * contract, check for check; X is untouched on a rejected call. */
MSPMV_API mspmv_status mspmv_ic0_apply_dev(mspmv_handle a, mspmv_ic0 m, const double *d_B, double *d_X, int L);

/* ---- measurement helpers (HIP events on the handle's stream) ------------------------ */
/* Enqueue `reps` back-to-back SpMV (L == 1) or SpMM launches on device buffers and return
 * the average milliseconds per call measured by hipEvents on the handle's stream.
 * flush_bytes > 0 sweeps a scratch buffer of that many bytes before every call (outside the
 * timed events) to evict the 256 MiB Infinity Cache ("cold" protocol): a
 * nontemporal read sweep, so the caches hold clean unrelated lines (MSPMV_FLUSH=write: a write
 * sweep, whose dirty lines the timed call would pay to write back). */
MSPMV_API mspmv_status mspmv_time_spmm_dev(mspmv_handle h, const double *d_X, double *d_Y, int L, int reps,
                                 size_t flush_bytes, double *avg_ms);
/* Batch form for benchmarks: `reps` steps, each step one SpMM launch per handle (all handles
 * on one device), HIP events only around the whole region.  Product i of every step is enqueued
 * on hs[i]'s own stream, as mspmv_spmm_batch_dev enqueues it, so the launches of a step may run
 * at the same time (the y / x ranges must then be disjoint, as there); the start event is
 * recorded on hs[0]'s stream and waited on once by every other stream, and the end event follows
 * one done event per other stream: nothing per step.  MSPMV_BATCH_OVERLAP=0 (read per call):
 * every launch back to back on hs[0]'s stream instead; a batch of one handle is that form.
 * *step_ms = region time / reps; *tile_kernel_ms = region time / (reps x count): the region
 * time per product -- the duration of one launch (its boundary included) in the single-stream
 * form, less than that when the launches of a step overlap; *kernels_per_step = launches per
 * step (one per handle with rows). */
MSPMV_API mspmv_status mspmv_time_spmm_batch_dev(int count, const mspmv_handle *hs, const double *const *d_X,
                                                 double *const *d_Y, int L, int reps, double *step_ms,
                                                 double *tile_kernel_ms, int *kernels_per_step);
/* The practical HBM ceiling the roofline fraction is read against: a STREAM-like
 * nontemporal read of a `bytes` buffer (>= 1 MiB; use >> 256 MiB so the Infinity Cache cannot hold
 * it) on `device`, one contiguous slice per workgroup (the fastest read shape measured: ~6.9 TB/s
 * at 1 GiB), `reps` timed passes after one warm-up, HIP events around the timed region.
 * *gbps = bytes x reps / time. */
MSPMV_API mspmv_status mspmv_time_stream_read(int device, size_t bytes, int reps, double *gbps);
/* Per-kernel average duration (ms) of the dominant (merge tile) kernel over the last
 * mspmv_time_spmm_dev call, and the number of kernels per SpMV/SpMM call. */
MSPMV_API mspmv_status mspmv_last_kernel_ms(mspmv_handle h, double *tile_kernel_ms, int *kernels_per_call);

/* ---- diagnostics ---------------------------------------------------------------------- */
/* The tile plan the L-column kernels use: *num_tiles tiles of nominal *tile_items merge
 * items; `bounds` (nullable, num_tiles+1 entries) receives the boundary coordinates after
 * row snapping, *num_carries the number of boundaries a carry crosses.  Lets tests locate
 * exactly which rows are split between threads (those are within tolerance, the rest are
 * bit-identical to SpmvGold). */
MSPMV_API mspmv_status mspmv_tile_plan(mspmv_handle h, int L, int *num_tiles, int *tile_items, int *num_carries,
                                       mspmv_coord *bounds);
/* Single-RHS plan: how many tiles stream 16-bit column offsets (*tiles_cols16) and how many
 * gather x through a per-tile column dictionary (*tiles_dict: tiles whose scattered columns
 * make direct gathers line-bound; the sorted distinct columns are gathered once into LDS).
 * Either output may be null. */
MSPMV_API mspmv_status mspmv_tile_streams(mspmv_handle h, int *tiles_cols16, int *tiles_dict);
/* The L-column plan's tiles that carry a column dictionary (*tiles_dict).  L = 1: as
 * mspmv_tile_streams.  L = 16: the SpMM parks each such tile's distinct panel rows in LDS and
 * reads them there (row-group tiles with at most 64 distinct columns, each repeated >= 2
 * times on average); other widths build none (0). */
MSPMV_API mspmv_status mspmv_plan_dict_tiles(mspmv_handle h, int L, int *tiles_dict);
/* Tiles of the L-column plan staged by node blocks (*tiles_blk): runs of consecutive rows whose
 * column lists are prefixes of one list (FEM unknowns of one mesh node) read that list once and
 * gather each of its x entries once for all the run's rows.  Runs <= 64 columns wide are summed
 * in registers by a fixed lane tree (tile mode 255); wider ones go through the striped path's
 * LDS slots and reduction (bit-identical to it).  Tiles that hold whole rows only, <= 16 run
 * chunks, mean run height >= ~1.7 (others: 0). */
MSPMV_API mspmv_status mspmv_plan_block_tiles(mspmv_handle h, int L, int *tiles_blk);
/* Of those, the tiles with more than 8 run chunks (*tiles_two_rounds): the column-pair kernel takes
 * them in a second round of its eight half-wave run slots. */
MSPMV_API mspmv_status mspmv_plan_block_rounds(mspmv_handle h, int L, int *tiles_two_rounds);
/* The run chunks of the plan's register run tiles by how the column-pair SpMV reads their pattern
 * columns: from the chunk's 64-B record, as at most 12 runs of consecutive columns (*chunks_compact),
 * or, a pattern of more such runs, from its row of the 16-bit column stream (*chunks_escaped).  Both 0
 * for plans without node blocks. */
MSPMV_API mspmv_status mspmv_plan_block_records(mspmv_handle h, int L, int *chunks_compact, int *chunks_escaped);
/* Which layout forms the column-slab plan of the plain L-column product holds (L = 1: k_spmv_slab or
 * k_spmv_sell; L = 8, 16: k_spmm_slab), counted on the host while the plan was built.  *on_slab = 0 and
 * no counter written when that product runs on another plan.  stats[i], i < min(count,
 * MSPMV_SLAB_STAT_COUNT), receives counter i; counters of another kernel's forms are 0. */
enum mspmv_slab_stat {
    /* every slab plan */
    MSPMV_SLAB_STAT_BLOCKS = 0,
    MSPMV_SLAB_STAT_GROUPS,            /* column groups (1: blocks hold whole rows' nonzeros) */
    MSPMV_SLAB_STAT_UNITS,             /* chunks (k_spmv_slab, k_spmm_slab) or segments (k_spmv_sell) */
    MSPMV_SLAB_STAT_UNITS_MAX,         /* ... the most in one block (the block's LDS table) */
    MSPMV_SLAB_STAT_ROWS_MAX,          /* the most rows ending in one block */
    MSPMV_SLAB_STAT_EMPTY_BLOCKS,      /* blocks without a nonzero (an empty column group) */
    MSPMV_SLAB_STAT_CARRIES,           /* block boundaries a split row crosses */
    /* k_spmv_slab and k_spmm_slab */
    MSPMV_SLAB_STAT_CHUNKS_FULL,       /* chunks of exactly cfg.chunk nonzeros */
    MSPMV_SLAB_STAT_CHUNKS_ENTRY_CUT,  /* chunks ended by their cfg.entries-th run */
    MSPMV_SLAB_STAT_RUNS_CUT,          /* runs of one row cut by a chunk's end */
    MSPMV_SLAB_STAT_CHUNKS_LONG,       /* chunks with runs summed by whole waves (SpMV) */
    MSPMV_SLAB_STAT_LONG_RUNS_MAX,     /* ... the most such runs in one chunk */
    MSPMV_SLAB_STAT_LG0,               /* chunks by lanes_log2 of their short runs: LG0 + lg, lg = 0..6 */
    MSPMV_SLAB_STAT_SEGMENTS = MSPMV_SLAB_STAT_LG0 + 7, /* column segments (SpMM) */
    MSPMV_SLAB_STAT_SEGMENTS_MAX,      /* ... the most in one block */
    MSPMV_SLAB_STAT_SEGMENTS_FULL,     /* segments of exactly cfg.cols columns */
    MSPMV_SLAB_STAT_SEGMENTS_RAGGED,   /* segments whose columns x L / 2 is no multiple of 64 (a partial DMA piece) */
    /* k_spmv_sell: slices of short runs by form */
    MSPMV_SLAB_STAT_PACK_8X1,          /* packed, K runs x slots: 8 x 1, 4 x 2, 2 x 3, 2 x 4 */
    MSPMV_SLAB_STAT_PACK_4X2,
    MSPMV_SLAB_STAT_PACK_2X3,
    MSPMV_SLAB_STAT_PACK_2X4,
    MSPMV_SLAB_STAT_PACK_1X5,          /* packed plans' slices of one run per lane: PACK_1X5 + slots - 5, slots = 5..8 */
    MSPMV_SLAB_STAT_UNPACKED_1 = MSPMV_SLAB_STAT_PACK_1X5 + 4, /* unpacked: UNPACKED_1 + slots - 1, slots = 1..8 */
    MSPMV_SLAB_STAT_MEDIUM_2 = MSPMV_SLAB_STAT_UNPACKED_1 + 8, /* medium slices: MEDIUM_2 + slots - 2, slots = 2..8 */
    MSPMV_SLAB_STAT_SLICES_ODD = MSPMV_SLAB_STAT_MEDIUM_2 + 7, /* slices with an odd slot count (a lone last slot) */
    MSPMV_SLAB_STAT_SLICES_PARTIAL,    /* slices holding fewer runs than they have places */
    MSPMV_SLAB_STAT_LONG_1,            /* long runs of one piece, of two, of three or more */
    MSPMV_SLAB_STAT_LONG_2,
    MSPMV_SLAB_STAT_LONG_3PLUS,
    MSPMV_SLAB_STAT_PIECES_MAX,        /* the most long-run pieces in one segment */
    MSPMV_SLAB_STAT_SEGS_PIECES_ONLY,  /* segments with pieces and no slice */
    MSPMV_SLAB_STAT_SEGS_REFILL,       /* segments of < 16 slices followed in their block by one of > 16 */
    MSPMV_SLAB_STAT_PACKED_ROW_MAX,    /* the largest local row in a packed 16-bit run word */
    MSPMV_SLAB_STAT_COUNT
};
MSPMV_API mspmv_status mspmv_slab_plan_stats(mspmv_handle h, int L, long long *stats, int count, int *on_slab);
/* Host-only test hooks on the record's codec, no device needed.  Encode: a pattern of wc (0..64)
 * sorted distinct 16-bit column offsets into entries[12] (start | len << 16 | prefix << 24 per run of
 * consecutive columns, unused entries 0); *escaped = 1 and no entry when there are more than 12 runs.
 * Decode: the offset at pattern position q (>= 0) of a whole record (16 dwords: the descriptor, whose
 * dword 0 holds wc in bits 24-31, then the 12 entries); positions >= wc give that of wc - 1, an
 * all-zero record 0. */
MSPMV_API mspmv_status mspmv_block_record_encode(const unsigned short *offsets, int wc, unsigned *entries,
                                                 int *escaped);
MSPMV_API mspmv_status mspmv_block_record_decode(const unsigned *record, int q, unsigned *offset);
/* Each tile's in-tile reduction for L right-hand sides (num_tiles entries; 255 = a node-block
 * tile summed in registers by a fixed lane tree, see mspmv_plan_block_tiles): 0 = merge walk
 * (one walker per thread, or per L/2 lanes), g > 0 = row groups with 2^(g-1) nonzero-parallel
 * lanes per row (times L/2 column-pair lanes for L > 1).  g = 1 sums each row sequentially in
 * CSR order -> bit-identical to SpmvGold / the row-split SpMM for rows the tile holds whole. */
MSPMV_API mspmv_status mspmv_tile_modes(mspmv_handle h, int L, unsigned char *modes);
/* Threads that share one tile of the plan the plain L-column product runs on (*lanes): 256, or 64
 * for a single-RHS matrix whose rows are skewed (most workgroup tiles would be merge walks), which
 * the plain SpMV runs on one-wave tiles of 512 merge items.  A merge-walk tile gives each of its
 * lanes (L = 1) ceil(items / lanes) consecutive merge items -- what mspmv_tile_plan's readers
 * need to tell the rows summed sequentially from the split ones. */
MSPMV_API mspmv_status mspmv_tile_lanes(mspmv_handle h, int L, int *lanes);
/* Offset windows (host planning only, no device needed): whether a CSR matrix fits the plan the plain
 * SpMV takes by default for structured-grid rows -- 64-row windows, each keeping the offsets col - row
 * that at least 8 of its rows hold (all rows when it has fewer; <= 64 offsets, the most frequent),
 * dropping its rarest while its kept entries fill less than min_window_fill of rows x offsets; every
 * other entry goes to the plan's remainder (summed after the row's offsets).  Every row's columns
 * must ascend strictly.  The plan holds when the kept entries fill >= min_fill of the
 * windows' 64 x sum K slots and the remainder is at most 5 % of the nonzeros (any share when min_fill
 * is 0: the forced plan).  The library's automatic choice uses 0.85 / 0.30.  *ok = 1 when the plan
 * holds; then *num_windows = ceil(m / 64), *sum_offsets = the offsets over all windows,
 * *masked_windows = windows where some row lacks a kept offset (or that hold fewer than 64 rows),
 * *remainder (nullable) = the remainder's entries; k_per_window (nullable, num_windows entries)
 * receives each window's offset count.  Outputs other than *ok are 0 when the plan does not hold. */
MSPMV_API mspmv_status mspmv_offset_windows(const mspmv_csr_d *a, double min_fill, double min_window_fill, int *ok,
                                            int *num_windows, long long *sum_offsets, int *masked_windows,
                                            int *k_per_window, long long *remainder);
/* Diagnostic (the small-matrix SpMV's per-tile phases): one plain SpMV y = A x on device
 * vectors through the stamped instantiation of the merge-tile kernel k_spmv_tile, whose thread 0 records
 * wall_clock64() (a constant 100 MHz clock) per tile: stamps[t * 6 + i], i = 0 entry, 1 stream and x
 * gathers issued, 2 staged products in LDS (stream and gathers landed), 3 row ends in LDS, 4 rows reduced
 * and stored, 5 the HW_ID register of the CU that ran it.  flush_bytes > 0: the cold protocol's read
 * sweep of that many bytes first (as mspmv_time_spmm_dev).  stamps NULL: only *num_tiles.
 * MSPMV_ERR_UNSUPPORTED when the matrix's plain SpMV runs another kernel (node blocks, windows, slabs,
 * one-wave tiles).  No reference counterpart. */
MSPMV_API mspmv_status mspmv_spmv_tile_stamps(mspmv_handle h, const double *d_x, double *d_y, size_t flush_bytes,
                                              unsigned long long *stamps, int *num_tiles);
/* The single-RHS SpMV kernel instantiation launched for this matrix (tuning read once from
 * the MSPMV_SPMV_* environment; nontemporal matrix loads for a handle without a cache lease), e.g.
 * "k_spmv_tile<8,0,true>" -- the name rocprofv3 reports.  Valid until the next call on this
 * thread. */
MSPMV_API const char *mspmv_spmv_kernel_name(mspmv_handle h);
/* The same for a plain SpMM with L right-hand sides (builds the plan for L if needed): e.g.
 * "k_spmm_blk<16,0,false,6>" on a node-block plan, "k_spmm_tile<8,16,0,true>" elsewhere; widths
 * outside 1, 2, 4, 8, 16 name their widest column chunk's kernel.  "" on error. */
MSPMV_API const char *mspmv_spmm_kernel_name(mspmv_handle h, int L);
/* The CG path the last solve on this handle ran: "k_cg_resident<RPT,NZR> x G" (single RHS, the
 * matrix register/LDS-resident on every CU, one cooperative launch per solve), "pipelined (...)"
 * (single RHS, two kernels per iteration), or the split multi-RHS / PCG forms.  "" before any. */
MSPMV_API const char *mspmv_cg_kernel_name(mspmv_handle h);
/* The kernel instantiation the two products of the last BiCGSTAB / ILU(0)-BiCGSTAB solve on this handle ran, in
 * rocprofv3's spelling: "k_spmm_dia<L,nt>" (offset windows), "k_spmm_slab<cfg,nt>" (column slabs, L = 8 / 16),
 * "k_spmm_blk<L,0,nt,KR>" (node blocks), "k_spmm_tile<L,ipt,0,nt,dict,carries>" (merge tiles; carries: rows split
 * across tiles), and for L = 1 off the windows "k_spmv_tile<...>" / "k_spmv_blk<...>".  It is the solver's own
 * choice, which mspmv_spmm_kernel_name does not report: a solver never multiplies on the plain SpMV's one-wave,
 * sliced-ELL or run-balanced plans.  For a width outside 1, 2, 4, 8, 16 it names the last column group's kernel.
 * "" before any such solve.  Read-only: it changes no launch.  Valid until the next solve on the handle. */
MSPMV_API const char *mspmv_solver_product_kernel_name(mspmv_handle h);
/* The launch shape of the streaming solver passes (the split CG's, BiCGSTAB's, the block CG's) for panels of native
 * width L on this handle: *pass_blocks = workgroups per pass (their folds run one level per factor of 32 blocks; the
 * count depends on rows x L alone, never on a CU limit), *batch_iters = iterations per batch, which is also the
 * length of the cached iteration graph (a solve of fewer iterations runs ungraphed).  Either may be null.
 * Read-only: it changes no launch. */
MSPMV_API mspmv_status mspmv_solver_pass_shape(mspmv_handle h, int L, int *pass_blocks, int *batch_iters);

/* ---- fault detection ----------------------------------------------------------------- */
/* The kernels' cross-workgroup folds (CG dot products, rows split between tiles, column groups) are
 * closed by the last arrival on a self-resetting ticket.  An arrival that draws past its group (the
 * ticket was not 0 when the launch began) raises a fault word.  CG solves return MSPMV_ERR_FAULT
 * themselves; for products, the host-pointer calls check after their copy-back and *_dev callers
 * call this: it synchronizes the handle's stream, clears the word and returns MSPMV_ERR_FAULT if any
 * product since the last check raised it.  No reference counterpart (OpenMP reductions need none). */
MSPMV_API mspmv_status mspmv_check_faults(mspmv_handle h);
/* Test hook: the next CG solve on h fills its fold tickets with `value` after its init, before its first
 * iteration (MSPMV_POISON_FILL), optionally zeroes them again after the first iteration is enqueued
 * (MSPMV_POISON_LATE_ZERO: the ordering of round 5's unordered null-stream memset) and optionally
 * records the fault without stopping (MSPMV_POISON_NO_STOP: the solve runs to its stop test and then
 * returns MSPMV_ERR_FAULT with the iteration count it reached).  One solve only.  A pending
 * MSPMV_POISON_FILL is also taken by h's next product in mspmv_spmm_batch_dev when its plan splits rows
 * between tiles: that product starts from split-row tickets of `value` (zeroed again behind it) and
 * mspmv_sync_batch reports it. */
enum { MSPMV_POISON_FILL = 1, MSPMV_POISON_LATE_ZERO = 2, MSPMV_POISON_NO_STOP = 4 };
MSPMV_API mspmv_status mspmv_test_poison_tickets(mspmv_handle h, unsigned value, int flags);

/* ---- device memory helpers (so hosts need no HIP headers) ---------------------------- */
MSPMV_API mspmv_status mspmv_device_malloc(int device, size_t bytes, void **d_ptr);
MSPMV_API mspmv_status mspmv_device_free(void *d_ptr);
MSPMV_API mspmv_status mspmv_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes);
MSPMV_API mspmv_status mspmv_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes);
MSPMV_API mspmv_status mspmv_memcpy_d2d(void *d_dst, const void *d_src, size_t bytes);
MSPMV_API mspmv_status mspmv_memset_dev(void *d_dst, int byte_value, size_t bytes);

#ifdef __cplusplus
}
#endif

#endif /* MSPMV_H */

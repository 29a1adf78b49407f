// mspmv.hpp -- header-only C++ facade with the reference's own names and signatures over the
// C-ABI in mspmv.h (libmspmv.so).  Two ways to use it:
//
// 1. Namespace mode (default): everything lives in namespace mspmv_ref and takes any type with
//    the CsrMatrix<double,int> fields (sparse_matrix.h:648-653):
//        mspmv_ref::OmpMergeCsrmv(t, a, a.row_offsets + 1, a.column_indices, a.values, x, y);
//        int it = mspmv_ref::CGSolveMultiple(a, B, X, L, max_iters, threshold, NONZERO_SPLIT, &errs);
//    Nothing is declared in the global namespace, so it can sit beside the reference's own
//    headers (e.g. cpu_spmv.cpp, which defines OmpMergeCsrmv / TestOmpMergeCsrmv itself, calls
//    mspmv_ref::TestOmpMergeCsrmv at :879).
//
// 2. Drop-in mode (include/mspmv_dropin.hpp, i.e. MSPMV_REPLACE_REFERENCE): included after
//    sparse_matrix.h / utils.h / work_2025/hyper_parameters.hpp and BEFORE the reference's
//    work_2025/main/*.hpp, it defines the reference's functions in the global namespace with
//    the reference's exact signatures (CsrMatrix<ValueT,OffsetT>&, SpmmKernel) and pre-defines
//    the include guards of the headers it replaces, so a driver's call sites AND its #include
//    lines stay unchanged (cpu_multicg.cpp, cpu_singlecg.cpp, verification/*).  Including a
//    replaced header first is a compile error (#error below); defining the same function twice
//    is one too -- the drop-in can never silently fall back to the CPU code.
//
// The matrix is uploaded to HBM on first use and cached per (array pointers, shape, device,
// sampled content fingerprint); it is treated as immutable afterwards, as every reference
// driver treats its CsrMatrix -- call mspmv_ref::release(a) after mutating a matrix in place.
// num_threads is accepted and ignored (the GPU decides).  The device is
// mspmv_ref::set_device() (thread-local; initially $MSPMV_DEVICE or 0).  Errors throw
// std::runtime_error with mspmv_last_error() (the reference exit()s instead); a CG breakdown
// (non-finite alpha in a column: that column frozen, the others solved) is not an error -- it
// is reported by mspmv_ref::last_status() == MSPMV_ERR_BREAKDOWN and one stderr line.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "mspmv.h"

namespace mspmv_ref {

// ---- configuration -------------------------------------------------------------------------
inline int &device_slot()
{
    static thread_local int d = [] {
        const char *e = std::getenv("MSPMV_DEVICE");
        return e ? std::atoi(e) : 0;
    }();
    return d;
}
inline void set_device(int device) { device_slot() = device; }
inline int device() { return device_slot(); }
// Status of the last CG call on this thread (MSPMV_OK or MSPMV_ERR_BREAKDOWN).
inline mspmv_status &last_status()
{
    static thread_local mspmv_status s = MSPMV_OK;
    return s;
}
// Test* harnesses print the reference's progress lines unless quiet (drop-in mode: g_quiet).
inline bool &quiet_slot()
{
    static thread_local bool q = true;
    return q;
}

namespace detail {

inline void check(mspmv_status s, const char *where)
{
    if (s != MSPMV_OK && s != MSPMV_ERR_BREAKDOWN)
        throw std::runtime_error(std::string(where) + ": " + mspmv_last_error());
}

inline void note_cg(mspmv_status s, const char *where)
{
    check(s, where);
    last_status() = s;
    if (s == MSPMV_ERR_BREAKDOWN)
        std::fprintf(stderr, "%s: %s\n", where, mspmv_last_error());
}

// Cache key of an uploaded matrix: its arrays, shape and device, plus a fingerprint of 64
// evenly spaced (row offset, column, value) samples -- a new matrix placed in freed buffers of
// the same shape is told apart from the one cached there.
struct Key {
    const void *ro, *ci, *va;
    long long m, n, nnz;
    int dev;
    unsigned long long fp;
    bool operator<(const Key &o) const
    {
        return std::tie(ro, ci, va, m, n, nnz, dev, fp) < std::tie(o.ro, o.ci, o.va, o.m, o.n, o.nnz, o.dev, o.fp);
    }
    bool same_arrays(const Key &o) const { return ro == o.ro && ci == o.ci && va == o.va; }
};

template <typename Csr>
Key key_of(const Csr &a)
{
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&](const void *p, size_t bytes) {
        const unsigned char *c = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < bytes; ++i)
            h = (h ^ c[i]) * 1099511628211ull;
    };
    const long long nnz = a.num_nonzeros, m = a.num_rows;
    for (int s = 0; s < 64 && nnz > 0; ++s) {
        const long long k = (nnz - 1) * s / 63;
        mix(&a.column_indices[k], sizeof(a.column_indices[k]));
        mix(&a.values[k], sizeof(a.values[k]));
    }
    for (int s = 0; s < 64 && m > 0; ++s)
        mix(&a.row_offsets[m * s / 63], sizeof(a.row_offsets[0]));
    return Key{a.row_offsets, a.column_indices, a.values, m, (long long)a.num_cols, nnz, device(), h};
}

inline std::map<Key, mspmv_handle> &handles()
{
    static std::map<Key, mspmv_handle> c;
    return c;
}
inline std::map<Key, mspmv_ic0> &factors()
{
    static std::map<Key, mspmv_ic0> c;
    return c;
}

inline std::map<Key, mspmv_ilu0> &ilu_factors()  // by the key of the matrix factored
{
    static std::map<Key, mspmv_ilu0> c;
    return c;
}

template <typename Csr>
mspmv_csr_d view(const Csr &a)
{
    static_assert(sizeof(*a.values) == 8 && sizeof(*a.row_offsets) == 4 && sizeof(*a.column_indices) == 4,
                  "mspmv: CsrMatrix<double,int> only");
    return mspmv_csr_d{(int)a.num_rows, (int)a.num_cols, (int)a.num_nonzeros, (const int *)a.row_offsets,
                       (const int *)a.column_indices, (const double *)a.values};
}

// Drop stale entries of the same arrays (same pointers, other shape or content): the buffers
// were reused for another matrix, whose handle replaces the old one.
template <typename V>
void evict_same_arrays(std::map<Key, V> &c, const Key &k, void (*destroy)(V))
{
    for (auto it = c.begin(); it != c.end();) {
        if (it->first.same_arrays(k) && it->first.dev == k.dev) {
            destroy(it->second);
            it = c.erase(it);
        } else {
            ++it;
        }
    }
}

template <typename Csr>
mspmv_handle handle_for(const Csr &a)
{
    const Key k = key_of(a);
    auto it = handles().find(k);
    if (it != handles().end())
        return it->second;
    evict_same_arrays<mspmv_handle>(handles(), k, [](mspmv_handle h) { (void)mspmv_destroy(h); });
    const mspmv_csr_d d = view(a);
    mspmv_handle h = nullptr;
    check(mspmv_csr_create(&d, device(), &h), "mspmv_csr_create");
    handles().emplace(k, h);
    return h;
}

template <typename Csr>
mspmv_ic0 ic0_for(const Csr &l)
{
    const Key k = key_of(l);
    auto it = factors().find(k);
    if (it != factors().end())
        return it->second;
    evict_same_arrays<mspmv_ic0>(factors(), k, [](mspmv_ic0 f) { (void)mspmv_ic0_destroy(f); });
    const mspmv_csr_d d = view(l);
    mspmv_ic0 f = nullptr;
    check(mspmv_ic0_create(&d, device(), &f), "mspmv_ic0_create");
    factors().emplace(k, f);
    return f;
}

// The ILU(0) factor of `a` itself (mspmv_ilu0_values on the host, then mspmv_ilu0_create), cached with it.
template <typename Csr>
mspmv_ilu0 ilu0_for(const Csr &a)
{
    const Key k = key_of(a);
    auto it = ilu_factors().find(k);
    if (it != ilu_factors().end())
        return it->second;
    evict_same_arrays<mspmv_ilu0>(ilu_factors(), k, [](mspmv_ilu0 f) { (void)mspmv_ilu0_destroy(f); });
    mspmv_csr_d d = view(a);
    std::vector<double> lu((size_t)std::max<long long>(a.num_nonzeros, 1));
    check(mspmv_ilu0_values(&d, lu.data()), "mspmv_ilu0_values");
    d.values = lu.data();
    mspmv_ilu0 f = nullptr;
    check(mspmv_ilu0_create(&d, device(), &f), "mspmv_ilu0_create");
    ilu_factors().emplace(k, f);
    return f;
}

// Device buffer (RAII) for the harnesses: inputs resident in HBM across timed repetitions.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    explicit DevBuf(size_t b) : bytes(b) { check(mspmv_device_malloc(device(), b ? b : 8, &p), "device_malloc"); }
    ~DevBuf() { (void)mspmv_device_free(p); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    void up(const void *h) { check(mspmv_memcpy_h2d(p, h, bytes), "memcpy_h2d"); }
    void down(void *h) const { check(mspmv_memcpy_d2h(h, p, bytes), "memcpy_d2h"); }
    double *d() const { return static_cast<double *>(p); }
};

// Arrays of an output CsrMatrix, allocated the way that container frees them (CsrMatrix::Clear,
// sparse_matrix.h:738-769: NUMA or mkl_malloc in the reference's CUB_MKL build, new[] otherwise).
template <typename Csr>
void csr_alloc(Csr &out, long long rows, long long cols, long long nnz)
{
    out.num_rows = (decltype(out.num_rows))rows;
    out.num_cols = (decltype(out.num_cols))cols;
    out.num_nonzeros = (decltype(out.num_nonzeros))nnz;
    using O = std::remove_reference_t<decltype(*out.row_offsets)>;
    using V = std::remove_reference_t<decltype(*out.values)>;
#if defined(MSPMV_REPLACE_REFERENCE) && defined(CUB_MKL)
    if (out.IsNumaMalloc()) {
        numa_set_strict(1);
        out.row_offsets = (O *)numa_alloc_onnode(sizeof(O) * (rows + 1), 0);
        out.column_indices = (O *)numa_alloc_onnode(sizeof(O) * nnz, 0);
        out.values = (V *)numa_alloc_onnode(sizeof(V) * nnz, numa_num_task_nodes() > 1 ? 1 : 0);
    } else {
        out.row_offsets = (O *)mkl_malloc(sizeof(O) * (rows + 1), 4096);
        out.column_indices = (O *)mkl_malloc(sizeof(O) * nnz, 4096);
        out.values = (V *)mkl_malloc(sizeof(V) * nnz, 4096);
    }
#else
    out.row_offsets = new O[rows + 1];
    out.column_indices = new O[nnz > 0 ? nnz : 1];
    out.values = new V[nnz > 0 ? nnz : 1];
#endif
}

template <typename F>
double wall_ms(F &&f)
{
    const auto t0 = std::chrono::steady_clock::now();
    f();
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace detail

// Forget the device copy (handle, IC(0) factor, or the ILU(0) factor computed from it) of a matrix: call
// after mutating it in place or before freeing it if its buffers will be reused.
template <typename Csr>
void release(const Csr &a)
{
    const detail::Key k = detail::key_of(a);
    detail::evict_same_arrays<mspmv_handle>(detail::handles(), k, [](mspmv_handle h) { (void)mspmv_destroy(h); });
    detail::evict_same_arrays<mspmv_ic0>(detail::factors(), k, [](mspmv_ic0 f) { (void)mspmv_ic0_destroy(f); });
    detail::evict_same_arrays<mspmv_ilu0>(detail::ilu_factors(), k, [](mspmv_ilu0 f) { (void)mspmv_ilu0_destroy(f); });
}
// The matrix's values were rewritten in place on the same pattern (a time step, a Newton iteration, a load
// case): refresh its cached device handle with mspmv_csr_update_values instead of release() + a new upload,
// so every plan built for it is kept.  The cache owns the handles, so this is the facade's UpdateValues; a
// matrix not uploaded yet is uploaded.  Factors computed from the old values (IC(0), ILU(0)) are dropped:
// they are not refreshed (mspmv.h) and are rebuilt on their next use.
template <typename Csr>
void UpdateValues(const Csr &a)
{
    const detail::Key k = detail::key_of(a);
    detail::evict_same_arrays<mspmv_ic0>(detail::factors(), k, [](mspmv_ic0 f) { (void)mspmv_ic0_destroy(f); });
    detail::evict_same_arrays<mspmv_ilu0>(detail::ilu_factors(), k, [](mspmv_ilu0 f) { (void)mspmv_ilu0_destroy(f); });
    auto &c = detail::handles();
    for (auto it = c.begin(); it != c.end(); ++it) {
        const detail::Key &o = it->first;
        if (o.same_arrays(k) && o.m == k.m && o.n == k.n && o.nnz == k.nnz && o.dev == k.dev) {
            const mspmv_handle h = it->second;
            detail::check(mspmv_csr_update_values(h, (const double *)a.values), "mspmv_csr_update_values");
            c.erase(it);
            c.emplace(k, h);  // under the new values' fingerprint
            return;
        }
    }
    (void)detail::handle_for(a);
}
inline void release_all()
{
    for (auto &e : detail::handles())
        (void)mspmv_destroy(e.second);
    for (auto &e : detail::factors())
        (void)mspmv_ic0_destroy(e.second);
    for (auto &e : detail::ilu_factors())
        (void)mspmv_ilu0_destroy(e.second);
    detail::handles().clear();
    detail::factors().clear();
    detail::ilu_factors().clear();
}

// ---- kernels ---------------------------------------------------------------------------------
// cpu_spmv.cpp:357-421 (row_end_offsets / column_indices / values are a's own arrays there)
template <typename Csr, typename OffsetT, typename ValueT>
void OmpMergeCsrmv(int /*num_threads*/, Csr &a, OffsetT * /*row_end_offsets*/, OffsetT * /*column_indices*/,
                   ValueT * /*values*/, ValueT *vector_x, ValueT *vector_y_out)
{
    detail::check(mspmv_dspmv(detail::handle_for(a), vector_x, vector_y_out), "mspmv_dspmv");
}

// work_2025/spmm/merge_based.hpp:46-153 (row-major n x num_vectors panels)
template <typename Csr, typename OffsetT, typename ValueT>
void OmpMergeCsrmm(int /*num_threads*/, Csr &a, OffsetT * /*row_end_offsets*/, OffsetT * /*column_indices*/,
                   ValueT * /*values*/, ValueT *vector_x, ValueT *vector_y_out, int num_vectors)
{
    detail::check(mspmv_dspmm(detail::handle_for(a), vector_x, vector_y_out, num_vectors), "mspmv_dspmm");
}

// work_2025/main/single_strategy.hpp:102-170
template <typename Csr, typename ValueT>
int CGSolveSingle(Csr &a, const ValueT *b, ValueT *x, int max_iters, ValueT tolerance)
{
    int iters = 0;
    detail::note_cg(mspmv_dcg_single(detail::handle_for(a), b, x, max_iters, tolerance, &iters, nullptr, 0),
                    "CGSolveSingle");
    return iters;
}

// work_2025/main/no_pretreatment.hpp:32-197.  kernel_type: any value convertible to int (the
// reference's SpmmKernel, work_2025/types.hpp:11-16); the GPU always runs its merge-path SpMM.
template <typename Csr, typename ValueT, typename KernelT>
int CGSolveMultiple(Csr &a, const ValueT *B, ValueT *X, int num_vectors, int max_iters, ValueT tolerance,
                    KernelT kernel_type, std::vector<double> *max_errors = nullptr)
{
    int iters = 0;
    std::vector<double> hist(max_errors ? (size_t)std::max(max_iters, 0) : 0);
    detail::note_cg(mspmv_dcg_multi(detail::handle_for(a), B, X, num_vectors, max_iters, tolerance,
                                    (mspmv_spmm_kernel)(int)kernel_type, &iters, max_errors ? hist.data() : nullptr,
                                    max_errors ? max_iters : 0),
                    "CGSolveMultiple");
    if (max_errors)
        max_errors->assign(hist.begin(), hist.begin() + std::min<size_t>(hist.size(), (size_t)iters));
    return iters;
}

// Multi-RHS BiCGSTAB for a square matrix that need not be symmetric (mspmv_dbicgstab_multi), in
// CGSolveMultiple's calling form.  No reference counterpart: every solver of the reference is a CG.
template <typename Csr, typename ValueT>
int BiCGStabSolveMultiple(Csr &a, const ValueT *B, ValueT *X, int num_vectors, int max_iters, ValueT tolerance,
                          std::vector<double> *max_errors = nullptr)
{
    int iters = 0;
    std::vector<double> hist(max_errors ? (size_t)std::max(max_iters, 0) : 0);
    detail::note_cg(mspmv_dbicgstab_multi(detail::handle_for(a), B, X, num_vectors, max_iters, tolerance, &iters,
                                          max_errors ? hist.data() : nullptr, max_errors ? max_iters : 0),
                    "BiCGStabSolveMultiple");
    if (max_errors)
        max_errors->assign(hist.begin(), hist.begin() + std::min<size_t>(hist.size(), (size_t)iters));
    return iters;
}

// The same right-preconditioned with the ILU(0) factor of `a` (mspmv_dpbicgstab_ilu0_multi); the factor is
// computed on the first call and cached with the matrix's handle.  No reference counterpart.
template <typename Csr, typename ValueT>
int ILU0BiCGStabSolveMultiple(Csr &a, const ValueT *B, ValueT *X, int num_vectors, int max_iters, ValueT tolerance,
                              std::vector<double> *max_errors = nullptr)
{
    int iters = 0;
    std::vector<double> hist(max_errors ? (size_t)std::max(max_iters, 0) : 0);
    detail::note_cg(mspmv_dpbicgstab_ilu0_multi(detail::handle_for(a), detail::ilu0_for(a), B, X, num_vectors,
                                                max_iters, tolerance, &iters, max_errors ? hist.data() : nullptr,
                                                max_errors ? max_iters : 0),
                    "ILU0BiCGStabSolveMultiple");
    if (max_errors)
        max_errors->assign(hist.begin(), hist.begin() + std::min<size_t>(hist.size(), (size_t)iters));
    return iters;
}

// work_2025/cg/incomplete_cholesky_decomp.hpp:11-78 (host: setup, as in the reference)
template <typename Csr>
void TransposeCsr(const Csr &in, Csr &out)
{
    detail::csr_alloc(out, in.num_cols, in.num_rows, in.num_nonzeros);
    const mspmv_csr_d d = detail::view(in);
    detail::check(mspmv_csr_transpose(&d, (int *)out.row_offsets, (int *)out.column_indices, (double *)out.values),
                  "mspmv_csr_transpose");
}

// work_2025/cg/sparse_approximate_inversion.hpp:40-321: m receives A's pattern and the SPAI values.
template <typename Csr>
bool SparseApproximateInversion(const Csr &a, Csr &m)
{
    detail::csr_alloc(m, a.num_rows, a.num_cols, a.num_nonzeros);
    std::copy(a.row_offsets, a.row_offsets + a.num_rows + 1, m.row_offsets);
    std::copy(a.column_indices, a.column_indices + a.num_nonzeros, m.column_indices);
    const mspmv_csr_d d = detail::view(a);
    detail::check(mspmv_spai_values(&d, (double *)m.values), "mspmv_spai_values");
    return true;
}

// work_2025/cg/incomplete_cholesky_decomp.hpp:84-201: l receives L; false when the factorization
// fails after its 20 shifted attempts (l is then left empty, as the reference leaves it unusable).
template <typename Csr>
bool IncompleteCholesky(const Csr &a, Csr &l)
{
    const mspmv_csr_d d = detail::view(a);
    int nz = 0;
    detail::check(mspmv_ic0_nnz(&d, &nz), "mspmv_ic0_nnz");
    detail::csr_alloc(l, a.num_rows, a.num_cols, nz);
    return mspmv_ic0_factor(&d, (int *)l.row_offsets, (int *)l.column_indices, (double *)l.values, nullptr) ==
           MSPMV_OK;
}

// work_2025/main/incomplete_cholesky.hpp:33-199 (l_transpose accepted for the signature; the
// device factor holds its own transpose).  The factor is uploaded once and cached like A.
template <typename Csr, typename ValueT, typename KernelT>
int PCGSolveMultiple(Csr &a, const Csr &l, const Csr & /*l_transpose*/, const ValueT *B, ValueT *X, int num_vectors,
                     int max_iters, ValueT tolerance, KernelT kernel_type, std::vector<double> *max_errors = nullptr)
{
    int iters = 0;
    std::vector<double> hist(max_errors ? (size_t)std::max(max_iters, 0) : 0);
    detail::note_cg(mspmv_dpcg_ic0_multi(detail::handle_for(a), detail::ic0_for(l), B, X, num_vectors, max_iters,
                                         tolerance, (mspmv_spmm_kernel)(int)kernel_type, &iters,
                                         max_errors ? hist.data() : nullptr, max_errors ? max_iters : 0),
                    "PCGSolveMultiple");
    if (max_errors)
        max_errors->assign(hist.begin(), hist.begin() + std::min<size_t>(hist.size(), (size_t)iters));
    return iters;
}

// work_2025/main/sparse_approximate_inverse.hpp:30-230
template <typename Csr, typename ValueT, typename KernelT>
int SPAISolveMultiple(Csr &a, Csr &m, const ValueT *B, ValueT *X, int num_vectors, int max_iters, ValueT tolerance,
                      KernelT kernel_type, std::vector<double> *max_errors = nullptr)
{
    int iters = 0;
    std::vector<double> hist(max_errors ? (size_t)std::max(max_iters, 0) : 0);
    detail::note_cg(mspmv_dpcg_spai_multi(detail::handle_for(a), detail::handle_for(m), B, X, num_vectors, max_iters,
                                          tolerance, (mspmv_spmm_kernel)(int)kernel_type, &iters,
                                          max_errors ? hist.data() : nullptr, max_errors ? max_iters : 0),
                    "SPAISolveMultiple");
    if (max_errors)
        max_errors->assign(hist.begin(), hist.begin() + std::min<size_t>(hist.size(), (size_t)iters));
    return iters;
}

// ---- initial guess (warm start; no reference counterpart: every solver of the reference starts from 0) ----
// While an InitialGuess(a) lives, every solver above called with `a` as the matrix reads X on entry as X0
// (mspmv_set_initial_guess, MSPMV_X0_CALLER: stop test still relative to ||B||, iterations counted from X0, a column
// already below the tolerance returned untouched); the handle's previous mode comes back when it goes.
template <typename Csr>
class InitialGuess {
    mspmv_handle h_;
    int old_ = MSPMV_X0_ZERO;

public:
    explicit InitialGuess(Csr &a) : h_(detail::handle_for(a))
    {
        detail::check(mspmv_set_initial_guess(h_, MSPMV_X0_CALLER, &old_), "mspmv_set_initial_guess");
    }
    ~InitialGuess() { (void)mspmv_set_initial_guess(h_, old_, nullptr); }
    InitialGuess(const InitialGuess &) = delete;
    InitialGuess &operator=(const InitialGuess &) = delete;
};
// ... or per call: the solvers' overloads that take the tag from_x after their reference arguments, e.g.
//     CGSolveMultiple(a, B, X, L, max_iters, tol, NONZERO_SPLIT, mspmv_ref::from_x, &errs);
struct from_x_t {};
constexpr from_x_t from_x{};

template <typename Csr, typename ValueT>
int CGSolveSingle(Csr &a, const ValueT *b, ValueT *x, int max_iters, ValueT tolerance, from_x_t)
{
    InitialGuess<Csr> guess(a);
    return CGSolveSingle(a, b, x, max_iters, tolerance);
}
template <typename Csr, typename ValueT, typename KernelT>
int CGSolveMultiple(Csr &a, const ValueT *B, ValueT *X, int num_vectors, int max_iters, ValueT tolerance,
                    KernelT kernel_type, from_x_t, std::vector<double> *max_errors = nullptr)
{
    InitialGuess<Csr> guess(a);
    return CGSolveMultiple(a, B, X, num_vectors, max_iters, tolerance, kernel_type, max_errors);
}
template <typename Csr, typename ValueT>
int BiCGStabSolveMultiple(Csr &a, const ValueT *B, ValueT *X, int num_vectors, int max_iters, ValueT tolerance,
                          from_x_t, std::vector<double> *max_errors = nullptr)
{
    InitialGuess<Csr> guess(a);
    return BiCGStabSolveMultiple(a, B, X, num_vectors, max_iters, tolerance, max_errors);
}
template <typename Csr, typename ValueT>
int ILU0BiCGStabSolveMultiple(Csr &a, const ValueT *B, ValueT *X, int num_vectors, int max_iters, ValueT tolerance,
                              from_x_t, std::vector<double> *max_errors = nullptr)
{
    InitialGuess<Csr> guess(a);
    return ILU0BiCGStabSolveMultiple(a, B, X, num_vectors, max_iters, tolerance, max_errors);
}
template <typename Csr, typename ValueT, typename KernelT>
int PCGSolveMultiple(Csr &a, const Csr &l, const Csr &l_transpose, const ValueT *B, ValueT *X, int num_vectors,
                     int max_iters, ValueT tolerance, KernelT kernel_type, from_x_t,
                     std::vector<double> *max_errors = nullptr)
{
    InitialGuess<Csr> guess(a);
    return PCGSolveMultiple(a, l, l_transpose, B, X, num_vectors, max_iters, tolerance, kernel_type, max_errors);
}
template <typename Csr, typename ValueT, typename KernelT>
int SPAISolveMultiple(Csr &a, Csr &m, const ValueT *B, ValueT *X, int num_vectors, int max_iters, ValueT tolerance,
                      KernelT kernel_type, from_x_t, std::vector<double> *max_errors = nullptr)
{
    InitialGuess<Csr> guess(a);
    return SPAISolveMultiple(a, m, B, X, num_vectors, max_iters, tolerance, kernel_type, max_errors);
}

// ---- the reference's timing harnesses --------------------------------------------------------
// cpu_spmv.cpp:426-475.  Correctness call into vector_y_out (pre-filled with 0xff bytes, as the
// reference's memset(-1)), then timing_iterations warm and timing_iterations timed SpMVs with x
// and y resident in HBM (HIP events on the handle's stream: the device-memory counterpart of
// the reference timing its in-memory loop); returns the average ms per SpMV.  setup_ms receives
// the upload + partition time of the matrix (0 in the reference, whose partition is per call).
template <typename Csr, typename ValueT>
float TestOmpMergeCsrmv(Csr &a, ValueT *vector_x, ValueT *reference_vector_y_out, ValueT *vector_y_out,
                        int timing_iterations, float &setup_ms)
{
    (void)reference_vector_y_out;  // compared by the drop-in wrapper (CompareResults, utils.h)
    mspmv_handle h = detail::handle_for(a);
    setup_ms = (float)mspmv_setup_ms(h);
    std::memset(vector_y_out, -1, sizeof(ValueT) * (size_t)a.num_rows);
    detail::check(mspmv_dspmv(h, vector_x, vector_y_out), "mspmv_dspmv");
    if (timing_iterations <= 0)
        return 0.0f;
    detail::DevBuf dx(sizeof(ValueT) * (size_t)a.num_cols), dy(sizeof(ValueT) * (size_t)a.num_rows);
    dx.up(vector_x);
    double ms = 0.0;
    detail::check(mspmv_time_spmm_dev(h, dx.d(), dy.d(), 1, timing_iterations, 0, &ms), "mspmv_time_spmm_dev");
    detail::check(mspmv_time_spmm_dev(h, dx.d(), dy.d(), 1, timing_iterations, 0, &ms), "mspmv_time_spmm_dev");
    return (float)ms;
}

// work_2025/main/single_strategy.hpp:176-240: num_vectors column blocks b_vectors[v*n ..] solved
// one after another per timed run (its warmup loop breaks at once, :197-199); min wall time over
// timing_iterations runs and the total iterations of that run.  B and X stay in HBM across runs.
template <typename Csr, typename ValueT>
void TestCGSolveSingle(Csr &a, ValueT *b_vectors, ValueT *x_solutions, int max_iters, ValueT tolerance,
                       int num_vectors, int timing_iterations, double &min_ms, double &iters_of_min_ms)
{
    mspmv_handle h = detail::handle_for(a);
    const size_t n = (size_t)a.num_rows, bytes = sizeof(ValueT) * n * (size_t)std::max(num_vectors, 0);
    detail::DevBuf dB(bytes), dX(bytes);
    dB.up(b_vectors);
    min_ms = std::numeric_limits<double>::max();
    iters_of_min_ms = 0;
    for (int it = 0; it < timing_iterations; ++it) {
        long long total = 0;
        mspmv_status worst = MSPMV_OK;
        const double ms = detail::wall_ms([&] {
            for (int v = 0; v < num_vectors; ++v) {
                int k = 0;
                const mspmv_status s = mspmv_dcg_single_dev(h, dB.d() + v * n, dX.d() + v * n, max_iters, tolerance,
                                                            &k, nullptr, 0);
                detail::check(s, "mspmv_dcg_single_dev");
                worst = s != MSPMV_OK ? s : worst;
                total += k;
            }
        });
        last_status() = worst;
        if (!quiet_slot())
            std::printf("\tTime: %.3f ms (Total Iters: %lld)\n", ms, total);
        if (ms < min_ms) {
            min_ms = ms;
            iters_of_min_ms = (double)total;
        }
    }
    dX.down(x_solutions);
}

namespace detail {
// The multi-RHS harnesses (no_pretreatment.hpp:202-256, incomplete_cholesky.hpp:205-257,
// sparse_approximate_inverse.hpp:232-288): `warmups` untimed solves, then timing_iterations timed
// solves; the max-error history is recorded on the first timed run only; min wall ms and its
// iteration count.  `solve(dB, dX, hist, cap, &iters)` runs one solve on device buffers.
template <typename ValueT, typename Solve>
void multi_harness(size_t n, int num_vectors, ValueT *b_vectors, ValueT *x_solutions, int max_iters, int warmups,
                   int timing_iterations, double &min_ms, double &iters_of_min_ms, std::vector<double> *max_errors,
                   const char *where, Solve &&solve)
{
    const size_t bytes = sizeof(ValueT) * n * (size_t)std::max(num_vectors, 0);
    DevBuf dB(bytes), dX(bytes);
    dB.up(b_vectors);
    for (int it = 0; it < warmups; ++it) {
        if (!quiet_slot())
            std::printf("Warmup iteration %d/%d\n", it + 1, warmups);
        int k = 0;
        check(solve(dB.d(), dX.d(), nullptr, 0, &k), where);
    }
    min_ms = std::numeric_limits<double>::max();
    iters_of_min_ms = 0;
    std::vector<double> hist;
    for (int it = 0; it < timing_iterations; ++it) {
        if (!quiet_slot())
            std::printf("Timed iteration %d/%d\n", it + 1, timing_iterations);
        const bool rec = it == 0 && max_errors;
        if (rec)
            hist.assign((size_t)std::max(max_iters, 1), 0.0);
        int k = 0;
        mspmv_status s = MSPMV_OK;
        const double ms = wall_ms([&] { s = solve(dB.d(), dX.d(), rec ? hist.data() : nullptr, rec ? max_iters : 0, &k); });
        note_cg(s, where);
        if (rec)
            max_errors->assign(hist.begin(), hist.begin() + std::min<size_t>(hist.size(), (size_t)k));
        if (!quiet_slot())
            std::printf("\tTime: %.3f ms (%d iterations)\n", ms, k);
        if (ms < min_ms) {
            min_ms = ms;
            iters_of_min_ms = k;
        }
    }
    dX.down(x_solutions);
}
}  // namespace detail

// work_2025/main/no_pretreatment.hpp:202-256 (timing_iterations warmups, then timed runs)
template <typename Csr, typename ValueT, typename KernelT>
void TestCGMultipleRHS(Csr &a, ValueT *b_vectors, ValueT *x_solutions, int max_iters, ValueT tolerance,
                       int num_vectors, int timing_iterations, KernelT kernel_type, double &min_ms,
                       double &iters_of_min_ms, std::vector<double> *max_errors = nullptr)
{
    mspmv_handle h = detail::handle_for(a);
    detail::multi_harness(
        (size_t)a.num_rows, num_vectors, b_vectors, x_solutions, max_iters, timing_iterations, timing_iterations,
        min_ms, iters_of_min_ms, max_errors, "TestCGMultipleRHS",
        [&](const double *dB, double *dX, double *hist, int cap, int *k) {
            return mspmv_dcg_multi_dev(h, dB, dX, num_vectors, max_iters, tolerance,
                                       (mspmv_spmm_kernel)(int)kernel_type, k, hist, cap);
        });
}

// work_2025/main/incomplete_cholesky.hpp:205-257
template <typename Csr, typename ValueT, typename KernelT>
void TestPCGMultipleRHS(Csr &a, const Csr &l, const Csr & /*l_transpose*/, ValueT *b_vectors, ValueT *x_solutions,
                        int max_iters, ValueT tolerance, int num_vectors, int timing_iterations, KernelT kernel_type,
                        double &min_ms, double &iters_of_min_ms, std::vector<double> *max_errors = nullptr)
{
    mspmv_handle h = detail::handle_for(a);
    mspmv_ic0 f = detail::ic0_for(l);
    detail::multi_harness(
        (size_t)a.num_rows, num_vectors, b_vectors, x_solutions, max_iters, timing_iterations, timing_iterations,
        min_ms, iters_of_min_ms, max_errors, "TestPCGMultipleRHS",
        [&](const double *dB, double *dX, double *hist, int cap, int *k) {
            return mspmv_dpcg_ic0_multi_dev(h, f, dB, dX, num_vectors, max_iters, tolerance,
                                            (mspmv_spmm_kernel)(int)kernel_type, k, hist, cap);
        });
}

// work_2025/main/sparse_approximate_inverse.hpp:232-288 (its warmup solve is commented out there:
// no warmups here either)
template <typename Csr, typename ValueT, typename KernelT>
void TestCGMultipleSPAI(Csr &a, Csr &m, ValueT *b_vectors, ValueT *x_solutions, int max_iters, ValueT tolerance,
                        int num_vectors, int timing_iterations, KernelT kernel_type, double &min_ms,
                        double &iters_of_min_ms, std::vector<double> *max_errors = nullptr)
{
    mspmv_handle h = detail::handle_for(a), hm = detail::handle_for(m);
    detail::multi_harness(
        (size_t)a.num_rows, num_vectors, b_vectors, x_solutions, max_iters, 0, timing_iterations, min_ms,
        iters_of_min_ms, max_errors, "TestCGMultipleSPAI",
        [&](const double *dB, double *dX, double *hist, int cap, int *k) {
            return mspmv_dpcg_spai_multi_dev(h, hm, dB, dX, num_vectors, max_iters, tolerance,
                                             (mspmv_spmm_kernel)(int)kernel_type, k, hist, cap);
        });
}

}  // namespace mspmv_ref

// ------------------------------------------------------------------------------------------------
// Drop-in mode: the reference's names, exact signatures, in the global namespace.
// ------------------------------------------------------------------------------------------------
#ifdef MSPMV_REPLACE_REFERENCE
#if defined(NO_PRETREATMENT_HPP) || defined(SINGLE_STRATEGY_HPP) || defined(INCOMPLETE_CHOLESKY_HPP) ||          \
    defined(SPARSE_APPROXIMATE_INVERSE_HPP) || defined(INCOMPLETE_CHOLESKY_DECOMP_HPP) ||                          \
    defined(SPARSE_MATRIX_LINEAR_EQUATIONS_CPU_MULTICG_HPP) || defined(MERGE_BASED_HPP)
#error "mspmv_dropin.hpp replaces work_2025/main/*.hpp, work_2025/cg/{incomplete_cholesky_decomp,sparse_approximate_inversion}.hpp and work_2025/spmm/merge_based.hpp: include it before them"
#endif
#ifndef HYPER_PARAMETERS_HPP
#error "mspmv_dropin.hpp: include sparse_matrix.h, utils.h and work_2025/hyper_parameters.hpp first"
#endif
#if __has_include("work_2025/types.hpp")
#include "work_2025/types.hpp"  // SpmmKernel (pulled in by the headers replaced below)
#endif
// The replaced headers become empty if a driver includes them afterwards.
#define NO_PRETREATMENT_HPP
#define SINGLE_STRATEGY_HPP
#define INCOMPLETE_CHOLESKY_HPP
#define SPARSE_APPROXIMATE_INVERSE_HPP
#define INCOMPLETE_CHOLESKY_DECOMP_HPP
#define SPARSE_MATRIX_LINEAR_EQUATIONS_CPU_MULTICG_HPP  // work_2025/cg/sparse_approximate_inversion.hpp
#define MERGE_BASED_HPP

namespace mspmv_ref {
inline bool dropin_quiet()
{
    quiet_slot() = g_quiet;  // hyper_parameters.hpp:8
    return g_quiet;
}
}  // namespace mspmv_ref

// cpu_spmv.cpp:357-421
template <typename ValueT, typename OffsetT>
void OmpMergeCsrmv(int num_threads, CsrMatrix<ValueT, OffsetT> &a, OffsetT *row_end_offsets, OffsetT *column_indices,
                   ValueT *values, ValueT *vector_x, ValueT *vector_y_out)
{
    mspmv_ref::OmpMergeCsrmv(num_threads, a, row_end_offsets, column_indices, values, vector_x, vector_y_out);
}

// cpu_spmv.cpp:426-475, with the reference's PASS/FAIL line (CompareResults, utils.h:710-733)
template <typename ValueT, typename OffsetT>
float TestOmpMergeCsrmv(CsrMatrix<ValueT, OffsetT> &a, ValueT *vector_x, ValueT *reference_vector_y_out,
                        ValueT *vector_y_out, int timing_iterations, float &setup_ms)
{
    const bool q = mspmv_ref::dropin_quiet();
    if (!q)
        printf("\tUsing the MI355X merge-path SpMV (libmspmv)\n");
    // vector_y_out keeps the correctness call's result (the timed calls write a device buffer)
    const float ms = mspmv_ref::TestOmpMergeCsrmv(a, vector_x, reference_vector_y_out, vector_y_out,
                                                  timing_iterations, setup_ms);
    if (!q) {
        int compare = CompareResults(reference_vector_y_out, vector_y_out, a.num_rows, true);
        printf("\t%s\n", compare ? "FAIL" : "PASS");
        fflush(stdout);
    }
    return ms;
}

// work_2025/spmm/merge_based.hpp:46-153
template <typename ValueT, typename OffsetT>
void OmpMergeCsrmm(int num_threads, CsrMatrix<ValueT, OffsetT> &a, OffsetT *row_end_offsets, OffsetT *column_indices,
                   ValueT *values, ValueT *vector_x, ValueT *vector_y_out, int num_vectors)
{
    mspmv_ref::OmpMergeCsrmm(num_threads, a, row_end_offsets, column_indices, values, vector_x, vector_y_out,
                             num_vectors);
}

// work_2025/main/single_strategy.hpp:102-170, :176-240
template <typename ValueT, typename OffsetT>
int CGSolveSingle(CsrMatrix<ValueT, OffsetT> &a, const ValueT *b, ValueT *x, int max_iters, ValueT tolerance)
{
    return mspmv_ref::CGSolveSingle(a, b, x, max_iters, tolerance);
}
template <typename ValueT, typename OffsetT>
void TestCGSolveSingle(CsrMatrix<ValueT, OffsetT> &a, ValueT *b_vectors, ValueT *x_solutions, int max_iters,
                       ValueT tolerance, int num_vectors, int timing_iterations, double &min_ms,
                       double &iters_of_min_ms)
{
    mspmv_ref::dropin_quiet();
    mspmv_ref::TestCGSolveSingle(a, b_vectors, x_solutions, max_iters, tolerance, num_vectors, timing_iterations,
                                 min_ms, iters_of_min_ms);
}

// work_2025/main/no_pretreatment.hpp:32-197, :202-256
template <typename ValueT, typename OffsetT>
int CGSolveMultiple(CsrMatrix<ValueT, OffsetT> &a, const ValueT *B, ValueT *X, int num_vectors, int max_iters,
                    ValueT tolerance, SpmmKernel kernel_type, std::vector<double> *max_errors = nullptr)
{
    return mspmv_ref::CGSolveMultiple(a, B, X, num_vectors, max_iters, tolerance, kernel_type, max_errors);
}
// (no reference counterpart) multi-RHS BiCGSTAB for nonsymmetric systems
template <typename ValueT, typename OffsetT>
int BiCGStabSolveMultiple(CsrMatrix<ValueT, OffsetT> &a, const ValueT *B, ValueT *X, int num_vectors, int max_iters,
                          ValueT tolerance, std::vector<double> *max_errors = nullptr)
{
    return mspmv_ref::BiCGStabSolveMultiple(a, B, X, num_vectors, max_iters, tolerance, max_errors);
}
template <typename ValueT, typename OffsetT>
int ILU0BiCGStabSolveMultiple(CsrMatrix<ValueT, OffsetT> &a, const ValueT *B, ValueT *X, int num_vectors,
                              int max_iters, ValueT tolerance, std::vector<double> *max_errors = nullptr)
{
    return mspmv_ref::ILU0BiCGStabSolveMultiple(a, B, X, num_vectors, max_iters, tolerance, max_errors);
}
template <typename ValueT, typename OffsetT>
void TestCGMultipleRHS(CsrMatrix<ValueT, OffsetT> &a, ValueT *b_vectors, ValueT *x_solutions, int max_iters,
                       ValueT tolerance, int num_vectors, int timing_iterations, SpmmKernel kernel_type,
                       double &min_ms, double &iters_of_min_ms, std::vector<double> *max_errors = nullptr)
{
    mspmv_ref::dropin_quiet();
    mspmv_ref::TestCGMultipleRHS(a, b_vectors, x_solutions, max_iters, tolerance, num_vectors, timing_iterations,
                                 kernel_type, min_ms, iters_of_min_ms, max_errors);
}

// work_2025/cg/incomplete_cholesky_decomp.hpp:11-78, :84-201
template <typename ValueT, typename OffsetT>
inline void TransposeCsr(const CsrMatrix<ValueT, OffsetT> &in, CsrMatrix<ValueT, OffsetT> &out)
{
    mspmv_ref::TransposeCsr(in, out);
}
template <typename ValueT, typename OffsetT>
bool IncompleteCholesky(const CsrMatrix<ValueT, OffsetT> &a, CsrMatrix<ValueT, OffsetT> &l)
{
    return mspmv_ref::IncompleteCholesky(a, l);
}

// work_2025/main/incomplete_cholesky.hpp:33-199, :205-257
template <typename ValueT, typename OffsetT>
int PCGSolveMultiple(CsrMatrix<ValueT, OffsetT> &a, const CsrMatrix<ValueT, OffsetT> &l,
                     const CsrMatrix<ValueT, OffsetT> &l_transpose, const ValueT *B, ValueT *X, int num_vectors,
                     int max_iters, ValueT tolerance, SpmmKernel kernel_type, std::vector<double> *max_errors = nullptr)
{
    return mspmv_ref::PCGSolveMultiple(a, l, l_transpose, B, X, num_vectors, max_iters, tolerance, kernel_type,
                                       max_errors);
}
template <typename ValueT, typename OffsetT>
void TestPCGMultipleRHS(CsrMatrix<ValueT, OffsetT> &a, const CsrMatrix<ValueT, OffsetT> &l,
                        const CsrMatrix<ValueT, OffsetT> &l_transpose, ValueT *b_vectors, ValueT *x_solutions,
                        int max_iters, ValueT tolerance, int num_vectors, int timing_iterations,
                        SpmmKernel kernel_type, double &min_ms, double &iters_of_min_ms,
                        std::vector<double> *max_errors = nullptr)
{
    mspmv_ref::dropin_quiet();
    mspmv_ref::TestPCGMultipleRHS(a, l, l_transpose, b_vectors, x_solutions, max_iters, tolerance, num_vectors,
                                  timing_iterations, kernel_type, min_ms, iters_of_min_ms, max_errors);
}

// work_2025/cg/sparse_approximate_inversion.hpp:40-321; main/sparse_approximate_inverse.hpp:30-288
template <typename ValueT, typename OffsetT>
bool SparseApproximateInversion(const CsrMatrix<ValueT, OffsetT> &a, CsrMatrix<ValueT, OffsetT> &l)
{
    return mspmv_ref::SparseApproximateInversion(a, l);
}
template <typename ValueT, typename OffsetT>
int SPAISolveMultiple(CsrMatrix<ValueT, OffsetT> &a, CsrMatrix<ValueT, OffsetT> &m, const ValueT *B, ValueT *X,
                      int num_vectors, int max_iters, ValueT tolerance, SpmmKernel kernel_type,
                      std::vector<double> *max_errors = nullptr)
{
    return mspmv_ref::SPAISolveMultiple(a, m, B, X, num_vectors, max_iters, tolerance, kernel_type, max_errors);
}
template <typename ValueT, typename OffsetT>
void TestCGMultipleSPAI(CsrMatrix<ValueT, OffsetT> &a, CsrMatrix<ValueT, OffsetT> &m, ValueT *b_vectors,
                        ValueT *x_solutions, int max_iters, ValueT tolerance, int num_vectors, int timing_iterations,
                        SpmmKernel kernel_type, double &min_ms, double &iters_of_min_ms,
                        std::vector<double> *max_errors = nullptr)
{
    mspmv_ref::dropin_quiet();
    mspmv_ref::TestCGMultipleSPAI(a, m, b_vectors, x_solutions, max_iters, tolerance, num_vectors, timing_iterations,
                                  kernel_type, min_ms, iters_of_min_ms, max_errors);
}
#endif  // MSPMV_REPLACE_REFERENCE

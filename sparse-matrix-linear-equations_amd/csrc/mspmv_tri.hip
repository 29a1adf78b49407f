// mspmv_tri.hip -- triangular factors on the device: the IC(0) and ILU(0) factor objects of include/mspmv.h
// (create, destroy, colours, one solve, the whole apply) and the level-scheduled sync-free solve of a
// natural-order factor (k_trsv_tagged).  The colour sweeps of a multi-colour factor are mspmv_color.hip's.
// The solvers (mspmv_solve.hip, mspmv_cg_passes.hip, mspmv_bicgstab.hip) see a factor through tri_apply,
// tri_workspace, ilu0_workspace and tri_graph_key (mspmv_internal.h) and never ask which kind it is.
#include "mspmv_internal.h"
#include "mspmv_device.h"

#include <algorithm>
#include <cmath>

namespace mspmv {

// ---- natural-order factors: sync-free sparse triangular solves -------------------------------
// x = T^-1 b for a triangular CSR T, one wave per row: ForwardSolveMultiple (FWD, T = L lower, rows
// ascending) and BackwardSolveMultiple (T = L^T upper, rows descending),
// incomplete_cholesky_decomp.hpp:231-348.  Waves are dispatched in dependency-level order and wait
// only on rows of earlier levels, so every awaited row belongs to a wave already resident or
// finished: no deadlock.  Data-tagged values: the output starts filled with a NaN pattern no
// arithmetic produces (kTrsvPending, written by one 32-bit fill), a row's x values are stored by
// single 8-B write-through stores, and a consumer lane polls the very value it needs until the
// pattern is gone -- one memory round trip per dependency hop (ready flags: poll, load, store, drain,
// raise -- measured 9.8 vs 6.35 ms per iteration, round 1).  Bounded: after ~2^20 polls the solve
// reports a stall instead of hanging the GPU.  The partial sums are folded in a tree, not in CSR
// order (the reference's sequential sum): results agree to rounding.
constexpr unsigned kTrsvPendingWord = 0x7ff4deadu;
constexpr unsigned long long kTrsvPending = 0x7ff4dead7ff4deadull;

__device__ __forceinline__ bool wait_value(const double *p, double &out)
{
    for (int it = 0; it < (1 << 20); ++it) {
        const double v = load_sc1(p);
        if ((unsigned long long)__double_as_longlong(v) != kTrsvPending) {
            out = v;
            return true;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    out = 0.0;
    return false;
}

template <int L, bool FWD>
__global__ __launch_bounds__(kBlock) void k_trsv_tagged(const int *__restrict__ ro, const int *__restrict__ ci,
                                                        const double *__restrict__ va, int n,
                                                        const int *__restrict__ order, const double *b, double *x,
                                                        CgControl *ctrl)
{
    constexpr int NZ = 64 / L;
    const int w = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (w >= n || ctrl->done)  // done is set only by earlier launches: uniform here
        return;
    const int i = order[w];  // rows in (level, row) order: awaited rows belong to earlier waves
    const int lane = threadIdx.x & 63;
    const int v = lane % L, q = lane / L;
    const int k1 = ro[i + 1];
    double sum = 0.0, diag = 0.0;
    bool ok = true;
    for (int k0 = ro[i]; k0 < k1; k0 += NZ) {
        const int k = k0 + q;
        if (k < k1) {
            const int j = ci[k];
            const double a = va[k];
            if (j == i) {
                diag = a;
            } else {
                double xj;
                ok = wait_value(&x[(size_t)j * L + v], xj) && ok;
                sum += a * xj;
            }
        }
    }
#pragma unroll
    for (int off = L; off < 64; off <<= 1) {
        sum += __shfl_xor(sum, off);
        diag += __shfl_xor(diag, off);
    }
    if (q == 0) {
        const double bi = b[(size_t)i * L + v];
        const double xi = (!FWD && diag == 0.0) ? 0.0 : (bi - sum) / diag;
        store_sc1(&x[(size_t)i * L + v], xi);
    }
    if (__ballot(!ok) != 0 && lane == 0) {  // a dependency never arrived: MSPMV_ERR_STALL, never hung
        ctrl->breakdown = 2;
        __hip_atomic_store(&ctrl->done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int L>
static void trsv_L(const TriFactor *ic, bool fwd, const double *b, double *x, CgControl *ctrl, hipStream_t s)
{
    const dim3 grid((ic->n + kBlock / 64 - 1) / (kBlock / 64)), block(kBlock);
    if (fwd)
        hipLaunchKernelGGL((k_trsv_tagged<L, true>), grid, block, 0, s, ic->d_lro, ic->d_lci, ic->d_lva, ic->n,
                           ic->d_fwd_order, b, x, ctrl);
    else
        hipLaunchKernelGGL((k_trsv_tagged<L, false>), grid, block, 0, s, ic->d_uro, ic->d_uci, ic->d_uva, ic->n,
                           ic->d_bwd_order, b, x, ctrl);
}

// One pass: the output panel filled with the pending pattern (one 32-bit fill), then the solve.
static hipError_t launch_ic0_trsv(const TriFactor *ic, bool fwd, const double *d_b, double *d_x, int L, CgControl *ctrl,
                           hipStream_t s)
{
    if (ic->n == 0)
        return hipSuccess;
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_x), kTrsvPendingWord, 2 * (size_t)ic->n * L, s);
    if (e != hipSuccess)
        return e;
    return dispatch_L(L, [&](auto Lc) {
        trsv_L<decltype(Lc)::value>(ic, fwd, d_b, d_x, ctrl, s);
        return hipGetLastError();
    });
}

// dst = M^-1 src.  Natural order: ForwardSolveMultiple into t->d_y, then BackwardSolveMultiple
// (incomplete_cholesky.hpp:89-92, :166-167), each into a panel pre-filled with the pending pattern.  A multi-colour
// factor: colour sweeps through t->d_y, no fill (mspmv_color.hip).
hipError_t tri_apply(const TriFactor *t, const double *d_src, double *d_dst, int L, CgControl *ctrl, hipStream_t s)
{
    if (t->num_colors > 0)
        return launch_color_apply(t, d_src, d_dst, L, ctrl, s);
    hipError_t e = launch_ic0_trsv(t, true, d_src, t->d_y, L, ctrl, s);
    if (e == hipSuccess)
        e = launch_ic0_trsv(t, false, t->d_y, d_dst, L, ctrl, s);
    return e;
}

hipError_t tri_solve(const TriFactor *t, int which, const double *d_b, double *d_x, int L, CgControl *ctrl,
                     hipStream_t s)
{
    if (t->num_colors > 0)  // one sweep per colour, in the colour ordering
        return launch_color_trsv(t, which != 0, d_b, d_x, L, ctrl, s);
    return launch_ic0_trsv(t, which == 0, d_b, d_x, L, ctrl, s);
}

mspmv_status tri_workspace(TriFactor *t, size_t elems, const char *what)
{
    HIP_TRY(hipSetDevice(t->device));
    if (elems > t->y_cap) {
        if (t->d_y)
            (void)hipFree(t->d_y);
        t->d_y = nullptr;
        t->y_cap = 0;
        if (hipMalloc(&t->d_y, sizeof(double) * elems) != hipSuccess)
            return (set_error(std::string(what) + " workspace allocation failed"), MSPMV_ERR_OOM);
        t->y_cap = elems;
    }
    return MSPMV_OK;
}

mspmv_status ilu0_workspace(mspmv_ilu0_s *ilu, size_t elems)
{
    ST_TRY(tri_workspace(ilu, elems, "ILU(0)"));
    if (elems > ilu->hat_cap) {
        dev_free(ilu->d_hat);
        ilu->hat_cap = 0;
        ST_TRY(dev_alloc(&ilu->d_hat, elems));
        ilu->hat_cap = elems;
    }
    return MSPMV_OK;
}

// Every array a launch of either kind reads, so a solver's key need not know the kind: a natural-order factor's
// d_perm and a multi-colour one's level orders are null.
void tri_graph_key(const TriFactor *t, std::vector<const void *> &key)
{
    key.insert(key.end(), {t, reinterpret_cast<const void *>((uintptr_t)t->gen), t->d_y, t->d_lro, t->d_lci, t->d_lva,
                           t->d_uro, t->d_uci, t->d_uva, t->d_fwd_order, t->d_bwd_order, t->d_perm,
                           reinterpret_cast<const void *>((intptr_t)t->num_colors)});
}

}  // namespace mspmv

using namespace mspmv;

// ---- the factor objects ------------------------------------------------------------------------
// Two triangular CSRs on the device: a lower one solved forward and an upper one solved backward.  IC(0) passes L
// and its transpose, ILU(0) passes L and U.  A natural-order factor (levels) stores L's diagonal in every row and
// gets its level orders for the sync-free solves (launch_ic0_trsv); a multi-colour one gets neither.
// Level sets: a row's level is 1 + the deepest level among the rows it reads (L: columns
// below the diagonal, solved ascending; L^T: columns above it, solved descending).  Waves
// take rows in (level, row) order, so every awaited row is in an earlier level, hence an
// earlier-dispatched wave, and a whole level's rows are solved concurrently (natural order
// would chain every row to its left neighbour: ~15x slower on a 2-D stencil).
static mspmv_status upload_triangles(const HostFactor &f, int device, bool levels, TriFactor *m, const char *what)
{
    const int n = (int)f.lro.size() - 1;
    auto order_by_level = [&](const std::vector<int> &rp, const std::vector<int> &cp, bool fwd) {
        std::vector<int> lev((size_t)n, 0);
        int maxlev = 0;
        for (int s = 0; s < n; ++s) {
            const int i = fwd ? s : n - 1 - s;
            int lv = 0;
            for (int k = rp[i]; k < rp[i + 1]; ++k) {
                const int j = cp[k];
                if (fwd ? j < i : j > i)
                    lv = std::max(lv, lev[j] + 1);
            }
            lev[i] = lv;
            maxlev = std::max(maxlev, lv);
        }
        std::vector<int> cnt((size_t)maxlev + 2, 0);
        for (int i = 0; i < n; ++i)
            ++cnt[(size_t)lev[i] + 1];
        for (int l2 = 0; l2 <= maxlev; ++l2)
            cnt[(size_t)l2 + 1] += cnt[l2];
        std::vector<int> order((size_t)std::max(n, 1), 0);
        for (int s = 0; s < n; ++s) {
            const int i = fwd ? s : n - 1 - s;
            order[(size_t)cnt[lev[i]]++] = i;
        }
        return order;
    };
    HIP_TRY(hipSetDevice(device));
    m->device = device;
    m->n = n;
    mspmv_status st = MSPMV_OK;
    auto up = [&](auto **d, const auto &src, size_t cnt) {
        if (st != MSPMV_OK)
            return;
        st = dev_alloc(d, std::max<size_t>(cnt, 1));
        if (st == MSPMV_OK && cnt && hipMemcpy(*d, src.data(), sizeof(**d) * cnt, hipMemcpyHostToDevice) != hipSuccess) {
            set_error(std::string(what) + " upload failed");
            st = MSPMV_ERR_HIP;
        }
    };
    const size_t lnnz = (size_t)f.lro[n], unnz = (size_t)f.uro[n];
    up(&m->d_lro, f.lro, (size_t)n + 1);
    up(&m->d_lci, f.lci, lnnz);
    up(&m->d_lva, f.lva, lnnz);
    up(&m->d_uro, f.uro, (size_t)n + 1);
    up(&m->d_uci, f.uci, unnz);
    up(&m->d_uva, f.uva, unnz);
    if (levels) {
        up(&m->d_fwd_order, order_by_level(f.lro, f.lci, true), (size_t)n);
        up(&m->d_bwd_order, order_by_level(f.uro, f.uci, false), (size_t)n);
    }
    return st;
}

// The colours of a multi-colour factor whose triangles upload_triangles has placed in t: perm on the device, and per
// colour the longest row of each triangle in off-diagonal entries (L's rows hold their diagonal when l_diag, U's
// always), which picks a sweep's LONG instantiation.  Takes f's perm and color_off.
static mspmv_status upload_colors(TriFactor *t, HostFactor &f, bool l_diag, const char *what)
{
    const int n = t->n, C = (int)f.color_off.size() - 1;
    ST_TRY(dev_alloc(&t->d_perm, (size_t)n));
    if (n && hipMemcpy(t->d_perm, f.perm.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) {
        set_error(std::string(what) + " upload failed");
        return MSPMV_ERR_HIP;
    }
    t->num_colors = C;
    t->l_diag = l_diag;
    t->lmax.assign((size_t)C, 0), t->umax.assign((size_t)C, 0);
    for (int c = 0; c < C; ++c)
        for (int i = f.color_off[c]; i < f.color_off[(size_t)c + 1]; ++i) {
            t->lmax[c] = std::max(t->lmax[c], f.lro[(size_t)i + 1] - f.lro[i] - (l_diag ? 1 : 0));
            t->umax[c] = std::max(t->umax[c], f.uro[(size_t)i + 1] - f.uro[i] - 1);
        }
    t->color_off.swap(f.color_off);
    t->perm.swap(f.perm);
    return MSPMV_OK;
}

// The device arrays of a factor's two triangles and its intermediate.
static void tri_release(TriFactor *m)
{
    (void)hipSetDevice(m->device);
    dev_free(m->d_lro);
    dev_free(m->d_lci);
    dev_free(m->d_lva);
    dev_free(m->d_uro);
    dev_free(m->d_uci);
    dev_free(m->d_uva);
    dev_free(m->d_fwd_order);
    dev_free(m->d_bwd_order);
    dev_free(m->d_perm);
    if (m->d_y)
        (void)hipFree(m->d_y);
}

static void destroy(mspmv_ic0 m) { (void)mspmv_ic0_destroy(m); }
static void destroy(mspmv_ilu0 m) { (void)mspmv_ilu0_destroy(m); }

// f on the device as a new factor of type F (mspmv_ic0_s / mspmv_ilu0_s); colored: with f's ordering.
template <typename F>
static mspmv_status create_factor(HostFactor &f, int device, bool colored, bool l_diag, const char *what, F **out)
{
    F *m = new F;
    mspmv_status st = upload_triangles(f, device, !colored, m, what);
    if (st == MSPMV_OK && colored)
        st = upload_colors(m, f, l_diag, what);
    if (st != MSPMV_OK) {
        destroy(m);
        return st;
    }
    *out = m;
    return MSPMV_OK;
}

// mspmv_ic0_create_colored / mspmv_ilu0_create_colored: host(f) runs the checks, the ordering and the
// factorisation, all on the host, before the device is touched.
template <typename F, typename Host>
static mspmv_status create_colored(int device, bool l_diag, const char *what, F **out, Host &&host)
{
    if (!out)
        return invalid("null output");
    *out = nullptr;
    HostFactor f;
    ST_TRY(host(f));
    return create_factor(f, device, true, l_diag, what, out);
}

static mspmv_status tri_colors(const TriFactor *t, int *num_colors, int *perm, const char *who)
{
    if (!t || !num_colors)
        return invalid(std::string(who) + ": null factor or output");
    *num_colors = t->num_colors;
    if (perm && t->num_colors > 0)
        std::copy(t->perm.begin(), t->perm.end(), perm);
    return MSPMV_OK;
}

// A factor applied alone, on a's stream with a's control word, synchronised: one triangular solve (which: 0 / 1,
// which_msg its error text), or with which_msg null the preconditioner apply, both triangles through the factor's
// intermediate.  what: "IC(0)" / "ILU(0)".
static mspmv_status tri_run_dev(mspmv_handle a, TriFactor *m, int which, const char *which_msg, const double *d_B,
                                double *d_X, int L, const char *what)
{
    const bool apply = !which_msg;
    const std::string panels = apply ? "preconditioner-apply panels" : "triangular-solve panels";
    ST_TRY(check_handle(a));
    if (!m)
        return invalid(std::string("null ") + what + " factor");
    if (!apply && which != 0 && which != 1)
        return invalid(which_msg);
    if (a->m != a->n || m->n != a->m || m->device != a->device)
        return invalid(std::string("the ") + what + " factor must match the matrix's shape and device");
    if (!supported_L(L))
        return (set_error("L must be one of 1, 2, 4, 8, 16"), MSPMV_ERR_UNSUPPORTED);
    if (m->n == 0)
        return MSPMV_OK;
    if (!d_B || !d_X)
        return invalid("null panel");
    if (!aligned16(d_B) || !aligned16(d_X))
        return invalid(panels + " must be 16-byte aligned");
    const uintptr_t b0 = (uintptr_t)d_B, x0 = (uintptr_t)d_X, bytes = sizeof(double) * (size_t)m->n * L;
    if (b0 < x0 + bytes && x0 < b0 + bytes)
        return invalid(panels + " must not overlap" + (apply ? "" : " (X is pre-filled with the pending pattern)"));
    if (apply) {
        ST_TRY(tri_workspace(m, (size_t)m->n * L, what));  // the intermediate d_y
        HIP_TRY(hipSetDevice(a->device));
    }
    if (!a->d_ctrl)
        ST_TRY(dev_alloc(&a->d_ctrl, 1));
    HIP_TRY(hipMemsetAsync(a->d_ctrl, 0, sizeof(CgControl), a->stream));
    HIP_TRY(apply ? tri_apply(m, d_B, d_X, L, a->d_ctrl, a->stream)
                  : tri_solve(m, which, d_B, d_X, L, a->d_ctrl, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    CgControl fin{};
    HIP_TRY(hipMemcpy(&fin, a->d_ctrl, sizeof(CgControl), hipMemcpyDeviceToHost));
    if (fin.breakdown == 2) {
        set_error(std::string(what) + (apply ? " apply" : " solve") +
                  ": a triangular-solve dependency never became ready (solve stalled)");
        return MSPMV_ERR_STALL;
    }
    return MSPMV_OK;
}

extern "C" {

// ---- IC(0) ---------------------------------------------------------------------------------------
mspmv_status mspmv_ic0_create(const mspmv_csr_d *l, int device, mspmv_ic0 *out)
{
    if (!out)
        return invalid("null output");
    *out = nullptr;
    ST_TRY(validate_host_csr(l));
    ST_TRY(check_csr(l, "ic0_create"));
    if (l->num_rows != l->num_cols)
        return invalid("IC(0) factor must be square");
    const int n = l->num_rows, nnz = l->num_nonzeros;
    // A lower-triangular factor with every diagonal present (IncompleteCholesky keeps A's lower
    // pattern, diagonal included): an entry above the diagonal would make the forward solve wait
    // on a row of a later level, a missing diagonal would divide by zero -- reject both here
    // rather than stall on the GPU.
    for (int r = 0; r < n; ++r) {
        bool diag = false;
        for (int k = l->row_offsets[r]; k < l->row_offsets[r + 1]; ++k) {
            if (l->column_indices[k] > r)
                return invalid("IC(0) factor has an entry above the diagonal in row " + std::to_string(r));
            diag = diag || l->column_indices[k] == r;
        }
        if (!diag)
            return invalid("IC(0) factor row " + std::to_string(r) + " has no diagonal entry");
    }
    HostFactor f;
    f.lro.assign(l->row_offsets, l->row_offsets + n + 1);
    f.lci.assign(l->column_indices, l->column_indices + nnz);
    f.lva.assign(l->values, l->values + nnz);
    // L^T by TransposeCsr (incomplete_cholesky_decomp.hpp:11-78): counting sort by column, rows in order
    f.uro.assign((size_t)n + 1, 0), f.uci.assign((size_t)std::max(nnz, 1), 0), f.uva.assign((size_t)std::max(nnz, 1), 0.0);
    ST_TRY(mspmv_csr_transpose(l, f.uro.data(), f.uci.data(), f.uva.data()));
    return create_factor(f, device, false, true, "IC(0)", out);
}

mspmv_status mspmv_ic0_create_colored(const mspmv_csr_d *a, const int *colors, int device, double *shift,
                                      mspmv_ic0 *out)
{
    return create_colored(device, true, "IC(0)", out,
                          [&](HostFactor &f) { return ic0_colored_host(a, colors, f, shift); });
}

mspmv_status mspmv_ic0_destroy(mspmv_ic0 m)
{
    if (!m)
        return MSPMV_OK;
    tri_release(m);
    delete m;
    return MSPMV_OK;
}

mspmv_status mspmv_ic0_colors(mspmv_ic0 m, int *num_colors, int *perm)
{
    return tri_colors(m, num_colors, perm, "ic0_colors");
}

mspmv_status mspmv_ic0_solve_dev(mspmv_handle a, mspmv_ic0 m, int transpose, const double *d_B, double *d_X, int L)
{
    return tri_run_dev(a, m, transpose, "transpose must be 0 (L X = B) or 1 (L^T X = B)", d_B, d_X, L, "IC(0)");
}

mspmv_status mspmv_ic0_apply_dev(mspmv_handle a, mspmv_ic0 m, const double *d_B, double *d_X, int L)
{
    return tri_run_dev(a, m, 0, nullptr, d_B, d_X, L, "IC(0)");
}

// ---- ILU(0) --------------------------------------------------------------------------------------
mspmv_status mspmv_ilu0_create(const mspmv_csr_d *lu, int device, mspmv_ilu0 *out)
{
    if (!out)
        return invalid("null output");
    *out = nullptr;
    ST_TRY(ilu0_check_rows(lu, "ilu0_create"));
    const int n = lu->num_rows;
    const int *ro = lu->row_offsets, *ci = lu->column_indices;
    // A solve divides by U's diagonal: zero or non-finite is refused here.
    for (int i = 0; i < n; ++i)
        for (int k = ro[i]; k < ro[i + 1]; ++k)
            if (ci[k] == i && (lu->values[k] == 0.0 || !std::isfinite(lu->values[k])))
                return invalid("ILU(0) factor row " + std::to_string(i) + " has a zero or non-finite diagonal");
    // L: the strictly lower entries, then a stored 1.0 diagonal (k_trsv_tagged finds a diagonal by j == i and
    // divides by it: by 1.0, exactly); U: the diagonal first, then the upper entries.
    HostFactor f;
    split_lu(n, ro, ci, lu->values, true, f);
    return create_factor(f, device, false, false, "ILU(0)", out);
}

mspmv_status mspmv_ilu0_create_colored(const mspmv_csr_d *a, const int *colors, int device, mspmv_ilu0 *out)
{
    return create_colored(device, false, "ILU(0)", out, [&](HostFactor &f) { return ilu0_colored_host(a, colors, f); });
}

mspmv_status mspmv_ilu0_destroy(mspmv_ilu0 m)
{
    if (!m)
        return MSPMV_OK;
    tri_release(m);
    dev_free(m->d_hat);
    delete m;
    return MSPMV_OK;
}

mspmv_status mspmv_ilu0_colors(mspmv_ilu0 m, int *num_colors, int *perm)
{
    return tri_colors(m, num_colors, perm, "ilu0_colors");
}

mspmv_status mspmv_ilu0_solve_dev(mspmv_handle a, mspmv_ilu0 m, int upper, const double *d_B, double *d_X, int L)
{
    return tri_run_dev(a, m, upper, "upper must be 0 (L X = B) or 1 (U X = B)", d_B, d_X, L, "ILU(0)");
}

mspmv_status mspmv_ilu0_apply_dev(mspmv_handle a, mspmv_ilu0 m, const double *d_B, double *d_X, int L)
{
    return tri_run_dev(a, m, 0, nullptr, d_B, d_X, L, "ILU(0)");
}

}  // extern "C"

// mspmv_solve.hip -- the solver drivers behind the C-ABI's CG, BiCGSTAB and block CG entry points: the handle's
// workspace, the protocol every batched solve follows (prologue, cached iteration graph, pipelined batches,
// collection), the native-width solvers, column groups for any other width, and the host-pointer forms.  The
// iterations' kernels are in mspmv_cg_passes.hip, mspmv_cg_resident.hip, mspmv_bicgstab.hip and mspmv_blockcg.hip,
// the factors in mspmv_tri.hip.
#include "mspmv_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <vector>

using namespace mspmv;

// ---- the workspace -------------------------------------------------------------------------
// fold_width: columns of a partial row when wider than L (BiCGSTAB's two-dot folds: 2 L; the block CG's Gram
// folds: L^2)
// The folds' share of it: partial rows of `width` columns for `slots` slots, their tickets (zeroed when allocated),
// the control word and the warm pass's sums -- all a fold outside a solve needs (mspmv_dresidual_dev).
static mspmv_status ensure_fold_workspace(mspmv_handle_s *h, size_t slots, int width)
{
    const size_t pcap = partials_capacity(slots, width);
    if (pcap > h->partials_cap) {
        dev_free(h->d_partials);
        h->partials_cap = 0;
        ST_TRY(dev_alloc(&h->d_partials, pcap));
        h->partials_cap = pcap;
    }
    if (gtickets_capacity(slots) > h->gtickets_cap) {
        dev_free(h->d_gtickets);
        h->gtickets_cap = 0;
        ST_TRY(dev_alloc(&h->d_gtickets, gtickets_capacity(slots)));
        // on the handle's stream: it is non-blocking, so a null-stream memset is not ordered before the
        // folds queued on it next
        HIP_TRY(hipMemsetAsync(h->d_gtickets, 0, sizeof(unsigned) * gtickets_capacity(slots), h->stream));
        h->gtickets_cap = gtickets_capacity(slots);
    }
    if (!h->d_ctrl)
        ST_TRY(dev_alloc(&h->d_ctrl, 1));
    if (!h->d_warm)
        ST_TRY(dev_alloc(&h->d_warm, (size_t)2 * 16));
    return MSPMV_OK;
}

static mspmv_status ensure_cg_workspace(mspmv_handle_s *h, int L, int nblk, int num_tiles, int hist_cap,
                                        int fold_width = 0)
{
    // L = 1: the pipelined CG's p buffers hold {r, p} interleaved (2 m doubles each)
    const size_t elems = (size_t)h->m * std::max(L, 2);
    if (elems > h->cg_cap_elems) {
        dev_free(h->d_r);
        dev_free(h->d_p0);
        dev_free(h->d_p1);
        dev_free(h->d_ap);
        h->cg_cap_elems = 0;
        ST_TRY(dev_alloc(&h->d_r, elems));
        ST_TRY(dev_alloc(&h->d_p0, elems));
        ST_TRY(dev_alloc(&h->d_p1, elems));
        ST_TRY(dev_alloc(&h->d_ap, elems));
        h->cg_cap_elems = elems;
    }
    ST_TRY(ensure_fold_workspace(h, (size_t)std::max(nblk, num_tiles), std::max(L, fold_width)));
    if (!h->d_partials_b)
        ST_TRY(dev_alloc(&h->d_partials_b, (size_t)kUpdateMaxBlocks));
    if (L > h->scal_cap) {
        dev_free(h->d_scal);
        dev_free(h->d_conv);
        h->scal_cap = 0;
        dev_free(h->d_red);
        ST_TRY(dev_alloc(&h->d_scal, (size_t)L));
        ST_TRY(dev_alloc(&h->d_conv, (size_t)L));
        ST_TRY(dev_alloc(&h->d_red, (size_t)L));
        h->scal_cap = L;
    }
    if (!h->h_ctrl)
        HIP_TRY(hipHostMalloc((void **)&h->h_ctrl, sizeof(CgControl) * 2, hipHostMallocDefault));
    if (hist_cap > h->hist_cap) {
        dev_free(h->d_hist);
        h->hist_cap = 0;
        ST_TRY(dev_alloc(&h->d_hist, (size_t)hist_cap));
        h->hist_cap = hist_cap;
    }
    return MSPMV_OK;
}

// Register-resident single-RHS CG: one launch runs the whole solve.  d_stamps: the diagnostic
// phase stamps (mspmv_cg_resident_stamps), null in ordinary solves.
static mspmv_status cg_solve_resident(mspmv_handle_s *h, ResidentCg *rc, const double *d_b, double *d_x,
                                      int max_iters, double tol, int *iters, double *hist, int use_cap,
                                      unsigned long long *d_stamps = nullptr, int stamp_iters = 0)
{
    const int saved_cap = h->hist_cap;
    h->hist_cap = use_cap;
    hipError_t e = hipMemsetAsync(h->d_ctrl, 0, sizeof(CgControl), h->stream);
    if (e == hipSuccess)
        e = launch_cg_resident(h, rc, d_b, d_x, max_iters, tol, d_stamps, stamp_iters);
    h->hist_cap = saved_cap;
    if (e != hipSuccess) {
        set_error(std::string("resident CG launch: ") + hipGetErrorString(e));
        return MSPMV_ERR_HIP;
    }
    h->last_cg_kernel = rc->name;
    CgControl fin{};
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(&fin, h->d_ctrl, sizeof(CgControl), hipMemcpyDeviceToHost));
    const int it = fin.iters_out;
    if (iters)
        *iters = it;
    if (hist && use_cap > 0) {
        const int nh = std::min(it, use_cap);
        if (nh > 0)
            HIP_TRY(hipMemcpy(hist, h->d_hist, sizeof(double) * nh, hipMemcpyDeviceToHost));
    }
    if (fin.breakdown == 2) {
        set_error("resident CG: a reduction hand-off never completed (solve stalled; workgroups not co-resident?)");
        return MSPMV_ERR_STALL;
    }
    if (fin.breakdown) {
        set_error("CG breakdown: p.Ap gave a non-finite alpha at iteration " + std::to_string(it));
        return MSPMV_ERR_BREAKDOWN;
    }
    return MSPMV_OK;
}

// The resident layout of h when the next single-RHS solve may use it: built for this handle's
// current CU count (all of the device's CUs), matrix fits.  nullptr otherwise.
static mspmv_status resident_for(mspmv_handle_s *h, ResidentCg **out)
{
    *out = nullptr;
    if (!cg_resident_enabled())
        return MSPMV_OK;
    ResidentCg *rc = nullptr;
    ST_TRY(resident_prepare(h, &rc));
    if (rc->ok && rc->G == h->num_cus)
        *out = rc;
    return MSPMV_OK;
}

// ---- the protocol every batched solve on a handle follows (cg_solve_native, bicgstab_solve_native) ----
// Prologue, on the handle's stream, before the solver's init: a zeroed control word, zeroed fold tickets and
// split-row tickets of the plans the solve multiplies with, and the pending mspmv_test_poison_tickets flags
// (returned in *poison_out; consumed).
static mspmv_status solve_prologue(mspmv_handle_s *h, std::initializer_list<const TilePlan *> plans, int *poison_out)
{
    HIP_TRY(hipMemsetAsync(h->d_ctrl, 0, sizeof(CgControl), h->stream));
    // test hook (mspmv_test_poison_tickets): dirty fold tickets at the first fold, as an unordered zeroing
    // of freshly allocated (recycled) memory leaves them
    const int poison = h->poison_flags;
    h->poison_flags = 0;
    *poison_out = poison;
    // the fold tickets reset themselves, but a solve that stopped early or faulted may leave some
    // raised: every solve starts from zeroed ones (a few KB, on the solve's stream)
    HIP_TRY(hipMemsetAsync(h->d_gtickets, 0, sizeof(unsigned) * h->gtickets_cap, h->stream));
    if (poison & MSPMV_POISON_NO_STOP)
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)&h->d_ctrl->fault_no_stop, 1, 1, h->stream));
    // Split-row tickets reset themselves when every tile sharing a row reaches close_split_rows; a CG
    // SpMM returns at its stop test before that (all tiles alike, but an aborted launch might not), so
    // every solve starts from zeroed tickets
    for (const TilePlan *tp : plans)
        if (tp && tp->d_fix_cnt)
            HIP_TRY(hipMemsetAsync(tp->d_fix_cnt, 0, sizeof(unsigned) * (size_t)tp->num_tiles, h->stream));
    return MSPMV_OK;
}

// test hook, after the solver's init: the iterations' folds meet dirty tickets
static mspmv_status solve_poison_fill(mspmv_handle_s *h, int poison)
{
    if (poison & MSPMV_POISON_FILL)
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)h->d_gtickets, (int)h->poison_value, h->gtickets_cap, h->stream));
    return MSPMV_OK;
}

// Warm start (mspmv_set_initial_guess, MSPMV_X0_CALLER), between the prologue and the solver's warm init: W = A X0
// into h->d_ap on the path the solve's own products take, then R0 = B - W into h->d_r with B.B and R0.R0 per column
// into h->d_warm (k_warm_residual, mspmv_warm.hip).  The workspace's partial rows are at least 2 L wide.
static bool warm_start(const mspmv_handle_s *h) { return h->x0_mode == MSPMV_X0_CALLER; }
static hipError_t launch_warm_start(mspmv_handle_s *h, const TilePlan &plan, const TilePlan *splan, const double *d_b,
                                    const double *d_x, int L, int nblk)
{
    const hipError_t e = launch_solver_product(h, plan, splan, d_x, h->d_ap, L);
    return e != hipSuccess ? e : launch_warm_residual(h, d_b, h->d_ap, h->d_r, L, nblk);
}

// Fills one of the handle's cached iteration graphs (GraphCache) for `key`: kept when it was captured with the
// same key, else captured anew.
using IterateFn = std::function<hipError_t(int)>;  // enqueue iteration i of a batch on the handle's stream
static mspmv_status solver_graph(mspmv_handle_s *h, GraphCache &g, const std::vector<const void *> &key, int K,
                                 const IterateFn &iterate, const char *name)
{
    if (g.exec && g.key == key)
        return MSPMV_OK;
    g.reset();
    hipError_t e = hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal);
    for (int i = 0; i < K && e == hipSuccess; ++i)
        e = iterate(i);
    hipGraph_t graph = nullptr;
    hipError_t e2 = hipStreamEndCapture(h->stream, &graph);
    if (e == hipSuccess)
        e = e2;
    g.graph = graph;
    if (e == hipSuccess)
        e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        set_error(std::string(name) + " graph capture: " + hipGetErrorString(e));
        return MSPMV_ERR_HIP;
    }
    g.key = key;
    return MSPMV_OK;
}

// The iterations, in batches of K (a replay of exec when given and the batch is whole, else launched one by
// one), the control word copied back after each.  Pipelined: batch b+1 is queued before batch b's control
// word is inspected, so the GPU never idles on the host check; after convergence at most one batch of
// kernels runs, each returning at its first instruction (the `done` test).
static mspmv_status solve_batches(mspmv_handle_s *h, int K, int max_iters, hipGraphExec_t exec, int poison,
                                  hipEvent_t (&evs)[2], const char *name, const IterateFn &iterate)
{
    if (hipEventCreateWithFlags(&evs[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&evs[1], hipEventDisableTiming) != hipSuccess) {
        set_error("hipEventCreate failed");
        return MSPMV_ERR_HIP;
    }
    int iterations_enqueued = 0;
    auto iterate_hook = [&](int i) -> hipError_t {
        hipError_t e = iterate(i);
        if (e == hipSuccess && (poison & MSPMV_POISON_LATE_ZERO) && ++iterations_enqueued == 1)
            e = hipMemsetAsync(h->d_gtickets, 0, sizeof(unsigned) * h->gtickets_cap, h->stream);  // the late zeroing
        return e;
    };
    int launched = 0, pending = 0, oldest = 0, slot = 0;
    for (;;) {
        const int k = std::min(K, max_iters - launched);
        if (k > 0) {
            hipError_t e = hipSuccess;
            if (k == K && exec)
                e = hipGraphLaunch(exec, h->stream);
            else
                for (int i = 0; i < k && e == hipSuccess; ++i)
                    e = iterate_hook(i);
            if (e == hipSuccess)
                e = hipMemcpyAsync(&h->h_ctrl[slot], h->d_ctrl, sizeof(CgControl), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess)
                e = hipEventRecord(evs[slot], h->stream);
            if (e != hipSuccess) {
                set_error(std::string(name) + " launch: " + hipGetErrorString(e));
                return MSPMV_ERR_HIP;
            }
            launched += k;
            ++pending;
            slot ^= 1;
        }
        if (pending == 0)
            break;
        if (pending == 2 || k <= 0) {
            if (hipEventSynchronize(evs[oldest]) != hipSuccess) {
                set_error(std::string(name) + " event sync failed");
                return MSPMV_ERR_HIP;
            }
            --pending;
            const bool done = h->h_ctrl[oldest].done != 0;
            oldest ^= 1;
            if (done)
                break;
        }
    }
    return MSPMV_OK;
}

// After the last launch: wait, read the control word into *fin, hand out the iteration count and the history,
// and report a ticket fault.  st: the solve's status so far (an error is passed through after the wait).
static mspmv_status solve_collect(mspmv_handle_s *h, mspmv_status st, hipEvent_t (&evs)[2], int saved_cap, int use_cap,
                                  int *iters, double *hist, CgControl *fin, const char *name)
{
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess)
        e = hipMemcpy(fin, h->d_ctrl, sizeof(CgControl), hipMemcpyDeviceToHost);
    if (st == MSPMV_OK && e != hipSuccess) {
        set_error(std::string(name) + " finish: " + hipGetErrorString(e));
        st = MSPMV_ERR_HIP;
    }
    for (auto &ev : evs)
        if (ev)
            (void)hipEventDestroy(ev);
    h->hist_cap = saved_cap;
    if (st != MSPMV_OK)
        return st;
    const int it = fin->done ? fin->iters_out : fin->iter;
    if (iters)
        *iters = it;
    if (hist && use_cap > 0) {
        const int nh = std::min(it, use_cap);
        if (nh > 0)
            HIP_TRY(hipMemcpy(hist, h->d_hist, sizeof(double) * nh, hipMemcpyDeviceToHost));
    }
    if (fin->fault) {
        set_error(std::string(name) + ": a reduction ticket drew past its group (the ticket array was not zero when a "
                  "fold began): the solve stopped, X is not a solution");
        return MSPMV_ERR_FAULT;
    }
    return MSPMV_OK;
}

// CG; SPAI-preconditioned CG with the preconditioner's handle hm; or IC(0)-preconditioned CG
// with the factor ic.
static mspmv_status cg_solve_native(mspmv_handle_s *h, const double *d_b, double *d_x, int L, int max_iters,
                                    double tol, int *iters, double *hist, int hist_cap, mspmv_handle_s *hm,
                                    mspmv_ic0_s *ic)
{
    if (h->m != h->n)
        return invalid("CG needs a square matrix");
    if (hm && (hm->m != h->m || hm->n != h->n || hm->device != h->device))
        return invalid("the preconditioner must match the matrix's shape and device");
    if (ic && (ic->n != h->m || ic->device != h->device))
        return invalid("the IC(0) factor must match the matrix's shape and device");
    if (ic)  // the apply's intermediate lives with the factor: grown here, before any capture
        ST_TRY(tri_workspace(ic, (size_t)h->m * L, "IC(0)"));
    if (!supported_L(L))
        return (set_error("L must be one of 1, 2, 4, 8, 16"), MSPMV_ERR_UNSUPPORTED);
    if (max_iters < 0)
        return invalid("max_iters < 0");
    if (h->m > 0 && (!d_b || !d_x))
        return invalid("null vector");
    if (!aligned16(d_b) || !aligned16(d_x))
        return invalid("CG vectors must be 16-byte aligned");
    if (iters)
        *iters = 0;
    if (h->m == 0)
        return MSPMV_OK;
    // A warm single-RHS solve runs the split iteration: the resident and pipelined kernels derive ||b|| from r.r
    // inside their first iteration.  (cg_split_iteration's process-wide switch is the cold solves' alone.)
    const bool warm = warm_start(h);
    const bool split = cg_split_iteration(L) || warm;
    const TilePlan *plan = nullptr, *mplan = nullptr, *splan = nullptr;
    if (!hm && !ic) {
        // the split iteration's plain SpMM runs on the handle's offset-window or column-slab plan when
        // the plain product takes one, the pipelined single-RHS iteration's SpMV on its offset windows
        // (k_cg1_dia): decided here, before any graph capture (it may copy the matrix to the host)
        ST_TRY(product_plan(h, L, &splan));
        if (!(splan->dia || (splan->slab && split)))
            splan = nullptr;
    }
    if (splan && splan->dia && !split)
        plan = splan;  // the pipelined form on the windows needs no merge tiles
    else
        ST_TRY(solver_plan(h, L, &plan));
    const bool dot_fused = dia_dot_fused();  // once per solve (an environment switch; in the graph key)
    if (hm) {
        ST_TRY(solver_plan(hm, L, &mplan));
        HIP_TRY(hipStreamSynchronize(hm->stream));  // hm's SpMMs are enqueued on h's stream
    }
    const bool pipelined = !hm && !ic && !split;  // single RHS: consumer-side reductions
    bool stalled = false;
    const int nblk = pipelined ? cg1_blocks(h->m) : cg_update_blocks((long long)h->m * L, h->num_cus);
    const int cap = hist ? std::max(hist_cap, 0) : 0;
    // partials: one per tile of the plan, or per window of the offset-window plan (its dot mode)
    ST_TRY(ensure_cg_workspace(h, L, nblk,
                               std::max({plan->num_tiles, mplan ? mplan->num_tiles : 0, splan ? splan->num_tiles : 0}),
                               cap, 2 * L));  // (2 L: the warm start's pass -- cold solves too, so that a warm solve
                                              // after a cold one keeps d_partials, which is in the graph's key)
    const int use_cap = hist ? cap : 0;
    if (pipelined) {
        // the whole solve as one register-resident launch, where the matrix fits (mspmv_cg_resident.hip)
        ResidentCg *rc = nullptr;
        ST_TRY(resident_for(h, &rc));
        if (rc) {
            const mspmv_status rs = cg_solve_resident(h, rc, d_b, d_x, max_iters, tol, iters, hist, use_cap);
            if (rs != MSPMV_ERR_STALL)
                return rs;
            // A hand-off never completed: the one-workgroup-per-CU grid was not co-resident (work on
            // another stream or process held CUs).  The solve is run again on the pipelined kernels,
            // whose init resets x, r and p; nothing of the stalled launch is kept.
            set_error("");
            stalled = true;
        }
    }
    const bool on_windows = pipelined && splan && splan->dia;
    h->last_cg_kernel = pipelined ? std::string(on_windows ? "pipelined (k_cg1_dia + k_cg1_update)"
                                                           : "pipelined (k_spmv_tile MODE 1 + k_cg1_update)") +
                                        (stalled ? " after a resident-CG stall" : "")
                        : hm      ? "SPAI-PCG (split)"
                        : ic      ? "IC0-PCG (split)"
                                  : "split (p update, SpMM, p.Ap, update)";
    if (ic && ic->num_colors > 0)  // an apply is 2 C - 1 colour sweeps (mspmv_color.hip)
        h->last_cg_kernel = "MC-IC0-PCG (split, " + std::to_string(2 * ic->num_colors - 1) + " sweeps of " +
                            std::to_string(ic->num_colors) + " colours)";
    if (stream_nt(h))  // the iteration's product kernels in their nontemporal instantiation (no cache lease)
        h->last_cg_kernel += ", nontemporal matrix loads";
    const int saved_cap = h->hist_cap;
    h->hist_cap = use_cap;  // kernels record only what the caller asked for
    int poison = 0;
    ST_TRY(solve_prologue(h, {plan, splan, mplan}, &poison));
    if (warm)
        HIP_TRY(launch_warm_start(h, *plan, splan, d_b, d_x, L, nblk));
    if (hm)
        HIP_TRY(launch_pcg_init(h, hm, *mplan, d_b, d_x, L, tol, nblk, warm));
    else if (ic)
        HIP_TRY(launch_pcg_ic0_init(h, ic, d_b, d_x, L, tol, nblk, warm));
    else if (pipelined)
        HIP_TRY(launch_cg1_init(h, d_b, d_x, nblk));
    else
        HIP_TRY(launch_cg_init(h, d_b, d_x, L, tol, nblk, warm));
    ST_TRY(solve_poison_fill(h, poison));  // (after the init's fold)
    auto iterate = [&](int i) -> hipError_t {
        if (hm)
            return launch_pcg_iteration(h, hm, *plan, *mplan, d_x, L, nblk, tol);
        if (ic)
            return launch_pcg_ic0_iteration(h, ic, *plan, d_x, L, nblk, tol);
        return launch_cg_iteration(h, *plan, splan, dot_fused, d_x, L, i & 1, nblk, tol, split);
    };

    const int K = cg_batch_iters(h->m, h->nnz, L);  // iterations per graph replay (even: p buffers alternate)
    mspmv_status st = MSPMV_OK;
    hipGraphExec_t exec = nullptr;
    if (max_iters >= K && !(poison & MSPMV_POISON_LATE_ZERO)) {
        // The graph bakes in every buffer, the plan, L, the tolerance and the history size:
        // reuse the handle's graph while all of them are unchanged (instantiation costs ms).
        const void *tk = nullptr;
        static_assert(sizeof(tk) == sizeof(tol), "tolerance bits as a key word");
        std::memcpy(&tk, &tol, sizeof tk);
        std::vector<const void *> key = {
            d_x, h->d_r, h->d_p0, h->d_p1, h->d_ap, h->d_partials, h->d_partials_b, h->d_gtickets, h->d_scal,
            h->d_conv, h->d_red, h->d_ctrl, h->d_hist, h->stream, plan, splan, tk,
            reinterpret_cast<const void *>((intptr_t)L), reinterpret_cast<const void *>((intptr_t)nblk),
            reinterpret_cast<const void *>((intptr_t)use_cap), hm, mplan,
            hm ? (const void *)hm->d_vals : nullptr,
            reinterpret_cast<const void *>((uintptr_t)(hm ? hm->gen : 0)),
            reinterpret_cast<const void *>((intptr_t)K), reinterpret_cast<const void *>((intptr_t)dot_fused),
            reinterpret_cast<const void *>((intptr_t)split)};  // L = 1: the split and pipelined forms share cg_graph
        if (ic)
            tri_graph_key(ic, key);
        st = solver_graph(h, h->cg_graph, key, K, iterate, "CG");
        exec = h->cg_graph.exec;
    }
    hipEvent_t evs[2] = {nullptr, nullptr};
    if (st == MSPMV_OK)
        st = solve_batches(h, K, max_iters, exec, poison, evs, "CG", iterate);
    if (st == MSPMV_OK && max_iters > 0 && !hm && !ic) {
        // pipelined: the last iteration's stop test (a no-op once the solve has stopped); both
        // forms: the deferred x += alpha p of the last update
        hipError_t ef = pipelined ? launch_cg1_finish(h, d_x, max_iters & 1, nblk) : launch_cg_xflush(h, d_x, L, nblk);
        if (ef != hipSuccess) {
            set_error(std::string("CG finish launch: ") + hipGetErrorString(ef));
            st = MSPMV_ERR_HIP;
        }
    }
    CgControl fin{};
    ST_TRY(solve_collect(h, st, evs, saved_cap, use_cap, iters, hist, &fin, "CG"));
    const int it = fin.done ? fin.iters_out : fin.iter;
    if (fin.breakdown == 2) {
        if (iters)
            *iters = fin.iter;
        set_error("IC(0) apply: a triangular-solve dependency never became ready (solve stalled)");
        return MSPMV_ERR_STALL;
    }
    if (fin.breakdown) {
        if (!pipelined && fin.done && fin.iters_out == fin.iter + 1 && hist && it >= 1 && it <= use_cap) {
            // The alpha test ended the solve (cg_alpha_finish: every column not yet converged broke down in
            // this iteration's p.Ap), so the update that records the iteration's history entry never ran and
            // the slot held what an earlier solve left there.  The entry is the reference's: the largest of
            // the converged columns' residuals, frozen since they converged -- a broken column's NaN is
            // skipped by its std::max -- and 0 when no column has converged.
            std::vector<CgScalars> sc((size_t)L);
            std::vector<unsigned char> cv((size_t)L);
            HIP_TRY(hipMemcpy(sc.data(), h->d_scal, sizeof(CgScalars) * (size_t)L, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(cv.data(), h->d_conv, (size_t)L, hipMemcpyDeviceToHost));
            double maxrel = 0.0;
            for (int j = 0; j < L; ++j)
                if (cv[(size_t)j] == 1) {
                    const double rel = std::sqrt(sc[(size_t)j].rs_new) / sc[(size_t)j].b_norm;
                    maxrel = maxrel < rel ? rel : maxrel;
                }
            hist[it - 1] = maxrel;
        }
        set_error(L == 1 ? "CG breakdown: p.Ap gave a non-finite alpha at iteration " + std::to_string(it)
                         : "CG breakdown: p.Ap gave a non-finite alpha in at least one column (frozen; the "
                           "other columns were solved)");
        return MSPMV_ERR_BREAKDOWN;
    }
    return MSPMV_OK;
}

// Any L: the reference's L lock-step recurrences are independent per column (per-column alpha,
// beta and converged masks, no_pretreatment.hpp:109-120,163-176), so a panel of width outside
// {1, 2, 4, 8, 16} (the reference's preconditioner_benchmark runs num_vectors = 32) is solved as
// column groups of native widths, each copied into a contiguous panel and back.  The iteration
// count is the groups' maximum; the history is the max over groups, a finished group's columns
// frozen at their last residual (alpha = 0 leaves r unchanged), as the reference records them.
// native(d_b, d_x, width, iters, hist, hist_cap): the solver on a panel of native width (cg_solve_native,
// bicgstab_solve_native); name / broke_msg: the solver's name and its breakdown report in the error text.
using NativeSolveFn = std::function<mspmv_status(const double *, double *, int, int *, double *, int)>;
static mspmv_status solve_dev_groups(mspmv_handle_s *h, const double *d_b, double *d_x, int L, int *iters,
                                     double *hist, int hist_cap, const NativeSolveFn &native, const char *name,
                                     const char *broke_msg)
{
    if (L < 1)
        return invalid("L must be >= 1");
    if (supported_L(L) || h->m == 0)
        return native(d_b, d_x, supported_L(L) ? L : 1, iters, hist, hist_cap);
    if (!d_b || !d_x)
        return invalid("null vector");
    const size_t m = (size_t)h->m;
    const int cap = hist ? std::max(hist_cap, 0) : 0;
    double *gb = nullptr, *gx = nullptr;
    ST_TRY(dev_alloc(&gb, m * 16));
    mspmv_status st = dev_alloc(&gx, m * 16);
    std::vector<std::vector<double>> gh;
    std::vector<int> git;
    int total = 0;
    bool faulted = false;  // a group's solve met a ticket fault (reported at the end)
    bool broke = false;  // a group's CG broke down: keep solving the other groups, report it at the end
    for (int c0 = 0; c0 < L && st == MSPMV_OK;) {
        const int w = native_chunk(L - c0);
        hipError_t e = launch_panel_copy(d_b + c0, L, gb, w, (long long)m, w, w, h->stream);
        if (e == hipSuccess && warm_start(h))  // the group's columns of X0, as B's
            e = launch_panel_copy(d_x + c0, L, gx, w, (long long)m, w, w, h->stream);
        if (e != hipSuccess) {
            set_error(std::string("column group copy: ") + hipGetErrorString(e));
            st = MSPMV_ERR_HIP;
            break;
        }
        std::vector<double> hg((size_t)cap);
        int it = 0;
        st = native(gb, gx, w, &it, cap ? hg.data() : nullptr, cap);
        if (st == MSPMV_ERR_BREAKDOWN) {
            broke = true;
            st = MSPMV_OK;
        } else if (st == MSPMV_ERR_FAULT) {  // the other groups still run (each solve re-zeroes its tickets)
            faulted = true;
            st = MSPMV_OK;
        }
        if (st == MSPMV_OK) {
            e = launch_panel_copy(gx, w, d_x + c0, L, (long long)m, w, w, h->stream);
            if (e == hipSuccess)
                e = hipStreamSynchronize(h->stream);
            if (e != hipSuccess) {
                set_error(std::string("column group copy: ") + hipGetErrorString(e));
                st = MSPMV_ERR_HIP;
            }
        }
        total = std::max(total, it);
        gh.push_back(std::move(hg));
        git.push_back(it);
        c0 += w;
    }
    dev_free(gb);
    dev_free(gx);
    if (st == MSPMV_OK && faulted) {
        set_error(std::string(name) +
                  ": a reduction ticket drew past its group in at least one column group: X is not a solution");
        st = MSPMV_ERR_FAULT;
    } else if (st == MSPMV_OK && broke) {
        set_error(broke_msg);
        st = MSPMV_ERR_BREAKDOWN;
    }
    if (iters)
        *iters = total;
    for (int k = 0; k < std::min(total, cap); ++k) {
        double v = 0.0;
        for (size_t g = 0; g < gh.size(); ++g)
            if (git[g] > 0)
                v = std::max(v, gh[g][(size_t)std::min(k, git[g] - 1)]);
        hist[k] = v;
    }
    return st;
}

static mspmv_status cg_solve_dev(mspmv_handle_s *h, const double *d_b, double *d_x, int L, int max_iters,
                                 double tol, int *iters, double *hist, int hist_cap, mspmv_handle_s *hm = nullptr,
                                 mspmv_ic0_s *ic = nullptr)
{
    return solve_dev_groups(
        h, d_b, d_x, L, iters, hist, hist_cap,
        [&](const double *b, double *x, int w, int *it, double *hg, int cap) {
            return cg_solve_native(h, b, x, w, max_iters, tol, it, hg, cap, hm, ic);
        },
        "CG",
        "CG breakdown: p.Ap gave a non-finite alpha in at least one column (frozen; the other columns were solved)");
}

// BiCGSTAB on a panel of native width (mspmv_bicgstab.hip), by cg_solve_native's protocol: control word and
// tickets zeroed on the handle's stream before the init, iterations in batches of cg_batch_iters with the
// control word copied back per batch, a batch replayed as a graph captured from the handle's one stream (a
// linear chain) and cached under the solver's own exec and key; fewer than a batch of iterations run ungraphed.
// ilu: the ILU(0) factor of the right-preconditioned form (launch_pbicgstab_iteration), else null.  The two forms
// share the handle's workspace and keep a cached graph each, so neither replays nor evicts the other's.
static mspmv_status bicgstab_solve_native(mspmv_handle_s *h, const double *d_b, double *d_x, int L, int max_iters,
                                          double tol, int *iters, double *hist, int hist_cap,
                                          mspmv_ilu0_s *ilu = nullptr)
{
    if (h->m != h->n)
        return invalid("BiCGSTAB needs a square matrix");
    if (ilu && (ilu->n != h->m || ilu->device != h->device))
        return invalid("the ILU(0) factor must match the matrix's shape and device");
    if (!supported_L(L))
        return (set_error("L must be one of 1, 2, 4, 8, 16"), MSPMV_ERR_UNSUPPORTED);
    if (max_iters < 0)
        return invalid("max_iters < 0");
    if (h->m > 0 && (!d_b || !d_x))
        return invalid("null vector");
    if (!aligned16(d_b) || !aligned16(d_x))
        return invalid("BiCGSTAB vectors must be 16-byte aligned");
    if (iters)
        *iters = 0;
    if (h->m == 0)
        return MSPMV_OK;
    // the two products run on the plan the handle's plain L-wide product takes (offset windows, column slabs),
    // else on the merge tiles: decided here, before any graph capture (it may copy the matrix to the host)
    const TilePlan *plan = nullptr, *splan = nullptr;
    ST_TRY(product_plan(h, L, &splan));
    if (!(splan->dia || (splan->slab && L > 1)))
        splan = nullptr;
    ST_TRY(solver_plan(h, L, &plan));
    const int nblk = cg_update_blocks((long long)h->m * L, h->num_cus);
    const int cap = hist ? std::max(hist_cap, 0) : 0;
    // partial rows of the two-dot folds are 2 L wide
    ST_TRY(ensure_cg_workspace(h, L, nblk, std::max(plan->num_tiles, splan ? splan->num_tiles : 0), cap, 2 * L));
    const size_t elems = (size_t)h->m * L;
    if (elems > h->rhat_cap) {
        dev_free(h->d_rhat);
        h->rhat_cap = 0;
        ST_TRY(dev_alloc(&h->d_rhat, elems));
        h->rhat_cap = elems;
    }
    if (ilu)  // the apply's intermediate and the hat panel live with the factor: grown here, before any capture
        ST_TRY(ilu0_workspace(ilu, elems));
    const char *name = ilu ? "ILU0-BiCGSTAB" : "BiCGSTAB";
    h->last_cg_kernel = ilu ? "ILU0-BiCGSTAB (2 SpMM + 4 trsv + 5 passes)" : "BiCGSTAB (2 SpMM + 5 passes)";
    if (ilu && ilu->num_colors > 0)
        h->last_cg_kernel =
            "MC-ILU0-BiCGSTAB (2 SpMM + 4 sweeps of " + std::to_string(ilu->num_colors) + " colours + 5 passes)";
    h->last_solver_product = solver_product_name(h, *plan, splan, L);
    const int use_cap = hist ? cap : 0;
    const int saved_cap = h->hist_cap;
    h->hist_cap = use_cap;  // kernels record only what the caller asked for
    int poison = 0;
    ST_TRY(solve_prologue(h, {plan, splan}, &poison));
    const bool warm = warm_start(h);
    if (warm)
        HIP_TRY(launch_warm_start(h, *plan, splan, d_b, d_x, L, nblk));
    HIP_TRY(launch_bicgstab_init(h, d_b, d_x, L, tol, nblk, warm));
    ST_TRY(solve_poison_fill(h, poison));
    auto iterate = [&](int) -> hipError_t {
        if (ilu)
            return launch_pbicgstab_iteration(h, ilu, *plan, splan, d_x, L, nblk, tol);
        return launch_bicgstab_iteration(h, *plan, splan, d_x, L, nblk, tol);
    };
    const int K = cg_batch_iters(h->m, h->nnz, L);
    mspmv_status st = MSPMV_OK;
    hipGraphExec_t exec = nullptr;
    if (max_iters >= K && !(poison & MSPMV_POISON_LATE_ZERO)) {
        const void *tk = nullptr;
        std::memcpy(&tk, &tol, sizeof tk);
        std::vector<const void *> key = {
            d_x, h->d_r, h->d_rhat, h->d_p0, h->d_p1, h->d_ap, h->d_partials, h->d_gtickets, h->d_scal, h->d_conv,
            h->d_red, h->d_ctrl, h->d_hist, h->stream, plan, splan, tk,
            reinterpret_cast<const void *>((intptr_t)L), reinterpret_cast<const void *>((intptr_t)nblk),
            reinterpret_cast<const void *>((intptr_t)use_cap), reinterpret_cast<const void *>((intptr_t)K)};
        if (ilu) {  // the factor and the hat panel
            tri_graph_key(ilu, key);
            key.push_back(ilu->d_hat);
        }
        GraphCache &g = ilu ? h->pbicg_graph : h->bicg_graph;
        st = solver_graph(h, g, key, K, iterate, name);
        exec = g.exec;
    }
    hipEvent_t evs[2] = {nullptr, nullptr};
    if (st == MSPMV_OK)
        st = solve_batches(h, K, max_iters, exec, poison, evs, name, iterate);
    CgControl fin{};
    ST_TRY(solve_collect(h, st, evs, saved_cap, use_cap, iters, hist, &fin, name));
    if (fin.breakdown == 2) {  // set by a triangular solve; a column freeze never overwrites it
        if (iters)
            *iters = fin.iter;
        set_error("ILU(0) apply: a triangular-solve dependency never became ready (solve stalled)");
        return MSPMV_ERR_STALL;
    }
    if (fin.breakdown) {
        set_error("BiCGSTAB breakdown: a non-finite alpha, omega or beta in at least one column (frozen; the other "
                  "columns were solved)");
        return MSPMV_ERR_BREAKDOWN;
    }
    return MSPMV_OK;
}

static mspmv_status bicgstab_solve_dev(mspmv_handle_s *h, const double *d_b, double *d_x, int L, int max_iters,
                                       double tol, int *iters, double *hist, int hist_cap,
                                       mspmv_ilu0_s *ilu = nullptr)
{
    return solve_dev_groups(
        h, d_b, d_x, L, iters, hist, hist_cap,
        [&](const double *b, double *x, int w, int *it, double *hg, int cap) {
            return bicgstab_solve_native(h, b, x, w, max_iters, tol, it, hg, cap, ilu);
        },
        ilu ? "ILU0-BiCGSTAB" : "BiCGSTAB",
        "BiCGSTAB breakdown: a non-finite alpha, omega or beta in at least one column (frozen; the other columns "
        "were solved)");
}

// Block CG (BCGrQ, mspmv_blockcg.hip) on a panel of native width, by bicgstab_solve_native's protocol and plan
// choice: one product per iteration on the plan the handle's plain L-wide product takes (offset windows, column
// slabs), else on the merge tiles; the iteration graph cached under the solver's own exec and key.  The columns
// share one Krylov space, so there are no column groups: any other width is MSPMV_ERR_UNSUPPORTED.
static mspmv_status bcg_solve_native(mspmv_handle_s *h, const double *d_b, double *d_x, int L, int max_iters,
                                     double tol, int *iters, double *hist, int hist_cap)
{
    if (h->m != h->n)
        return invalid("block CG needs a square matrix");
    if (!supported_L(L))
        return (set_error("block CG: L must be one of 1, 2, 4, 8, 16 (the columns are coupled: no column groups)"),
                MSPMV_ERR_UNSUPPORTED);
    if (max_iters < 0)
        return invalid("max_iters < 0");
    if (h->m > 0 && (!d_b || !d_x))
        return invalid("null vector");
    if (!aligned16(d_b) || !aligned16(d_x))
        return invalid("block CG vectors must be 16-byte aligned");
    if (iters)
        *iters = 0;
    if (h->m == 0)
        return MSPMV_OK;
    const TilePlan *plan = nullptr, *splan = nullptr;
    ST_TRY(product_plan(h, L, &splan));
    if (!(splan->dia || (splan->slab && L > 1)))
        splan = nullptr;
    ST_TRY(solver_plan(h, L, &plan));
    const int nblk = cg_update_blocks((long long)h->m * L, h->num_cus);
    const int cap = hist ? std::max(hist_cap, 0) : 0;
    // partial rows of the Gram folds are L^2 wide, one per block of the passes: the products take no partials
    ST_TRY(ensure_cg_workspace(h, L, nblk, 0, cap, std::max(L * L, 2 * L)));  // (2 L: the warm start's pass)
    if (!h->d_bcg)
        ST_TRY(dev_alloc(&h->d_bcg, (size_t)kBcgSmallDoubles));
    h->last_cg_kernel = "BlockCG-rQ (1 SpMM + 3 passes)";
    h->last_solver_product = solver_product_name(h, *plan, splan, L);
    const int use_cap = hist ? cap : 0;
    const int saved_cap = h->hist_cap;
    h->hist_cap = use_cap;  // kernels record only what the caller asked for
    int poison = 0;
    ST_TRY(solve_prologue(h, {plan, splan}, &poison));
    const bool warm = warm_start(h);
    if (warm)
        HIP_TRY(launch_warm_start(h, *plan, splan, d_b, d_x, L, nblk));
    HIP_TRY(launch_bcg_init(h, d_b, d_x, L, tol, nblk, warm));
    ST_TRY(solve_poison_fill(h, poison));
    auto iterate = [&](int) -> hipError_t { return launch_bcg_iteration(h, *plan, splan, d_x, L, nblk, tol); };
    const int K = cg_batch_iters(h->m, h->nnz, L);
    mspmv_status st = MSPMV_OK;
    hipGraphExec_t exec = nullptr;
    if (max_iters >= K && !(poison & MSPMV_POISON_LATE_ZERO)) {
        const void *tk = nullptr;
        std::memcpy(&tk, &tol, sizeof tk);
        std::vector<const void *> key = {
            d_x, h->d_r, h->d_p0, h->d_ap, h->d_partials, h->d_gtickets, h->d_bcg, h->d_ctrl, h->d_hist, h->stream,
            plan, splan, tk, reinterpret_cast<const void *>((intptr_t)L),
            reinterpret_cast<const void *>((intptr_t)nblk), reinterpret_cast<const void *>((intptr_t)use_cap),
            reinterpret_cast<const void *>((intptr_t)K)};
        st = solver_graph(h, h->bcg_graph, key, K, iterate, "block CG");
        exec = h->bcg_graph.exec;
    }
    hipEvent_t evs[2] = {nullptr, nullptr};
    if (st == MSPMV_OK)
        st = solve_batches(h, K, max_iters, exec, poison, evs, "block CG", iterate);
    CgControl fin{};
    ST_TRY(solve_collect(h, st, evs, saved_cap, use_cap, iters, hist, &fin, "block CG"));
    if (fin.breakdown) {
        const bool of_g = (fin.breakdown & kBcgBrokeG) != 0;
        set_error(std::string("block CG breakdown: pivot ") + std::to_string(fin.breakdown & 0xf) + " of " +
                  (of_g ? "G = S^T A S" : "H = V^T V") + " is <= 0 or non-finite " +
                  (fin.iter == 0 && !of_g ? warm ? "at the init (a zero or dependent column of the initial residuals)"
                                                  : "at the init (a zero or dependent right-hand-side column)"
                                          : "in iteration " + std::to_string(fin.iter - (of_g ? 0 : 1))) +
                  "; the block is rank deficient -- solve the columns independently with mspmv_dcg_multi");
        return MSPMV_ERR_BREAKDOWN;
    }
    return MSPMV_OK;
}

// Host-pointer form of a device solve: B up (and X, the initial guess, on a warm-start handle), solve_dev(dB, dX),
// X down (also after a breakdown: the other columns were solved).
static mspmv_status solve_host(mspmv_handle h, const double *B, double *X, int L, int *iters,
                               const std::function<mspmv_status(const double *, double *)> &solve_dev)
{
    ST_TRY(check_handle(h));
    if (h->m == 0) {
        if (iters)
            *iters = 0;
        return MSPMV_OK;
    }
    if (!B || !X)
        return invalid("null vector");
    double *dB = nullptr, *dX = nullptr;
    const size_t bytes = sizeof(double) * (size_t)h->m * L;
    ST_TRY(dev_alloc(&dB, (size_t)h->m * L));
    mspmv_status st = dev_alloc(&dX, (size_t)h->m * L);
    if (st == MSPMV_OK && hipMemcpy(dB, B, bytes, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("B upload failed");
        st = MSPMV_ERR_HIP;
    }
    if (st == MSPMV_OK && warm_start(h) && hipMemcpy(dX, X, bytes, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("X0 upload failed");
        st = MSPMV_ERR_HIP;
    }
    if (st == MSPMV_OK)
        st = solve_dev(dB, dX);
    if ((st == MSPMV_OK || st == MSPMV_ERR_BREAKDOWN) && hipMemcpy(X, dX, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("X download failed");
        st = MSPMV_ERR_HIP;
    }
    dev_free(dB);
    dev_free(dX);
    return st;
}

static mspmv_status cg_solve_host(mspmv_handle h, const double *B, double *X, int L, int max_iters, double tol,
                                  int *iters, double *hist, int hist_cap, mspmv_handle hm = nullptr,
                                  mspmv_ic0 ic = nullptr)
{
    return solve_host(h, B, X, L, iters, [&](const double *dB, double *dX) {
        return cg_solve_dev(h, dB, dX, L, max_iters, tol, iters, hist, hist_cap, hm, ic);
    });
}

extern "C" {

mspmv_status mspmv_dcg_single_dev(mspmv_handle h, const double *d_b, double *d_x, int max_iters, double tolerance,
                                  int *iters, double *resid_hist, int hist_cap)
{
    ST_TRY(check_handle(h));
    return cg_solve_dev(h, d_b, d_x, 1, max_iters, tolerance, iters, resid_hist, hist_cap);
}

mspmv_status mspmv_cg_resident_stamps(mspmv_handle h, const double *d_b, double *d_x, int max_iters, double tolerance,
                                      int *iters, unsigned long long *stamps, int stamp_iters, int *workgroups)
{
    ST_TRY(check_handle(h));
    if (!d_b || !d_x || !stamps || stamp_iters < 1 || max_iters < 0)
        return invalid("cg_resident_stamps: vectors, stamps and stamp_iters >= 1 required");
    if (!aligned16(d_b) || !aligned16(d_x))
        return invalid("CG vectors must be 16-byte aligned");
    if (h->m < 1 || h->m != h->n)
        return invalid("CG needs a non-empty square matrix");
    HIP_TRY(hipSetDevice(h->device));
    const TilePlan *plan = nullptr;
    ST_TRY(solver_plan(h, 1, &plan));
    ST_TRY(ensure_cg_workspace(h, 1, cg1_blocks(h->m), plan->num_tiles, 0));
    ResidentCg *rc = nullptr;
    ST_TRY(resident_for(h, &rc));
    if (!rc)
        return (set_error("cg_resident_stamps: this matrix does not take the register-resident CG"),
                MSPMV_ERR_UNSUPPORTED);
    const size_t n = (size_t)stamp_iters * rc->G * 5;
    unsigned long long *d_st = nullptr;
    ST_TRY(dev_alloc(&d_st, n));
    mspmv_status st = MSPMV_OK;
    if (hipMemsetAsync(d_st, 0, sizeof(unsigned long long) * n, h->stream) != hipSuccess) {
        set_error("cg_resident_stamps: memset failed");
        st = MSPMV_ERR_HIP;
    }
    if (st == MSPMV_OK)
        st = cg_solve_resident(h, rc, d_b, d_x, max_iters, tolerance, iters, nullptr, 0, d_st, stamp_iters);
    if (st == MSPMV_OK && hipMemcpy(stamps, d_st, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("cg_resident_stamps: download failed");
        st = MSPMV_ERR_HIP;
    }
    dev_free(d_st);
    if (workgroups)
        *workgroups = rc->G;
    return st;
}

mspmv_status mspmv_dcg_single(mspmv_handle h, const double *b, double *x, int max_iters, double tolerance,
                              int *iters, double *resid_hist, int hist_cap)
{
    return cg_solve_host(h, b, x, 1, max_iters, tolerance, iters, resid_hist, hist_cap);
}

mspmv_status mspmv_dcg_multi_dev(mspmv_handle h, const double *d_B, double *d_X, int L, int max_iters,
                                 double tolerance, mspmv_spmm_kernel kernel, int *iters, double *max_err_hist,
                                 int hist_cap)
{
    (void)kernel;  // the GPU always runs the merge-path SpMM
    ST_TRY(check_handle(h));
    return cg_solve_dev(h, d_B, d_X, L, max_iters, tolerance, iters, max_err_hist, hist_cap);
}

mspmv_status mspmv_dcg_multi(mspmv_handle h, const double *B, double *X, int L, int max_iters, double tolerance,
                             mspmv_spmm_kernel kernel, int *iters, double *max_err_hist, int hist_cap)
{
    (void)kernel;
    return cg_solve_host(h, B, X, L, max_iters, tolerance, iters, max_err_hist, hist_cap);
}

mspmv_status mspmv_dbicgstab_multi_dev(mspmv_handle h, const double *d_B, double *d_X, int L, int max_iters,
                                       double tolerance, int *iters, double *max_err_hist, int hist_cap)
{
    ST_TRY(check_handle(h));
    return bicgstab_solve_dev(h, d_B, d_X, L, max_iters, tolerance, iters, max_err_hist, hist_cap);
}

mspmv_status mspmv_dbicgstab_multi(mspmv_handle h, const double *B, double *X, int L, int max_iters, double tolerance,
                                   int *iters, double *max_err_hist, int hist_cap)
{
    return solve_host(h, B, X, L, iters, [&](const double *dB, double *dX) {
        return bicgstab_solve_dev(h, dB, dX, L, max_iters, tolerance, iters, max_err_hist, hist_cap);
    });
}

mspmv_status mspmv_solver_pass_shape(mspmv_handle h, int L, int *pass_blocks, int *batch_iters)
{
    ST_TRY(check_handle(h));
    if (!supported_L(L))
        return (set_error("L must be one of 1, 2, 4, 8, 16"), MSPMV_ERR_UNSUPPORTED);
    if (pass_blocks)
        *pass_blocks = cg_update_blocks((long long)h->m * L, h->num_cus);
    if (batch_iters)
        *batch_iters = cg_batch_iters(h->m, h->nnz, L);
    return MSPMV_OK;
}

mspmv_status mspmv_dbcg_multi_dev(mspmv_handle h, const double *d_B, double *d_X, int L, int max_iters,
                                  double tolerance, int *iters, double *max_err_hist, int hist_cap)
{
    ST_TRY(check_handle(h));
    return bcg_solve_native(h, d_B, d_X, L, max_iters, tolerance, iters, max_err_hist, hist_cap);
}

mspmv_status mspmv_dbcg_multi(mspmv_handle h, const double *B, double *X, int L, int max_iters, double tolerance,
                              int *iters, double *max_err_hist, int hist_cap)
{
    if (h && !supported_L(L))  // before the panels are sized by L
        return (set_error("block CG: L must be one of 1, 2, 4, 8, 16 (the columns are coupled: no column groups)"),
                MSPMV_ERR_UNSUPPORTED);
    return solve_host(h, B, X, L, iters, [&](const double *dB, double *dX) {
        return bcg_solve_native(h, dB, dX, L, max_iters, tolerance, iters, max_err_hist, hist_cap);
    });
}

mspmv_status mspmv_dpbicgstab_ilu0_multi_dev(mspmv_handle a, mspmv_ilu0 m, const double *d_B, double *d_X, int L,
                                             int max_iters, double tolerance, int *iters, double *max_err_hist,
                                             int hist_cap)
{
    ST_TRY(check_handle(a));
    if (!m)
        return invalid("null ILU(0) factor");
    return bicgstab_solve_dev(a, d_B, d_X, L, max_iters, tolerance, iters, max_err_hist, hist_cap, m);
}

mspmv_status mspmv_dpbicgstab_ilu0_multi(mspmv_handle a, mspmv_ilu0 m, const double *B, double *X, int L,
                                         int max_iters, double tolerance, int *iters, double *max_err_hist,
                                         int hist_cap)
{
    if (!m)
        return invalid("null ILU(0) factor");
    return solve_host(a, B, X, L, iters, [&](const double *dB, double *dX) {
        return bicgstab_solve_dev(a, dB, dX, L, max_iters, tolerance, iters, max_err_hist, hist_cap, m);
    });
}

mspmv_status mspmv_dpcg_spai_multi_dev(mspmv_handle a, mspmv_handle m, const double *d_B, double *d_X, int L,
                                       int max_iters, double tolerance, mspmv_spmm_kernel kernel, int *iters,
                                       double *max_err_hist, int hist_cap)
{
    (void)kernel;  // the GPU always runs the merge-path SpMM
    ST_TRY(check_handle(a));
    ST_TRY(check_handle(m));
    return cg_solve_dev(a, d_B, d_X, L, max_iters, tolerance, iters, max_err_hist, hist_cap, m);
}

mspmv_status mspmv_dpcg_spai_multi(mspmv_handle a, mspmv_handle m, const double *B, double *X, int L, int max_iters,
                                   double tolerance, mspmv_spmm_kernel kernel, int *iters, double *max_err_hist,
                                   int hist_cap)
{
    (void)kernel;
    ST_TRY(check_handle(m));
    return cg_solve_host(a, B, X, L, max_iters, tolerance, iters, max_err_hist, hist_cap, m);
}

// ---- warm start and the fused true residual (mspmv_warm.hip) -------------------------------------
mspmv_status mspmv_set_initial_guess(mspmv_handle h, int mode, int *old)
{
    if (mode != MSPMV_X0_ZERO && mode != MSPMV_X0_CALLER)
        return invalid("set_initial_guess: unknown mode");
    if (!h)
        return invalid("null handle");
    if (old)
        *old = h->x0_mode;
    h->x0_mode = mode;  // the inits run outside the cached iteration graphs: nothing to drop
    return MSPMV_OK;
}

// One native-width panel: W = A X on the plain product's plan into h->d_resw (the one m x w panel this entry needs:
// a handle never solved on allocates no solver workspace for it), then k_warm_residual; the 2 w sums to the host.
// The pass's own tickets are zeroed first (a solve that stopped early may have left some raised) and a ticket fault
// comes back in the control word.
static mspmv_status residual_native(mspmv_handle_s *h, const double *d_B, const double *d_X, double *d_R, int w,
                                    double *sums)
{
    const TilePlan *plan = nullptr;
    ST_TRY(product_plan(h, w, &plan));
    const int nblk = cg_update_blocks((long long)h->m * w, h->num_cus);
    ST_TRY(ensure_fold_workspace(h, (size_t)nblk, 2 * w));
    const size_t elems = (size_t)h->m * w;
    if (elems > h->resw_cap) {
        dev_free(h->d_resw);
        h->resw_cap = 0;
        ST_TRY(dev_alloc(&h->d_resw, elems));
        h->resw_cap = elems;
    }
    HIP_TRY(hipMemsetAsync(h->d_ctrl, 0, sizeof(CgControl), h->stream));
    HIP_TRY(hipMemsetAsync(h->d_gtickets, 0, sizeof(unsigned) * gtickets_capacity((size_t)nblk), h->stream));
    int nk = 0;
    HIP_TRY(launch_spmm(h, *plan, d_X, h->d_resw, w, &nk));
    HIP_TRY(launch_warm_residual(h, d_B, h->d_resw, d_R, w, nblk));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(sums, h->d_warm, sizeof(double) * 2 * w, hipMemcpyDeviceToHost));
    CgControl fin{};
    HIP_TRY(hipMemcpy(&fin, h->d_ctrl, sizeof fin, hipMemcpyDeviceToHost));
    if (fin.fault) {
        set_error("residual: a reduction ticket drew past its group (the ticket array was not zero when the fold "
                  "began): the norms are invalid");
        return MSPMV_ERR_FAULT;
    }
    return MSPMV_OK;
}

mspmv_status mspmv_dresidual_dev(mspmv_handle h, const double *d_B, const double *d_X, double *d_R, int L,
                                 double *norms)
{
    ST_TRY(check_handle(h));
    if (L < 1)
        return invalid("L must be >= 1");
    if (!norms)
        return invalid("residual: null norms");
    if ((h->m > 0 && !d_B) || (h->m > 0 && h->n > 0 && !d_X))
        return invalid("null vector");
    for (int j = 0; j < 2 * L; ++j)
        norms[j] = 0.0;
    if (h->m == 0)
        return MSPMV_OK;
    double sums[32];
    mspmv_status st = MSPMV_OK;
    if (supported_L(L)) {
        if (!aligned16(d_B) || !aligned16(d_X) || !aligned16(d_R))
            return invalid("residual panels must be 16-byte aligned");
        st = residual_native(h, d_B, d_X, d_R, L, sums);
        for (int j = 0; st == MSPMV_OK && j < L; ++j) {
            norms[j] = std::sqrt(sums[j]);
            norms[L + j] = std::sqrt(sums[L + j]);
        }
    } else {
        // column groups of native widths, each copied into contiguous panels (solve_dev_groups' way)
        double *gb = nullptr, *gx = nullptr, *gr = nullptr;
        ST_TRY(dev_alloc(&gb, (size_t)h->m * 16));
        st = dev_alloc(&gx, (size_t)h->n * 16);
        if (st == MSPMV_OK && d_R)
            st = dev_alloc(&gr, (size_t)h->m * 16);
        for (int c0 = 0; c0 < L && st == MSPMV_OK;) {
            const int w = native_chunk(L - c0);
            hipError_t e = launch_panel_copy(d_B + c0, L, gb, w, h->m, w, w, h->stream);
            if (e == hipSuccess)
                e = launch_panel_copy(d_X + c0, L, gx, w, h->n, w, w, h->stream);
            if (e == hipSuccess)
                st = residual_native(h, gb, gx, gr, w, sums);
            if (e == hipSuccess && st == MSPMV_OK && d_R) {
                e = launch_panel_copy(gr, w, d_R + c0, L, h->m, w, w, h->stream);
                if (e == hipSuccess)
                    e = hipStreamSynchronize(h->stream);
            }
            if (e != hipSuccess) {
                set_error(std::string("residual column group: ") + hipGetErrorString(e));
                st = MSPMV_ERR_HIP;
            }
            for (int j = 0; st == MSPMV_OK && j < w; ++j) {
                norms[c0 + j] = std::sqrt(sums[j]);
                norms[L + c0 + j] = std::sqrt(sums[w + j]);
            }
            c0 += w;
        }
        dev_free(gb);
        dev_free(gx);
        dev_free(gr);
    }
    if (st == MSPMV_OK)
        st = mspmv_check_faults(h);  // the product's own tickets, as mspmv_dspmm
    return st;
}

mspmv_status mspmv_dresidual(mspmv_handle h, const double *B, const double *X, double *R, int L, double *norms)
{
    ST_TRY(check_handle(h));
    if (L < 1)
        return invalid("L must be >= 1");
    if (!norms)
        return invalid("residual: null norms");
    if ((h->m > 0 && !B) || (h->m > 0 && h->n > 0 && !X))
        return invalid("null vector");
    double *dB = nullptr, *dX = nullptr, *dR = nullptr;
    const size_t mb = (size_t)h->m * L, nb = (size_t)h->n * L;
    ST_TRY(dev_alloc(&dB, mb));
    mspmv_status st = dev_alloc(&dX, nb);
    if (st == MSPMV_OK && R)
        st = dev_alloc(&dR, mb);
    if (st == MSPMV_OK && (hipMemcpy(dB, B, sizeof(double) * mb, hipMemcpyHostToDevice) != hipSuccess ||
                           hipMemcpy(dX, X, sizeof(double) * nb, hipMemcpyHostToDevice) != hipSuccess)) {
        set_error("residual: upload failed");
        st = MSPMV_ERR_HIP;
    }
    if (st == MSPMV_OK)
        st = mspmv_dresidual_dev(h, dB, dX, dR, L, norms);
    if (st == MSPMV_OK && R && hipMemcpy(R, dR, sizeof(double) * mb, hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("residual: download failed");
        st = MSPMV_ERR_HIP;
    }
    dev_free(dB);
    dev_free(dX);
    dev_free(dR);
    return st;
}

// ---- IC(0)-preconditioned CG (the factor: mspmv_tri.hip) ---------------------------------------
mspmv_status mspmv_dpcg_ic0_multi_dev(mspmv_handle a, mspmv_ic0 m, const double *d_B, double *d_X, int L,
                                      int max_iters, double tolerance, mspmv_spmm_kernel kernel, int *iters,
                                      double *max_err_hist, int hist_cap)
{
    (void)kernel;
    ST_TRY(check_handle(a));
    if (!m)
        return invalid("null IC(0) factor");
    return cg_solve_dev(a, d_B, d_X, L, max_iters, tolerance, iters, max_err_hist, hist_cap, nullptr, m);
}

mspmv_status mspmv_dpcg_ic0_multi(mspmv_handle a, mspmv_ic0 m, const double *B, double *X, int L, int max_iters,
                                  double tolerance, mspmv_spmm_kernel kernel, int *iters, double *max_err_hist,
                                  int hist_cap)
{
    (void)kernel;
    if (!m)
        return invalid("null IC(0) factor");
    return cg_solve_host(a, B, X, L, max_iters, tolerance, iters, max_err_hist, hist_cap, nullptr, m);
}
}  // extern "C"

// mspmv_cg_passes.hip -- the CG layer above the products: the streaming vector passes of the split
// (multi-RHS) iteration, the pipelined single-RHS CG's passes, the row-sharded CG's passes, the
// k_fold_dot reduction, and the per-iteration launchers of plain, split, SPAI and IC(0) CG.  The
// products themselves live in mspmv_kernels.hip (merge-path tiles), mspmv_dia.hip (offset windows)
// and mspmv_slab.hip (column slabs), the IC(0) apply in mspmv_tri.hip (tri_apply); this file
// reaches them through the launchers declared in mspmv_internal.h only.
// Compiled with -ffp-contract=off like every kernel here: every a*b+c is two roundings.
#include "mspmv_internal.h"
#include "mspmv_device.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

namespace mspmv {

// (reduce_slots, kConvBroken, colpair_block_reduce, for_pairs: mspmv_device.h, shared with mspmv_bicgstab.hip)

// What the fold's last block derives from the totals (k_fold_dot `mode`).
enum : int { kFoldDot = 0, kFoldCgAlpha = 1, kFoldPcgAlpha = 2, kFoldPcgBeta = 3, kFoldPcgInit = 4 };

// Split CG, after p.Ap of column j is known (one thread per column): the per-column breakdown
// (no_pretreatment.hpp:109-120 has no guard: a zero RHS column gives alpha = 0/0 and a NaN column
// that never converges).  The column is frozen (conv = kConvBroken: alpha = beta = 0 from here on,
// x and r keep their last finite values, left out of the max-error history as the reference's NaN
// is) and the other columns keep iterating.
__device__ __forceinline__ void cg_alpha_column(int j, double pAp, const CgScalars *scal, const unsigned char *conv,
                                                CgControl *ctrl)
{
    if (conv[j])
        return;
    const double alpha = scal[j].rs_old / pAp;
    if (!(alpha == alpha && fabs(alpha) < HUGE_VAL)) {
        const_cast<unsigned char *>(conv)[j] = kConvBroken;
        ctrl->breakdown = 1;
    }
}

// ... then (after a barrier, thread 0): the deferred x term was applied by the p update before
// this reduction (CgVecArgs::lazy_x), and every column converged or broken stops the solve here.
template <int L>
__device__ __forceinline__ void cg_alpha_finish(const unsigned char *conv, CgControl *ctrl)
{
    if (threadIdx.x != 0)
        return;
    ctrl->x_pending = 0;
    if (ctrl->breakdown) {
        int live = 0;
        for (int j = 0; j < L; ++j)
            live += conv[j] == 0;
        if (live == 0) {
            ctrl->done = 1;
            ctrl->iters_out = ctrl->iter + 1;
        }
    }
}

// x.(A x) per column from the tile kernels' MODE 2 partials [T][L], in a fixed order: block g
// folds tiles [g*q, g*q + q) (fold_cols), reduce_slots folds the block sums and its last block
// writes dot_out.  The tile kernels thus end without any ticket or store drain (a ticket per
// tile cost the L = 8 SpMM ~40 % on the nlpkkt120 shape).  scal given (single-GPU split CG): a
// non-finite alpha = rs_old / dot stops the solve before the update touches x and r.
template <int L>
__global__ __launch_bounds__(kBlock) void k_fold_dot(const double *part, int T, int q, double *lvl,
                                                     unsigned *tickets, double *dot_out, CgScalars *scal,
                                                     const unsigned char *conv, CgControl *ctrl, int mode)
{
    __shared__ double s_tmp[kBlock];
    __shared__ double s_out[L];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    if (ctrl && ctrl->done)
        return;
    const int t0 = min((int)blockIdx.x * q, T);
    fold_cols<L>(part + (size_t)t0 * L, min(q, T - t0), s_tmp, s_out);
    if (tid < L) {
        store_sc1(&lvl[(size_t)blockIdx.x * L + tid], s_out[tid]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (!reduce_slots<L, true>(lvl, tickets, blockIdx.x, gridDim.x, s_tmp, s_out, &s_last, ctrl))
        return;
    if (tid < L) {
        const double d = s_out[tid];
        dot_out[tid] = d;
        if (mode == kFoldCgAlpha) {
            cg_alpha_column(tid, d, scal, conv, ctrl);
        } else if (mode == kFoldPcgAlpha) {  // sparse_approximate_inverse.hpp:131-138
            CgScalars &s = scal[tid];
            s.pAp = d;
            s.alpha = (!conv[tid] && d != 0.0) ? s.rs_old / d : 0.0;
        } else if (mode == kFoldPcgBeta) {  // :200-210 (rs_old <- rs_new for every column)
            CgScalars &s = scal[tid];
            s.beta = (!conv[tid] && s.rs_old != 0.0) ? d / s.rs_old : 0.0;
            s.rs_old = d;
        } else if (mode == kFoldPcgInit) {  // :99-100
            scal[tid].rs_old = d;
        }
    }
    if (mode == kFoldCgAlpha) {
        __syncthreads();
        cg_alpha_finish<L>(conv, ctrl);
    }
}

// ------------------------------------------------------------------------------------------
// CG: init and the fused update (x += alpha p; r += (-alpha) Ap; r.r; stop test; beta)
// ------------------------------------------------------------------------------------------
// (CgVecArgs: mspmv_internal.h)

// x = 0, r = p0 = b; rs_old_j = r_j.r_j, b_norm_j = sqrt(b_j.b_j) (no_pretreatment.hpp:61-79,
// single_strategy.hpp:120-131).
// WARM (mspmv_set_initial_guess): x is kept and a.p = a.r holds R0 = B - A X0 (k_warm_residual), taken where the
// cold init takes b -- same grid, sweep and fold, so R0.R0 has the cold B.B's bits when X0 = 0; b_norm_j comes from
// bb_in (B_j.B_j, folded in this fold's order); a column with sqrt(R0_j.R0_j) / b_norm_j < tol starts converged,
// and all of them end the solve here with 0 iterations.
template <int L, bool WARM = false>
__global__ __launch_bounds__(kBlock) void k_cg_init(CgVecArgs a)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    __shared__ double2 s_red2[kBlock / 64][GL];
    __shared__ double s_colred[kBlock];
    __shared__ double s_out[L];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const long long npairs = a.n_elems / 2;
    const long long stride = (long long)gridDim.x * kBlock;
    double2 acc = make_double2(0.0, 0.0);
    for (long long i = (long long)blockIdx.x * kBlock + tid; i < npairs; i += stride) {
        const double2 b = reinterpret_cast<const double2 *>(a.p)[i];
        if (!WARM) {
            reinterpret_cast<double2 *>(a.x)[i] = make_double2(0.0, 0.0);
            reinterpret_cast<double2 *>(a.r)[i] = b;
        }
        reinterpret_cast<double2 *>(a.p0)[i] = b;
        acc.x += b.x * b.x;
        acc.y += b.y * b.y;
    }
    if ((a.n_elems & 1) && blockIdx.x == 0 && tid == 0) {  // L == 1 with odd n
        const long long i = a.n_elems - 1;
        const double b = a.p[i];
        if (!WARM) {
            a.x[i] = 0.0;
            a.r[i] = b;
        }
        a.p0[i] = b;
        acc.x += b * b;
    }
    colpair_block_reduce<L>(acc, s_red2, a.partials + (size_t)blockIdx.x * L);
    if (!reduce_slots<L>(a.partials, a.gtickets, blockIdx.x, gridDim.x, s_colred, s_out, &s_last, a.ctrl))
        return;
    if (a.red_out) {
        if (tid < L)
            a.red_out[tid] = s_out[tid];
    } else {
        if (tid < L) {
            CgScalars &s = a.scal[tid];
            const double bb = s_out[tid];
            s.rs_old = bb;
            double bn = sqrt(WARM ? a.bb_in[tid] : bb);
            s.b_norm = bn == 0.0 ? 1.0 : bn;
            s.alpha = 0.0;
            s.beta = 0.0;
            s.pAp = 0.0;
            s.rs_new = 0.0;
            a.conv[tid] = WARM && sqrt(bb) / s.b_norm < a.tol ? 1 : 0;  // a NaN ratio: not converged
        }
        if (WARM)
            __syncthreads();
        if (tid == 0) {
            int nconv = 0;
            if (WARM)
                for (int j = 0; j < L; ++j)
                    nconv += a.conv[j] != 0;
            a.ctrl->iter = 0;
            a.ctrl->done = WARM && nconv == L;
            a.ctrl->iters_out = 0;
            a.ctrl->breakdown = 0;
        }
    }
}

// x += alpha p (AxpySingle / axpy_multiple), r += (-alpha) Ap, rs_new = r.r, then on the last
// block: convergence with the reference's masks, history, beta, rs_old
// (single_strategy.hpp:143-163; no_pretreatment.hpp:122-182).
template <int L>
__global__ __launch_bounds__(kBlock) void k_cg_update(CgVecArgs a)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    __shared__ double2 s_red2[kBlock / 64][GL];
    __shared__ double s_colred[kBlock];
    __shared__ double s_out[L];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    if (a.ctrl->done)
        return;
    const long long npairs = a.n_elems / 2;
    const long long stride = (long long)gridDim.x * kBlock;
    const long long i0 = (long long)blockIdx.x * kBlock + tid;
    double2 al;
    if (a.red_in) {  // alpha_j = rs_old_j / (reduced p.Ap)_j, masked (no_pretreatment.hpp:109-120)
        // A non-finite alpha (breakdown of column j) applies as 0: x_j and r_j stay finite and
        // the column is frozen (k_fold_dot on one GPU, k_dist_finish when sharded).
        auto masked = [&](int j) {
            const double al = a.conv[j] ? 0.0 : a.scal[j].rs_old / a.red_in[j];
            return (al == al && fabs(al) < HUGE_VAL) ? al : 0.0;
        };
        const int j0 = L == 1 ? 0 : 2 * (int)(i0 % GL);
        al.x = masked(j0);
        al.y = L == 1 ? al.x : masked(j0 + 1);
    } else if (L == 1) {
        al.x = a.scal[0].alpha;
        al.y = al.x;
    } else {
        const int cp = (int)(i0 % GL);
        al.x = a.scal[2 * cp].alpha;
        al.y = a.scal[2 * cp + 1].alpha;
    }
    const double2 nal = make_double2(-al.x, -al.y);
    double2 acc = make_double2(0.0, 0.0);
    if (a.lazy_x) {  // x += alpha p: deferred to the next p update (CgVecArgs::lazy_x)
        (void)stride;
        for_pairs<GL>(npairs, 0, [&](long long i) {
            const v2d_t qv = __builtin_nontemporal_load(reinterpret_cast<const v2d_t *>(a.ap) + i);
            const double2 q = make_double2(qv[0], qv[1]);
            double2 r = reinterpret_cast<double2 *>(a.r)[i];
            r.x = r.x + nal.x * q.x;
            r.y = r.y + nal.y * q.y;
            reinterpret_cast<double2 *>(a.r)[i] = r;
            acc.x += r.x * r.x;
            acc.y += r.y * r.y;
        });
    } else {
        for (long long i = i0; i < npairs; i += stride) {
            const double2 p = reinterpret_cast<const double2 *>(a.p)[i];
            const double2 q = reinterpret_cast<const double2 *>(a.ap)[i];
            double2 x = reinterpret_cast<double2 *>(a.x)[i];
            double2 r = reinterpret_cast<double2 *>(a.r)[i];
            x.x = x.x + al.x * p.x;
            x.y = x.y + al.y * p.y;
            r.x = r.x + nal.x * q.x;
            r.y = r.y + nal.y * q.y;
            reinterpret_cast<double2 *>(a.x)[i] = x;
            reinterpret_cast<double2 *>(a.r)[i] = r;
            acc.x += r.x * r.x;
            acc.y += r.y * r.y;
        }
    }
    if ((a.n_elems & 1) && blockIdx.x == 0 && tid == 0) {
        const long long i = a.n_elems - 1;
        if (!a.lazy_x)
            a.x[i] = a.x[i] + al.x * a.p[i];
        const double r = a.r[i] + nal.x * a.ap[i];
        a.r[i] = r;
        acc.x += r * r;
    }
    colpair_block_reduce<L>(acc, s_red2, a.partials + (size_t)blockIdx.x * L);
    if (!reduce_slots<L>(a.partials, a.gtickets, blockIdx.x, gridDim.x, s_colred, s_out, &s_last, a.ctrl))
        return;
    if (a.red_out) {
        if (tid < L)
            a.red_out[tid] = s_out[tid];
    } else {
        if (tid == 0) {
            if (a.lazy_x) {  // this iteration's alpha per column (as every block formed it above,
                             // before the masks below change), for the deferred x += alpha p
                for (int j = 0; j < L; ++j) {
                    const double aj = a.conv[j] ? 0.0 : a.scal[j].rs_old / a.red_in[j];
                    a.scal[j].alpha = (aj == aj && fabs(aj) < HUGE_VAL) ? aj : 0.0;
                }
                a.ctrl->x_pending = 1;
            }
            const int iter = a.ctrl->iter;
            int nconv = 0;
            double maxrel = 0.0;
            for (int j = 0; j < L; ++j) {
                CgScalars &s = a.scal[j];
                const double rs_new = s_out[j];
                s.rs_new = rs_new;
                const double rel = sqrt(rs_new) / s.b_norm;
                // std::max(max, rel): a NaN rel is skipped -- as is a broken-down column, whose
                // reference counterpart is NaN from its breakdown on
                if (a.conv[j] != kConvBroken)
                    maxrel = maxrel < rel ? rel : maxrel;  // std::max: a NaN rel is skipped
                if (!a.conv[j] && rel < a.tol)
                    a.conv[j] = 1;
                nconv += a.conv[j] != 0;
            }
            if (a.hist && iter < a.hist_cap)
                a.hist[iter] = maxrel;
            if (nconv == L) {
                a.ctrl->done = 1;
                a.ctrl->iters_out = iter + 1;
            } else if (!a.pcg) {  // PCG: beta and rs_old follow Z = M R (k_fold_dot kFoldPcgBeta)
                for (int j = 0; j < L; ++j) {
                    CgScalars &s = a.scal[j];
                    s.beta = a.conv[j] ? 0.0 : s.rs_new / s.rs_old;
                    s.rs_old = s.rs_new;
                }
            }
            a.ctrl->iter = iter + 1;
        }
    }
}

// ---- row-sharded CG helpers ------------------------------------------------------------
// After the all-reduce of b.b: rs_old_j = b_j.b_j, b_norm_j = sqrt (or 1), fresh control.
template <int L>
__global__ void k_dist_init_finish(CgVecArgs a)
{
    const int j = threadIdx.x;
    if (j < L) {
        CgScalars &s = a.scal[j];
        const double bb = a.red_in[j];
        s.rs_old = bb;
        const double bn = sqrt(bb);
        s.b_norm = bn == 0.0 ? 1.0 : bn;
        s.alpha = s.beta = s.pAp = s.rs_new = 0.0;
        a.conv[j] = 0;
    }
    if (j == 0) {
        a.ctrl->iter = 0;
        a.ctrl->done = 0;
        a.ctrl->iters_out = 0;
        a.ctrl->breakdown = 0;
    }
}

// p_own = r + beta p_own  (update_p_multiple, utils_multiple.hpp:43-59; beta = 0 on the first
// iteration gives p = r = b, the reference's P = B).
template <int L>
__global__ __launch_bounds__(kBlock) void k_dist_pupdate(CgVecArgs a, double *p)
{
    if (a.ctrl->done)
        return;
    const long long stride = (long long)gridDim.x * kBlock;
    const long long i0 = (long long)blockIdx.x * kBlock + threadIdx.x;
    const bool lag = a.lazy_x && a.ctrl->x_pending;  // the previous update's x += alpha p (lazy_x)
    if (L == 1) {
        const double beta = a.scal[0].beta, alpha = a.scal[0].alpha;
        for (long long i = i0; i < a.n_elems; i += stride) {
            const double q = p[i];
            if (lag)
                a.x[i] = a.x[i] + alpha * q;
            p[i] = a.r[i] + beta * q;
        }
        return;
    }
    // column pairs: the stride (in pairs) is a multiple of L/2, so a thread keeps its pair
    constexpr int GL = L > 1 ? L / 2 : 1;
    const int cp = (int)(i0 % GL);
    const double2 beta = make_double2(a.scal[2 * cp].beta, a.scal[2 * cp + 1].beta);
    const double2 alpha = make_double2(a.scal[2 * cp].alpha, a.scal[2 * cp + 1].alpha);
    const long long npairs = a.n_elems / 2;
    if (lag) {
        for_pairs<GL>(npairs, a.rev, [&](long long i) {
            const v2d_t rv = __builtin_nontemporal_load(reinterpret_cast<const v2d_t *>(a.r) + i);
            const double2 r = make_double2(rv[0], rv[1]);
            double2 q = reinterpret_cast<double2 *>(p)[i];
            const v2d_t xo = __builtin_nontemporal_load(reinterpret_cast<const v2d_t *>(a.x) + i);
            __builtin_nontemporal_store(v2d_t{xo[0] + alpha.x * q.x, xo[1] + alpha.y * q.y},
                                        reinterpret_cast<v2d_t *>(a.x) + i);
            q.x = r.x + beta.x * q.x;
            q.y = r.y + beta.y * q.y;
            reinterpret_cast<double2 *>(p)[i] = q;
        });
        return;
    }
    for (long long i = i0; i < npairs; i += stride) {
        const double2 r = reinterpret_cast<const double2 *>(a.r)[i];
        double2 q = reinterpret_cast<double2 *>(p)[i];
        q.x = r.x + beta.x * q.x;
        q.y = r.y + beta.y * q.y;
        reinterpret_cast<double2 *>(p)[i] = q;
    }
}

// After the split CG's loop: the deferred x += alpha p of the last update, if no p update applied
// it (CgVecArgs::lazy_x).  p still holds that iteration's p: the p updates after the stop return at
// once, and a stop in the fold (every column converged or broken) follows a p update that applied
// the term and a fold that cleared the flag.
template <int L>
__global__ __launch_bounds__(kBlock) void k_cg_xflush(CgVecArgs a, const double *p)
{
    if (!a.ctrl->x_pending)
        return;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n_elems; i += stride)
        a.x[i] = a.x[i] + a.scal[L == 1 ? 0 : (int)(i % L)].alpha * p[i];
}

// R.Z per column and the PCG scalars after it (PCGSolveMultiple): mode 0 (init, :96-104)
// rs_old = R.Z; mode 1 (:171-185) beta = converged ? 0 : R.Z / rs_old, rs_old = R.Z.
// Mode 2 (split CG with a plain SpMM, cg_dot_pass): p.Ap per column into red_out, then the
// breakdown checks k_fold_dot makes in kFoldCgAlpha mode.
template <int L>
__global__ __launch_bounds__(kBlock) void k_pcg_dot(CgVecArgs a, int mode)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    __shared__ double2 s_red2[kBlock / 64][GL];
    __shared__ double s_colred[kBlock];
    __shared__ double s_out[L];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    if (a.ctrl->done)
        return;
    const long long npairs = a.n_elems / 2;
    const long long stride = (long long)gridDim.x * kBlock;
    const long long i0 = (long long)blockIdx.x * kBlock + tid;
    double2 acc = make_double2(0.0, 0.0);
    (void)stride;
    (void)i0;
    if (mode == 2) {  // split CG: a.r = p (next read by the p update, two passes on): nontemporal
        for_pairs<GL>(npairs, a.rev, [&](long long i) {
            const v2d_t r = __builtin_nontemporal_load(reinterpret_cast<const v2d_t *>(a.r) + i);
            const double2 z = reinterpret_cast<const double2 *>(a.p)[i];
            acc.x += r[0] * z.x;
            acc.y += r[1] * z.y;
        });
    } else {
        for_pairs<GL>(npairs, a.rev, [&](long long i) {
            const double2 r = reinterpret_cast<const double2 *>(a.r)[i];
            const double2 z = reinterpret_cast<const double2 *>(a.p)[i];
            acc.x += r.x * z.x;
            acc.y += r.y * z.y;
        });
    }
    if ((a.n_elems & 1) && blockIdx.x == 0 && tid == 0)
        acc.x += a.r[a.n_elems - 1] * a.p[a.n_elems - 1];
    colpair_block_reduce<L>(acc, s_red2, a.partials + (size_t)blockIdx.x * L);
    if (!reduce_slots<L>(a.partials, a.gtickets, blockIdx.x, gridDim.x, s_colred, s_out, &s_last, a.ctrl))
        return;
    if (mode == 2) {  // split CG: p.Ap (a.r = p, a.p = Ap) -> red_out, breakdown per column
        if (tid < L) {
            a.red_out[tid] = s_out[tid];
            cg_alpha_column(tid, s_out[tid], a.scal, a.conv, a.ctrl);
        }
        __syncthreads();
        cg_alpha_finish<L>(a.conv, a.ctrl);
        return;
    }
    if (tid < L) {
        CgScalars &s = a.scal[tid];
        const double d = s_out[tid];
        if (mode == 1)
            s.beta = a.conv[tid] ? 0.0 : d / s.rs_old;
        s.rs_old = d;
    }
}

// Pack the owned entries other ranks need: send[e] = p[idx[e / L] * L + e % L].
__global__ void k_dist_pack(const double *__restrict__ p, const int *__restrict__ idx, long long n_elems, int L,
                            double *__restrict__ send, const CgControl *ctrl)
{
    if (ctrl && ctrl->done)
        return;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_elems;
         e += (long long)gridDim.x * blockDim.x)
        send[e] = p[(size_t)idx[e / L] * L + e % L];
}

// One block, after the all-reduces of p.Ap (red_in) and r.r (red_out): breakdown test,
// convergence masks, max-residual history, beta, rs_old (no_pretreatment.hpp:109-182).
template <int L>
__global__ void k_dist_finish(CgVecArgs a)
{
    if (threadIdx.x != 0 || a.ctrl->done)
        return;
    const int iter = a.ctrl->iter;
    // The update (k_cg_update with red_in) already applied alpha = 0 to broken columns: their
    // x and r stay as they were; here they are marked and frozen (k_fold_dot's rule, per column).
    for (int j = 0; j < L; ++j) {
        if (a.conv[j])
            continue;
        const double alpha = a.scal[j].rs_old / a.red_in[j];
        if (!(alpha == alpha && fabs(alpha) < HUGE_VAL)) {
            a.ctrl->breakdown = 1;
            a.conv[j] = kConvBroken;
        }
    }
    int nconv = 0;
    double maxrel = 0.0;
    for (int j = 0; j < L; ++j) {
        CgScalars &s = a.scal[j];
        const double rs_new = a.red_out[j];
        s.rs_new = rs_new;
        const double rel = sqrt(rs_new) / s.b_norm;
        if (a.conv[j] != kConvBroken)
            maxrel = maxrel < rel ? rel : maxrel;  // std::max: a NaN rel is skipped
        if (!a.conv[j] && rel < a.tol)
            a.conv[j] = 1;
        nconv += a.conv[j] != 0;
    }
    if (a.hist && iter < a.hist_cap)
        a.hist[iter] = maxrel;
    if (nconv == L) {
        a.ctrl->done = 1;
        a.ctrl->iters_out = iter + 1;
    } else {
        for (int j = 0; j < L; ++j) {
            CgScalars &s = a.scal[j];
            s.beta = a.conv[j] ? 0.0 : s.rs_new / s.rs_old;
            s.rs_old = s.rs_new;
        }
    }
    a.ctrl->iter = iter + 1;
}

// Workgroups of the CG's streaming passes: ~12 pairs per thread, at most three per CU -- fewer,
// longer-lived workgroups stream faster here: configs[4] (nlpkkt120 size, L = 8) 0.915 -> 0.886 ms
// per iteration against the old 2,048 (~4 pairs per thread); 4 and 2 per CU 0.895 / 0.893 (r04ae,
// r04af).
int cg_update_blocks(long long elems, int /*num_cus*/)
{
    // ~12 pairs per thread on long vectors, capped at 768 workgroups (3 per CU of the whole chip).  Below that
    // (a single-RHS vector of a few hundred thousand rows: 70 workgroups at 12 pairs) one pair per thread up to
    // the cap instead: the passes are latency bound on a quarter of the CUs otherwise -- 15.4 us per pass on
    // the 427,500-row CG (r06e trace).  The grid -- and so every partial sum's order -- does not depend on the
    // handle's CU limit: a CU mask changes the speed of a solve, never its iterates (tests/test_parallel_
    // efficiency.py; round 5's cap of 3 per *available* CU made it depend on them).
    constexpr long long cap = 768;
    const long long pairs = (elems + 1) / 2;
    long long b = std::max((pairs + kBlock * 12 - 1) / (kBlock * 12), std::min((pairs + kBlock - 1) / kBlock, cap));
    if (b < 1)
        b = 1;
    if (b > cap)
        b = cap;
    return (int)b;
}

// Iterations per CG batch (one graph replay).  The host inspects batch b's control word while
// b + 1 runs, so a solve launches up to 2K - 1 iterations past its convergence (each returning
// early, but a multi-RHS SpMM still streams part of its tile before its stop test).  K = 32 wasted
// 48 of 96 launched iterations on the nlpkkt120-size 8-RHS solve (584 us each): size K so a batch
// lasts ~300 us at ~5 TB/s of the SURVEY 8(d) iteration bytes -- long enough to hide the host's
// check, short enough to bound the overshoot.  Even (the p buffers alternate by parity), 2..32.
// MSPMV_CG_BATCH overrides (lab).
int cg_batch_iters(long long m, long long nnz, int L)
{
    static const int forced = [] {
        const char *e = getenv("MSPMV_CG_BATCH");
        return e ? atoi(e) : 0;
    }();
    int k = forced;
    if (k <= 0) {
        const double est_us = (12.0 * (double)nnz + 88.0 * (double)m * L) / 5.0e6;
        k = (int)std::ceil(300.0 / std::max(est_us, 1.0));
    }
    k = (k + 1) & ~1;
    return std::min(32, std::max(2, k));
}

// The handle-derived fields of a CgVecArgs: the solve's vectors (p = p0 = the handle's p buffer), scalars,
// control word, partials, tickets and history.  What the passes branch on -- red_in, red_out, pcg, lazy_x,
// rev -- stays 0 for the caller to set.  Every single-GPU launcher below starts from it, so some passes are
// handed fields they never read:
//   k_cg_init (launch_cg_init) reads none of ap, hist, hist_cap, tol, and takes p = b from its caller;
//   k_cg_xflush (launch_cg_xflush) reads n_elems, x, scal and ctrl only;
//   p0 is read by k_cg_init alone (the split iteration's passes get it and ignore it).
// hist, which the updates test, is the handle's in every launcher that runs one (null without a history).
static CgVecArgs cg_vec_args(mspmv_handle_s *h, double *d_x, int L, double tol)
{
    CgVecArgs va{};
    va.n_elems = (long long)h->m * L;
    va.x = d_x;
    va.r = h->d_r;
    va.p = h->d_p0;
    va.p0 = h->d_p0;
    va.ap = h->d_ap;
    va.scal = h->d_scal;
    va.ctrl = h->d_ctrl;
    va.conv = h->d_conv;
    va.partials = h->d_partials;
    va.gtickets = h->d_gtickets;
    va.hist = h->d_hist;
    va.hist_cap = h->hist_cap;
    va.tol = tol;
    return va;
}

hipError_t launch_cg_init(mspmv_handle_s *h, const double *d_b, double *d_x, int L, double tol, int nblk, bool warm)
{
    CgVecArgs a = cg_vec_args(h, d_x, L, tol);
    a.p = warm ? h->d_r : d_b;
    a.bb_in = warm ? h->d_warm : nullptr;
    return launch_dist_vec(warm ? CgVecPass::InitWarm : CgVecPass::InitPartials, a, L, nblk, nullptr, h->stream);
}

// ---- pipelined single-RHS CG (consumer-side reductions, no ticket chains) -------------------
// Iteration k = [k_spmv_tile MODE 1: stop test + beta from the r.r partials, p = r + beta p_old
// gathered, Ap, p.Ap partials] -> [k_cg1_update: alpha from the p.Ap partials, x, r, r.r
// partials].  Each kernel sums its producer's partials itself (part_load / part_sum), so no
// kernel ends on a chain of tickets and folds.
struct Cg1Args {
    long long m;
    double *x;
    double *rp;            // init: {r, p_0} = {b, b}.  update: {r_k, p_{k-1}} (r_k read at rp[2 i])
    double *rp_next;       // update: {., p_k} -> {r_{k+1}, p_k} (p_k read, r_{k+1} written)
    const double *b;       // init
    const double *ap;
    CgScalars *scal;
    CgControl *ctrl;
    const double *part_in;  // producer partials (update: the SpMV's p.Ap; finish: the update's r.r)
    int n_part_in;
    double *part_out;       // this kernel's per-block partials (r.r, or b.b at init)
    int parity;
    double *hist;
    int hist_cap;
};

// x = 0, {r, p_0} = {b, b} (interleaved, see cg_rp), and this block's b.b partial (the first
// SpMV sums them: rs_0, ||b||).
__global__ __launch_bounds__(kBlock) void k_cg1_init(Cg1Args a)
{
    __shared__ double s_red[kBlock / 64];
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.m; i += (long long)gridDim.x * kBlock) {
        const double b = a.b[i];
        a.x[i] = 0.0;
        reinterpret_cast<double2 *>(a.rp)[i] = make_double2(b, b);
        acc += b * b;
    }
    const double t = block_sum(acc, s_red);
    if (threadIdx.x == 0)
        a.part_out[blockIdx.x] = t;
}

// Tail of iteration k (single_strategy.hpp:140-148): alpha = rs_k / p.Ap (every block sums the
// SpMV's partials in the same order), r += (-alpha) Ap, r.r partial per block; x += alpha p is
// deferred to the next SpMV (cg1_lag_*), which takes alpha from scal[0].alpha.  A non-finite
// alpha stops the solve before r changes (the reference keeps going on NaN).
__global__ __launch_bounds__(kBlock) void k_cg1_update(Cg1Args a)
{
    __shared__ double s_red[kBlock / 64];
    const int tid = threadIdx.x;
    if (a.ctrl->done)
        return;
    PartRegs<kConsumeTile / kBlock> pin;
    part_load(a.part_in, a.n_part_in, pin);
    const long long stride = (long long)gridDim.x * kBlock;
    const long long i0 = (long long)blockIdx.x * kBlock + tid;
    double q = 0.0, r = 0.0;  // the first element's operands, in flight under the sum
    if (i0 < a.m) {
        q = a.ap[i0];
        r = a.rp[2 * i0];
    }
    const double pAp = part_sum(pin, s_red);
    const double alpha = a.scal[0].rs_par[a.parity] / pAp;
    if (!(alpha == alpha && fabs(alpha) < HUGE_VAL)) {
        if (blockIdx.x == 0 && tid == 0) {
            a.ctrl->breakdown = 1;
            a.ctrl->iters_out = a.ctrl->iter_par[a.parity] + 1;
            a.ctrl->done = 1;
        }
        return;
    }
    if (blockIdx.x == 0 && tid == 0)
        a.scal[0].alpha = alpha;  // x += alpha p_k: the next SpMV's rows, or k_cg1_xflush
    const double nal = -alpha;
    double acc = 0.0;
    for (long long i = i0; i < a.m; i += stride) {
        if (i != i0) {
            q = a.ap[i];
            r = a.rp[2 * i];
        }
        r = r + nal * q;
        a.rp_next[2 * i] = r;
        acc += r * r;
    }
    const double t = block_sum(acc, s_red);
    if (tid == 0)
        a.part_out[blockIdx.x] = t;
}

// After max_iters iterations: the last iteration's stop test and history entry (the SpMV that
// would take it is not launched); iterations = max_iters either way (single_strategy.hpp:152-170).
__global__ __launch_bounds__(kBlock) void k_cg1_finish(Cg1Args a)
{
    __shared__ double s_red[kBlock / 64];
    if (a.ctrl->done)
        return;
    PartRegs<kUpdateMaxBlocks / kBlock> pin;
    part_load(a.part_in, a.n_part_in, pin);
    const double rs = part_sum(pin, s_red);
    if (threadIdx.x == 0) {
        CgControl *c = a.ctrl;
        const int k = c->iter_par[a.parity];
        if (a.hist && k >= 1 && k - 1 < a.hist_cap)
            a.hist[k - 1] = sqrt(rs) / a.scal[0].b_norm;
        c->iter = k;
        c->iters_out = k;
        c->done = 1;
    }
}

// After the loop (converged, max_iters or breakdown): the last deferred x += alpha p.  The solve
// reported j + 1 = iters_out iterations; the update of iteration j ran (it stored alpha_j) and no
// SpMV after it applied its term (the stop test that ended the solve returns before that, and
// max_iters launches none).  p_j was written into the {r, p} buffer of parity (j + 1) & 1.  A
// breakdown (non-finite alpha_j) leaves nothing pending: the update stopped before storing alpha_j
// and iteration j's SpMV had applied alpha_{j-1} p_{j-1} already.
__global__ __launch_bounds__(kBlock) void k_cg1_xflush(Cg1Args a)
{
    const CgControl *c = a.ctrl;
    if (c->breakdown || c->iters_out < 1)
        return;
    const int j = c->iters_out - 1;
    const double *rp = ((j + 1) & 1) ? a.rp_next : a.rp;  // rp: d_p0, rp_next: d_p1
    const double alpha = a.scal[0].alpha;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.m; i += (long long)gridDim.x * kBlock)
        a.x[i] = a.x[i] + alpha * rp[2 * i + 1];
}

int cg1_blocks(long long m)
{
    // one element per thread up to kUpdateMaxBlocks (512 / 256 update blocks measured no faster, r02u)
    const long long b = (m + kBlock - 1) / kBlock;
    return (int)std::max<long long>(1, std::min<long long>(b, kUpdateMaxBlocks));
}

static Cg1Args cg1_args(mspmv_handle_s *h, double *d_x)
{
    Cg1Args a{};
    a.m = h->m;
    a.x = d_x;
    a.rp = h->d_p0;  // {r, p} of parity 0; the iterations alternate d_p0 / d_p1 (2 m doubles each)
    a.ap = h->d_ap;
    a.scal = h->d_scal;
    a.ctrl = h->d_ctrl;
    a.hist = h->d_hist;
    a.hist_cap = h->hist_cap;
    return a;
}

hipError_t launch_cg1_init(mspmv_handle_s *h, const double *d_b, double *d_x, int nblk)
{
    Cg1Args a = cg1_args(h, d_x);
    a.b = d_b;
    a.part_out = h->d_partials_b;
    hipLaunchKernelGGL(k_cg1_init, dim3(nblk), dim3(kBlock), 0, h->stream, a);
    return hipGetLastError();
}

hipError_t launch_cg1_finish(mspmv_handle_s *h, double *d_x, int parity, int nblk)
{
    Cg1Args a = cg1_args(h, nullptr);
    a.part_in = h->d_partials_b;
    a.n_part_in = nblk;
    a.parity = parity;
    hipLaunchKernelGGL(k_cg1_finish, dim3(1), dim3(kBlock), 0, h->stream, a);
    if (hipGetLastError() != hipSuccess)
        return hipErrorLaunchFailure;
    a.x = d_x;
    a.rp = h->d_p0;
    a.rp_next = h->d_p1;
    hipLaunchKernelGGL(k_cg1_xflush, dim3(nblk), dim3(kBlock), 0, h->stream, a);
    return hipGetLastError();
}


// k_pcg_dot (mode 0 / 1: R.Z of the IC(0) PCG; 2: the split CG's p.Ap pass)
static hipError_t pcg_dot(const CgVecArgs &va, int L, int nblk, int mode, hipStream_t s)
{
    return dispatch_L(L, [&](auto Lc) {
        hipLaunchKernelGGL((k_pcg_dot<decltype(Lc)::value>), dim3(nblk), dim3(kBlock), 0, s, va, mode);
        return hipGetLastError();
    });
}

// Multi-RHS iteration, split: p = r + beta p (one streaming pass), then Y = A p with p.Ap by
// linearity (MODE 2, which also stops on a non-finite alpha), then the update with alpha from
// that p.Ap.  For L >= 2 the fused iteration would gather two L-wide panel rows (r and
// p_old) per nonzero, and the SpMM is gather-bound: measured 1.33 ms vs 0.62 + 0.14 ms split
// on the nlpkkt120-sized L = 8 case.

// Split CG: p.Ap from the SpMM's dot mode (x.(Ax) partials per tile) or from a separate pass over
// p and Ap after the plain SpMM (MSPMV_CG_DOT=pass / fused; default: the pass).
static bool cg_dot_pass(int L)
{
    static const int mode = [] {
        const char *e = getenv("MSPMV_CG_DOT");
        return e && std::string(e) == "fused" ? 0 : 1;
    }();
    return mode != 0 && L >= 1;
}

// The block CG's SpMM on the offset windows takes p.Ap in its dot mode (MSPMV_DIA_DOT=0: the plain window
// SpMM and the separate pass, as the tiles do).
bool dia_dot_fused()
{
    const char *e = getenv("MSPMV_DIA_DOT");
    return !(e && *e && atoi(e) == 0);
}

// Y = A X inside a solver's iteration: the plain L-wide product on the plan the solve chose for it (splan: the
// handle's offset-window or column-slab plan, else null -> the merge tiles of `plan`), with the control word,
// so the launch returns at once when the solve has stopped.  The split CG and BiCGSTAB launch it.
static const TilePlan &solver_product_plan(const TilePlan &p, const TilePlan *sp) { return sp ? *sp : p; }

hipError_t launch_solver_product(mspmv_handle_s *h, const TilePlan &plan, const TilePlan *splan, const double *d_X,
                                 double *d_Y, int L)
{
    return launch_spmm_tile_only(h, solver_product_plan(plan, splan), d_X, d_Y, L, L, h->d_ctrl);
}

std::string solver_product_name(const mspmv_handle_s *h, const TilePlan &plan, const TilePlan *splan, int L)
{
    return product_kernel_name(h, solver_product_plan(plan, splan), L);
}

// splan: the plan the solve chose for the plain L-wide product (cg_solve_native: the offset-window or
// column-slab plan, else null -> the tiles of `plan`); dot_fused: the window SpMM takes p.Ap in its dot
// mode (resolved once per solve, and part of the CG graph's key).
// The p update stays its own pass: fused into the window SpMM (the spans staged as r + beta p_old, the
// window's own rows written to a second p buffer) it measured 0.773-0.779 against 0.657-0.658 ms per
// configs[4] iteration (r06c): the SpMM then loads r's spans beside p's -- nine times per row through L2
// -- which costs the issue-bound kernel more than the pass it replaces.
static hipError_t launch_cg_iteration_split(mspmv_handle_s *h, const TilePlan &plan, const TilePlan *splan,
                                            bool dot_fused, double *d_x, int L, int nblk, double tol)
{
    CgVecArgs va = cg_vec_args(h, d_x, L, tol);
    va.lazy_x = 1;
    static const int rev = [] {  // measured knob: alternate sweep directions (CgVecArgs::rev)
        const char *e = getenv("MSPMV_CG_REV");
        return e ? atoi(e) : 1;
    }();
    va.rev = rev;  // the p update (after the forward update) sweeps backwards
    hipError_t e = launch_dist_vec(CgVecPass::PUpdate, va, L, nblk, h->d_p0, h->stream);
    va.rev = 0;
    if (e != hipSuccess)
        return e;
    const TilePlan *dp = splan && splan->dia ? splan : nullptr;
    if (dp && dot_fused) {
        // offset windows (mspmv_dia.hip) in dot mode: Ap and one p.Ap partial per window, folded with the
        // non-finite-alpha stop -- no separate pass over p and Ap
        if ((e = launch_dia(h, *dp, h->d_p0, h->d_ap, L, L, h->d_ctrl, h->d_partials)) != hipSuccess)
            return e;
        if ((e = launch_fold_dot(dp->num_tiles, L, h->d_partials, h->d_gtickets, h->d_red, h->d_scal, h->d_conv,
                                 h->d_ctrl, -1, h->stream)) != hipSuccess)
            return e;
    } else if (cg_dot_pass(L)) {
        // the plain SpMM (its tile kernel holds fewer registers than the dot mode's, so more
        // workgroups per CU, and never spills), stopped by the control word, then p.Ap in one
        // streaming pass over p and Ap with the fold's breakdown checks (k_pcg_dot mode 2)
        // (on the offset-window or column-slab plan when the handle's plain L-wide product took one)
        if ((e = launch_solver_product(h, plan, splan, h->d_p0, h->d_ap, L)) != hipSuccess)
            return e;
        CgVecArgs vd = va;
        vd.r = h->d_p0;
        vd.p = h->d_ap;
        vd.red_out = h->d_red;
        vd.rev = rev;  // ... the p.Ap pass backwards, so the update finds Ap's first lines cached
        if ((e = pcg_dot(vd, L, nblk, 2, h->stream)) != hipSuccess)
            return e;
    } else if ((e = launch_spmm_dot(h, plan, h->d_p0, h->d_ap, L, h->d_ctrl, h->d_partials, h->d_gtickets, h->d_red,
                                    h->d_scal, h->d_conv)) != hipSuccess) {
        return e;
    }
    va.red_in = h->d_red;
    return launch_dist_vec(CgVecPass::XrUpdate, va, L, nblk, nullptr, h->stream);
}

// After the split iteration's loop: the x += alpha p still pending (CgVecArgs::lazy_x).
hipError_t launch_cg_xflush(mspmv_handle_s *h, double *d_x, int L, int nblk)
{
    const CgVecArgs va = cg_vec_args(h, d_x, L, 0.0);
    return dispatch_L(L, [&](auto Lc) {
        hipLaunchKernelGGL((k_cg_xflush<decltype(Lc)::value>), dim3(nblk), dim3(kBlock), 0, h->stream, va, h->d_p0);
        return hipGetLastError();
    });
}

// Multi-RHS CG always runs the split iteration; single-RHS the pipelined one unless
// MSPMV_CG_SPLIT=1 asks for the split form (A/B runs, and its own parity test).
bool cg_split_iteration(int L)
{
    static const int mode = [] {
        const char *e = getenv("MSPMV_CG_SPLIT");
        return e ? atoi(e) : 0;
    }();
    return L >= 2 || mode != 0;
}

hipError_t launch_cg_iteration(mspmv_handle_s *h, const TilePlan &plan, const TilePlan *splan, bool dot_fused,
                               double *d_x, int L, int parity, int nblk, double tol, bool split)
{
    if (split)
        return launch_cg_iteration_split(h, plan, splan, dot_fused, d_x, L, nblk, tol);
    double *rp_old = parity ? h->d_p1 : h->d_p0;  // {r_k, p_{k-1}} interleaved (cg_rp)
    double *rp_new = parity ? h->d_p0 : h->d_p1;  // receives p_k, then r_{k+1}
    int nslots = plan.num_tiles;                   // the SpMV's p.Ap partials
    hipError_t e = hipSuccess;
    if (splan && splan->dia)  // the SpMV on the offset windows (mspmv_dia.hip, k_cg1_dia)
        e = launch_cg1_dia(h, *splan, rp_old, rp_new, d_x, parity, nblk, tol, &nslots);
    else  // ... or on the merge-path tiles (mspmv_kernels.hip, k_spmv_tile MODE 1)
        e = launch_cg1_tile(h, plan, rp_old, rp_new, d_x, parity, nblk, tol, &nslots);
    if (e != hipSuccess)
        return e;
    Cg1Args a = cg1_args(h, d_x);
    a.rp = rp_old;
    a.rp_next = rp_new;
    long long off = 0;
    int count = 0;
    consumer_level(nslots, kConsumeTile, 1, &off, &count);
    a.part_in = h->d_partials + off;
    a.n_part_in = count;
    a.part_out = h->d_partials_b;
    a.parity = parity;
    hipLaunchKernelGGL(k_cg1_update, dim3(nblk), dim3(kBlock), 0, h->stream, a);
    return hipGetLastError();
}

// ---- row-sharded CG launchers --------------------------------------------------------------
template <int L>
static hipError_t dist_launch_L(CgVecPass pass, const CgVecArgs &a, int nblk, double *p, hipStream_t s)
{
    switch (pass) {
    case CgVecPass::InitPartials: hipLaunchKernelGGL((k_cg_init<L>), dim3(nblk), dim3(kBlock), 0, s, a); break;
    case CgVecPass::InitWarm: hipLaunchKernelGGL((k_cg_init<L, true>), dim3(nblk), dim3(kBlock), 0, s, a); break;
    case CgVecPass::InitFinish: hipLaunchKernelGGL((k_dist_init_finish<L>), dim3(1), dim3(64), 0, s, a); break;
    case CgVecPass::PUpdate: hipLaunchKernelGGL((k_dist_pupdate<L>), dim3(nblk), dim3(kBlock), 0, s, a, p); break;
    case CgVecPass::XrUpdate: hipLaunchKernelGGL((k_cg_update<L>), dim3(nblk), dim3(kBlock), 0, s, a); break;
    case CgVecPass::Finish: hipLaunchKernelGGL((k_dist_finish<L>), dim3(1), dim3(64), 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The single-GPU iterations run the same passes: InitPartials and XrUpdate with red_out null finish the
// scalars in their last block, so InitFinish and Finish are the row-sharded CG's alone.
hipError_t launch_dist_vec(CgVecPass pass, const CgVecArgs &a, int L, int nblk, double *p, hipStream_t s)
{
    return dispatch_L(L, [&](auto Lc) { return dist_launch_L<decltype(Lc)::value>(pass, a, nblk, p, s); });
}

hipError_t launch_dist_pack(const double *p, const int *idx, long long n_elems, int L, double *send,
                            const CgControl *ctrl, hipStream_t s)
{
    if (n_elems <= 0)
        return hipSuccess;
    const long long nb = std::min<long long>((n_elems + 255) / 256, 4096);
    hipLaunchKernelGGL(k_dist_pack, dim3((unsigned)nb), dim3(256), 0, s, p, idx, n_elems, L, send, ctrl);
    return hipGetLastError();
}

// Sum T tiles' partials [T][L] in tile order into dot_out (k_fold_dot; partials_capacity() leaves
// room for the fold's levels after the T * L partials).
hipError_t launch_fold_dot(int T, int L, double *partials, unsigned *gtickets, double *dot_out, CgScalars *scal,
                           const unsigned char *conv, CgControl *ctrl, int fold_mode, hipStream_t s)
{
    const int mode = fold_mode >= 0 ? fold_mode : scal ? kFoldCgAlpha : kFoldDot;
    if (T == 0)  // no rows: contributes 0 (a rank's share of the all-reduce)
        return hipMemsetAsync(dot_out, 0, sizeof(double) * L, s);
    const int G = std::max(1, std::min(256, (T + 63) / 64));  // >= 64 tiles per fold block
    const int q = (T + G - 1) / G;
    double *lvl = partials + (size_t)T * L;
    return dispatch_L(L, [&](auto Lc) {
        hipLaunchKernelGGL((k_fold_dot<decltype(Lc)::value>), dim3(G), dim3(kBlock), 0, s, partials, T, q, lvl,
                           gtickets, dot_out, scal, conv, ctrl, mode);
        return hipGetLastError();
    });
}

// Y = A X with x.(AX) per column reduced into dot_out (the tiles' MODE 2, then the partials' fold).
// scal / conv (single-GPU split CG) add the non-finite-alpha stop.
hipError_t launch_spmm_dot(mspmv_handle_s *h, const TilePlan &plan, const double *d_X, double *d_Y, int L,
                           CgControl *ctrl, double *partials, unsigned *gtickets, double *dot_out,
                           CgScalars *scal, const unsigned char *conv, int fold_mode)
{
    hipError_t e = launch_spmm_dot_tiles(h, plan, d_X, d_Y, L, ctrl, partials, h->stream, 0);
    if (e != hipSuccess)
        return e;
    return launch_fold_dot(plan.num_tiles, L, partials, gtickets, dot_out, scal, conv, ctrl, fold_mode, h->stream);
}

// ---- SPAI-preconditioned block CG (SPAISolveMultiple) ------------------------------------------
static CgVecArgs pcg_vec_args(mspmv_handle_s *h, double *d_x, int L, double tol)
{
    CgVecArgs va = cg_vec_args(h, d_x, L, tol);
    va.pcg = 1;
    return va;
}

// X = 0, R = B, b_norms (sparse_approximate_inverse.hpp:59-78); Z = M R and rs_old = R.Z
// (:80-92, :99-100); P = Z (:94-97).  Z lives in h->d_p1, P in h->d_p0.
hipError_t launch_pcg_init(mspmv_handle_s *h, mspmv_handle_s *hm, const TilePlan &mplan, const double *d_b,
                           double *d_x, int L, double tol, int nblk, bool warm)
{
    hipError_t e = launch_cg_init(h, d_b, d_x, L, tol, nblk, warm);
    if (e != hipSuccess)
        return e;
    hipStream_t own = hm->stream;
    hm->stream = h->stream;
    e = launch_spmm_dot(hm, mplan, h->d_r, h->d_p1, L, h->d_ctrl, h->d_partials, h->d_gtickets, h->d_red,
                        h->d_scal, h->d_conv, kFoldPcgInit);
    hm->stream = own;
    if (e != hipSuccess)
        return e;
    return hipMemcpyAsync(h->d_p0, h->d_p1, sizeof(double) * (size_t)h->m * L, hipMemcpyDeviceToDevice, h->stream);
}

// One PCG iteration, four launches plus two folds: AP = A P with P.AP -> alpha (:111-138);
// X += alpha P, R -= alpha AP, R.R -> masks, max-residual history, stop (:140-181);
// Z = M R with R.Z -> beta, rs_old (:183-210); P = Z + beta P (:212-214).
hipError_t launch_pcg_iteration(mspmv_handle_s *h, mspmv_handle_s *hm, const TilePlan &plan, const TilePlan &mplan,
                                double *d_x, int L, int nblk, double tol)
{
    CgVecArgs va = pcg_vec_args(h, d_x, L, tol);
    hipError_t e = launch_spmm_dot(h, plan, h->d_p0, h->d_ap, L, h->d_ctrl, h->d_partials, h->d_gtickets, h->d_red,
                                   h->d_scal, h->d_conv, kFoldPcgAlpha);
    if (e != hipSuccess)
        return e;
    if ((e = launch_dist_vec(CgVecPass::XrUpdate, va, L, nblk, nullptr, h->stream)) != hipSuccess)
        return e;
    hipStream_t own = hm->stream;
    hm->stream = h->stream;
    e = launch_spmm_dot(hm, mplan, h->d_r, h->d_p1, L, h->d_ctrl, h->d_partials, h->d_gtickets, h->d_red,
                        h->d_scal, h->d_conv, kFoldPcgBeta);
    hm->stream = own;
    if (e != hipSuccess)
        return e;
    va.r = h->d_p1;  // P = Z + beta P
    return launch_dist_vec(CgVecPass::PUpdate, va, L, nblk, h->d_p0, h->stream);
}
// ---- IC(0)-preconditioned block CG (PCGSolveMultiple) -------------------------------------------
// Z = M^-1 R is tri_apply (mspmv_tri.hip): L^-T (L^-1 R), ForwardSolveMultiple then BackwardSolveMultiple
// (incomplete_cholesky.hpp:89-92, :166-167), through ic->d_y.
// X = 0, R = B, b_norms (incomplete_cholesky.hpp:66-85); Z = M^-1 R (:87-92); P = Z (:94-95);
// rs_old = R.Z (:97).  Z lives in h->d_p1, P in h->d_p0.
hipError_t launch_pcg_ic0_init(mspmv_handle_s *h, mspmv_ic0_s *ic, const double *d_b, double *d_x, int L, double tol,
                               int nblk, bool warm)
{
    hipError_t e = launch_cg_init(h, d_b, d_x, L, tol, nblk, warm);
    if (e == hipSuccess)
        e = tri_apply(ic, h->d_r, h->d_p1, L, h->d_ctrl, h->stream);
    CgVecArgs va = pcg_vec_args(h, d_x, L, tol);
    va.p = h->d_p1;
    if (e == hipSuccess)
        e = pcg_dot(va, L, nblk, 0, h->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(h->d_p0, h->d_p1, sizeof(double) * (size_t)h->m * L, hipMemcpyDeviceToDevice, h->stream);
    return e;
}

// One iteration (:104-191): AP = A P with P.AP (fold: alpha = rs_old / P.AP, non-finite stops);
// X += alpha P, R -= alpha AP, R.R -> masks, history, stop; Z = M^-1 R; R.Z -> beta, rs_old;
// P = Z + beta P.
hipError_t launch_pcg_ic0_iteration(mspmv_handle_s *h, mspmv_ic0_s *ic, const TilePlan &plan, double *d_x, int L,
                                    int nblk, double tol)
{
    hipError_t e = launch_spmm_dot(h, plan, h->d_p0, h->d_ap, L, h->d_ctrl, h->d_partials, h->d_gtickets, h->d_red,
                                   h->d_scal, h->d_conv, kFoldCgAlpha);
    CgVecArgs va = pcg_vec_args(h, d_x, L, tol);
    va.red_in = h->d_red;  // alpha_j = converged ? 0 : rs_old_j / P.AP_j, in every block
    if (e == hipSuccess)
        e = launch_dist_vec(CgVecPass::XrUpdate, va, L, nblk, nullptr, h->stream);
    if (e == hipSuccess)
        e = tri_apply(ic, h->d_r, h->d_p1, L, h->d_ctrl, h->stream);
    CgVecArgs vd = va;
    vd.p = h->d_p1;
    if (e == hipSuccess)
        e = pcg_dot(vd, L, nblk, 1, h->stream);
    va.r = h->d_p1;  // P = Z + beta P
    if (e == hipSuccess)
        e = launch_dist_vec(CgVecPass::PUpdate, va, L, nblk, h->d_p0, h->stream);
    return e;
}


}  // namespace mspmv

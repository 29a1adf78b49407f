// mspmv_bicgstab.hip -- multi-RHS BiCGSTAB for nonsymmetric systems: the streaming vector passes of one
// iteration and their launcher.  Per column j of a row-major n x L panel (van der Vorst's recurrence,
// unpreconditioned, rhat = b):
//     V = A P;  alpha = rho / (rhat.V);  s = R - alpha V (in R's storage);  X += alpha P
//     T = A s;  omega = (T.s) / (T.T)  (T.T == 0: omega = 0, s is exactly 0);  X += omega s;  R = s - omega T
//     rho' = rhat.R;  stop test on sqrt(R.R) / ||b||;  beta = (rho' / rho)(alpha / omega);  P = R + beta (P - omega V)
// An iteration is two products (launch_solver_product: the plan the handle's plain L-wide product runs) and five
// streaming passes; the four dot products close in three folds -- rhat.V alone, then (T.T, T.s) and (R.R, rhat.R)
// as folds of 2 L values each (two L-wide partial rows per block under one round of tickets).  The folds, the
// column-pair accesses and the grids (cg_update_blocks: independent of a CU mask) are the split CG's
// (mspmv_device.h).  Breakdown is per column, as in the split CG: a non-finite alpha, omega or beta freezes the
// column (kConvBroken: alpha = omega = beta = 0 from then on, X and R keep their last finite values, left out
// of the history) and the other columns keep iterating.
// Right-preconditioned with an ILU(0) factor M = L U (mspmv_dpbicgstab_ilu0_multi; launch_pbicgstab_iteration):
//     Phat = U^-1 L^-1 P;  V = A Phat;  ...  X += alpha Phat;  Shat = U^-1 L^-1 s;  T = A Shat;  ...  X += omega Shat
// and everything else as above: R is the original system's residual, so the stop test and the history mean the
// same.  Two applies of the factor per iteration (tri_apply, mspmv_tri.hip: L into the factor's intermediate, U
// into the factor's hat panel, which Phat and then Shat share), and the s and update passes in their PRE
// instantiation, which take X's direction from the hat panel; the other three passes are shared.
// Compiled with -ffp-contract=off like every kernel here: every a*b+c is two roundings.
#include "mspmv_internal.h"
#include "mspmv_device.h"

#include <cmath>

namespace mspmv {

struct BicgArgs {
    long long n_elems;  // n * L
    double *x;
    double *r;          // the residual; between the s pass and the update pass it holds s
    double *rhat;       // the shadow residual: b, fixed
    double *p;
    double *v;          // A p
    double *t;          // A s
    const double *hat;  // preconditioned only: Phat in the s pass, Shat in the update pass
    const double *b;    // init only
    const double *bb_in;  // warm init only: [L] B_j.B_j (k_warm_residual)
    CgScalars *scal;
    CgControl *ctrl;
    unsigned char *conv;
    double *partials;   // [blocks][2 L] and the fold's levels
    unsigned *gtickets;
    double *red;        // [L] rhat.V of the running iteration
    double *hist;
    int hist_cap;
    double tol;
};

__device__ __forceinline__ bool bicg_finite(double a) { return a == a && fabs(a) < HUGE_VAL; }

// A column froze: MSPMV_ERR_BREAKDOWN, unless a triangular-solve stall (2: MSPMV_ERR_STALL) is on record.
__device__ __forceinline__ void bicg_note_freeze(CgControl *ctrl)
{
    if (ctrl->breakdown != 2)
        ctrl->breakdown = 1;
}

// {f(j), f(j + 1)} for the column pair (j, j + 1) this thread meets in every chunk of a pass (for_pairs); L == 1:
// f(0) twice, the pair being two rows of the one column.
template <int L, typename F>
__device__ __forceinline__ double2 bicg_col_pair(F &&f)
{
    if (L == 1) {
        const double a = f(0);
        return make_double2(a, a);
    }
    constexpr int GL = L > 1 ? L / 2 : 1;
    const int j = 2 * (int)(((long long)blockIdx.x * kBlock + threadIdx.x) % GL);
    return make_double2(f(j), f(j + 1));
}

// After a fold's last block froze some column (ctrl->breakdown): no live column left stops the solve here.  The
// iteration changed nothing (every alpha, omega is 0); its history entry is the converged columns' residual.
template <int L>
__device__ __forceinline__ void bicg_stop_if_none_live(const BicgArgs &a)
{
    if (threadIdx.x != 0 || !a.ctrl->breakdown)
        return;
    int live = 0;
    double maxrel = 0.0;
    for (int j = 0; j < L; ++j) {
        live += a.conv[j] == 0;
        if (a.conv[j] == 1) {
            const double rel = sqrt(a.scal[j].rs_new) / a.scal[j].b_norm;
            maxrel = maxrel < rel ? rel : maxrel;
        }
    }
    if (live)
        return;
    const int iter = a.ctrl->iter;
    if (a.hist && iter < a.hist_cap)
        a.hist[iter] = maxrel;
    a.ctrl->done = 1;
    a.ctrl->iters_out = iter + 1;
}

// The two L-wide sums of a pass as one fold of 2 L values: this block's partial row is {acc0's columns, acc1's
// columns}, and one round of tickets (reduce_slots at width 2 L) closes both.  True in the last block only, with
// the totals in s_out[0 .. 2 L).
template <int L>
__device__ __forceinline__ bool bicg_fold2(const BicgArgs &a, double2 acc0, double2 acc1,
                                           double2 (*s_red2)[L > 1 ? L / 2 : 1], double *s_colred, double *s_out,
                                           int *s_last)
{
    double *row = a.partials + (size_t)blockIdx.x * 2 * L;
    colpair_block_reduce<L>(acc0, s_red2, row);
    colpair_block_reduce<L>(acc1, s_red2, row + L);
    return reduce_slots<2 * L>(a.partials, a.gtickets, blockIdx.x, gridDim.x, s_colred, s_out, s_last, a.ctrl);
}

// X = 0, R = Rhat = P = B; rho_j = B_j.B_j, bnorm_j = sqrt of it (0 -> 1); scalars and control reset.
// WARM (k_cg_init's rule): X kept, a.b = a.r holds R0, so Rhat = P = R0 and rho_j = R0_j.R0_j; bnorm_j from bb_in;
// the entry test.
template <int L, bool WARM>
__global__ __launch_bounds__(kBlock) void k_bicg_init(BicgArgs a)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    __shared__ double2 s_red2[kBlock / 64][GL];
    __shared__ double s_colred[kBlock];
    __shared__ double s_out[L];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const long long npairs = a.n_elems / 2;
    double2 acc = make_double2(0.0, 0.0);
    for_pairs<GL>(npairs, 0, [&](long long i) {
        const double2 b = reinterpret_cast<const double2 *>(a.b)[i];
        if (!WARM) {
            reinterpret_cast<double2 *>(a.x)[i] = make_double2(0.0, 0.0);
            reinterpret_cast<double2 *>(a.r)[i] = b;
        }
        reinterpret_cast<double2 *>(a.rhat)[i] = b;
        reinterpret_cast<double2 *>(a.p)[i] = b;
        acc.x += b.x * b.x;
        acc.y += b.y * b.y;
    });
    if ((a.n_elems & 1) && blockIdx.x == 0 && tid == 0) {  // L == 1 with odd n
        const long long i = a.n_elems - 1;
        const double b = a.b[i];
        if (!WARM) {
            a.x[i] = 0.0;
            a.r[i] = b;
        }
        a.rhat[i] = b;
        a.p[i] = b;
        acc.x += b * b;
    }
    colpair_block_reduce<L>(acc, s_red2, a.partials + (size_t)blockIdx.x * L);
    if (!reduce_slots<L>(a.partials, a.gtickets, blockIdx.x, gridDim.x, s_colred, s_out, &s_last, a.ctrl))
        return;
    if (tid < L) {
        CgScalars &s = a.scal[tid];
        const double bb = s_out[tid];
        const double bn = sqrt(WARM ? a.bb_in[tid] : bb);
        s.rho = bb;
        s.rs_old = bb;
        s.b_norm = bn == 0.0 ? 1.0 : bn;
        s.alpha = 0.0;
        s.beta = 0.0;
        s.omega = 0.0;
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

// rhat.V per column -> red (alpha's denominator); the last block freezes the columns whose alpha is not finite.
template <int L>
__global__ __launch_bounds__(kBlock) void k_bicg_dot(BicgArgs a)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    __shared__ double2 s_red2[kBlock / 64][GL];
    __shared__ double s_colred[kBlock];
    __shared__ double s_out[L];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    if (a.ctrl->done)
        return;
    double2 acc = make_double2(0.0, 0.0);
    for_pairs<GL>(a.n_elems / 2, 0, [&](long long i) {
        const double2 h = reinterpret_cast<const double2 *>(a.rhat)[i];
        const double2 v = reinterpret_cast<const double2 *>(a.v)[i];
        acc.x += h.x * v.x;
        acc.y += h.y * v.y;
    });
    if ((a.n_elems & 1) && blockIdx.x == 0 && tid == 0)
        acc.x += a.rhat[a.n_elems - 1] * a.v[a.n_elems - 1];
    colpair_block_reduce<L>(acc, s_red2, a.partials + (size_t)blockIdx.x * L);
    if (!reduce_slots<L>(a.partials, a.gtickets, blockIdx.x, gridDim.x, s_colred, s_out, &s_last, a.ctrl))
        return;
    if (tid < L) {
        CgScalars &s = a.scal[tid];
        const double d = s_out[tid];
        a.red[tid] = d;
        double al = 0.0;
        if (!a.conv[tid]) {
            al = s.rho / d;
            if (!bicg_finite(al)) {  // rho = 0 (a zero right-hand side: 0/0) or rhat.V = 0
                a.conv[tid] = kConvBroken;
                bicg_note_freeze(a.ctrl);
                al = 0.0;
            }
        }
        s.pAp = d;
        s.alpha = al;  // for beta (the update pass's last block)
    }
    __syncthreads();
    bicg_stop_if_none_live<L>(a);
}

// s = R - alpha V in R's storage, X += alpha P (PRE: alpha Phat); every block forms the masked alpha from
// rho / red.
template <int L, bool PRE>
__global__ __launch_bounds__(kBlock) void k_bicg_s(BicgArgs a)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    if (a.ctrl->done)
        return;
    const double *dir = PRE ? a.hat : a.p;
    const double2 al = bicg_col_pair<L>([&](int j) {
        const double q = a.conv[j] ? 0.0 : a.scal[j].rho / a.red[j];
        return bicg_finite(q) ? q : 0.0;
    });
    for_pairs<GL>(a.n_elems / 2, 0, [&](long long i) {
        const double2 v = reinterpret_cast<const double2 *>(a.v)[i];
        const double2 p = reinterpret_cast<const double2 *>(dir)[i];
        double2 r = reinterpret_cast<double2 *>(a.r)[i];
        double2 x = reinterpret_cast<double2 *>(a.x)[i];
        r.x = r.x - al.x * v.x;
        r.y = r.y - al.y * v.y;
        x.x = x.x + al.x * p.x;
        x.y = x.y + al.y * p.y;
        reinterpret_cast<double2 *>(a.r)[i] = r;
        reinterpret_cast<double2 *>(a.x)[i] = x;
    });
    if ((a.n_elems & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const long long i = a.n_elems - 1;
        a.r[i] = a.r[i] - al.x * a.v[i];
        a.x[i] = a.x[i] + al.x * dir[i];
    }
}

// T.T and T.s per column in one sweep over T and s, closed by one fold of 2 L values; the last block stores
// omega = T.s / T.T (T.T == 0: s is exactly 0, the lucky half-step: omega = 0, not a breakdown).
template <int L>
__global__ __launch_bounds__(kBlock) void k_bicg_tdots(BicgArgs a)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    __shared__ double2 s_red2[kBlock / 64][GL];
    __shared__ double s_colred[kBlock];
    __shared__ double s_out[2 * L];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    if (a.ctrl->done)
        return;
    double2 tt = make_double2(0.0, 0.0), ts = make_double2(0.0, 0.0);
    for_pairs<GL>(a.n_elems / 2, 0, [&](long long i) {
        const double2 t = reinterpret_cast<const double2 *>(a.t)[i];
        const double2 s = reinterpret_cast<const double2 *>(a.r)[i];
        tt.x += t.x * t.x;
        tt.y += t.y * t.y;
        ts.x += t.x * s.x;
        ts.y += t.y * s.y;
    });
    if ((a.n_elems & 1) && blockIdx.x == 0 && tid == 0) {
        const double t = a.t[a.n_elems - 1];
        tt.x += t * t;
        ts.x += t * a.r[a.n_elems - 1];
    }
    if (!bicg_fold2<L>(a, tt, ts, s_red2, s_colred, s_out, &s_last))
        return;
    if (tid < L) {
        const double d = s_out[tid];
        double om = 0.0;
        if (!a.conv[tid] && d != 0.0) {
            om = s_out[L + tid] / d;
            if (!bicg_finite(om)) {  // x keeps alpha p, r keeps s
                a.conv[tid] = kConvBroken;
                bicg_note_freeze(a.ctrl);
                om = 0.0;
            }
        }
        a.scal[tid].omega = om;
    }
    __syncthreads();
    bicg_stop_if_none_live<L>(a);
}

// X += omega s (PRE: omega Shat), R = s - omega T, with R.R and rhat.R from the same sweep as one fold of 2 L
// values.  The last block: convergence masks, the history entry, the stop test, beta and rho (a non-finite
// beta -- rho = 0 or omega = 0 on a column still iterating -- freezes the column), the iteration counter.
template <int L, bool PRE>
__global__ __launch_bounds__(kBlock) void k_bicg_update(BicgArgs a)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    __shared__ double2 s_red2[kBlock / 64][GL];
    __shared__ double s_colred[kBlock];
    __shared__ double s_out[2 * L];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    if (a.ctrl->done)
        return;
    const double2 om = bicg_col_pair<L>([&](int j) { return a.scal[j].omega; });  // masked by k_bicg_tdots
    double2 rr = make_double2(0.0, 0.0), hr = make_double2(0.0, 0.0);
    for_pairs<GL>(a.n_elems / 2, 0, [&](long long i) {
        const double2 t = reinterpret_cast<const double2 *>(a.t)[i];
        const double2 h = reinterpret_cast<const double2 *>(a.rhat)[i];
        double2 r = reinterpret_cast<double2 *>(a.r)[i];
        double2 x = reinterpret_cast<double2 *>(a.x)[i];
        if (PRE) {
            const double2 sh = reinterpret_cast<const double2 *>(a.hat)[i];
            x.x = x.x + om.x * sh.x;
            x.y = x.y + om.y * sh.y;
        } else {
            x.x = x.x + om.x * r.x;
            x.y = x.y + om.y * r.y;
        }
        r.x = r.x - om.x * t.x;
        r.y = r.y - om.y * t.y;
        reinterpret_cast<double2 *>(a.x)[i] = x;
        reinterpret_cast<double2 *>(a.r)[i] = r;
        rr.x += r.x * r.x;
        rr.y += r.y * r.y;
        hr.x += h.x * r.x;
        hr.y += h.y * r.y;
    });
    if ((a.n_elems & 1) && blockIdx.x == 0 && tid == 0) {
        const long long i = a.n_elems - 1;
        const double s = a.r[i];
        a.x[i] = a.x[i] + om.x * (PRE ? a.hat[i] : s);
        const double r = s - om.x * a.t[i];
        a.r[i] = r;
        rr.x += r * r;
        hr.x += a.rhat[i] * r;
    }
    if (!bicg_fold2<L>(a, rr, hr, s_red2, s_colred, s_out, &s_last))
        return;
    if (tid != 0)
        return;
    const int iter = a.ctrl->iter;
    int nconv = 0;
    double maxrel = 0.0;
    for (int j = 0; j < L; ++j) {
        CgScalars &s = a.scal[j];
        s.rs_new = s_out[j];
        const double rel = sqrt(s_out[j]) / s.b_norm;
        if (a.conv[j] != kConvBroken)
            maxrel = maxrel < rel ? rel : maxrel;  // a NaN rel is skipped
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
        int live = 0;
        for (int j = 0; j < L; ++j) {
            CgScalars &s = a.scal[j];
            double be = 0.0;
            if (!a.conv[j]) {
                const double rho_new = s_out[L + j];
                be = (rho_new / s.rho) * (s.alpha / s.omega);
                if (bicg_finite(be)) {
                    s.rho = rho_new;
                    ++live;
                } else {
                    a.conv[j] = kConvBroken;
                    bicg_note_freeze(a.ctrl);
                    be = 0.0;
                }
            }
            s.beta = be;
        }
        if (live == 0) {
            a.ctrl->done = 1;
            a.ctrl->iters_out = iter + 1;
        }
    }
    a.ctrl->iter = iter + 1;
}

// P = R + beta (P - omega V), on the columns still iterating (a converged or frozen column's P stays).
template <int L>
__global__ __launch_bounds__(kBlock) void k_bicg_p(BicgArgs a)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    if (a.ctrl->done)
        return;
    const double2 be = bicg_col_pair<L>([&](int j) { return a.scal[j].beta; });
    const double2 om = bicg_col_pair<L>([&](int j) { return a.scal[j].omega; });
    const double2 live = bicg_col_pair<L>([&](int j) { return a.conv[j] ? 0.0 : 1.0; });
    for_pairs<GL>(a.n_elems / 2, 0, [&](long long i) {
        const double2 r = reinterpret_cast<const double2 *>(a.r)[i];
        const double2 v = reinterpret_cast<const double2 *>(a.v)[i];
        double2 p = reinterpret_cast<double2 *>(a.p)[i];
        const double px = r.x + be.x * (p.x - om.x * v.x);
        const double py = r.y + be.y * (p.y - om.y * v.y);
        p.x = live.x != 0.0 ? px : p.x;
        p.y = live.y != 0.0 ? py : p.y;
        reinterpret_cast<double2 *>(a.p)[i] = p;
    });
    if ((a.n_elems & 1) && blockIdx.x == 0 && threadIdx.x == 0 && live.x != 0.0) {
        const long long i = a.n_elems - 1;
        a.p[i] = a.r[i] + be.x * (a.p[i] - om.x * a.v[i]);
    }
}

static BicgArgs bicg_args(mspmv_handle_s *h, double *d_x, int L, double tol)
{
    BicgArgs a{};
    a.n_elems = (long long)h->m * L;
    a.x = d_x;
    a.r = h->d_r;
    a.rhat = h->d_rhat;
    a.p = h->d_p0;
    a.v = h->d_ap;
    a.t = h->d_p1;
    a.scal = h->d_scal;
    a.ctrl = h->d_ctrl;
    a.conv = h->d_conv;
    a.partials = h->d_partials;
    a.gtickets = h->d_gtickets;
    a.red = h->d_red;
    a.hist = h->d_hist;
    a.hist_cap = h->hist_cap;
    a.tol = tol;
    return a;
}

hipError_t launch_bicgstab_init(mspmv_handle_s *h, const double *d_b, double *d_x, int L, double tol, int nblk,
                                bool warm)
{
    BicgArgs a = bicg_args(h, d_x, L, tol);
    a.b = warm ? h->d_r : d_b;
    a.bb_in = warm ? h->d_warm : nullptr;
    return dispatch_L(L, [&](auto Lc) {
        constexpr int LL = decltype(Lc)::value;
        if (warm)
            hipLaunchKernelGGL((k_bicg_init<LL, true>), dim3(nblk), dim3(kBlock), 0, h->stream, a);
        else
            hipLaunchKernelGGL((k_bicg_init<LL, false>), dim3(nblk), dim3(kBlock), 0, h->stream, a);
        return hipGetLastError();
    });
}

hipError_t launch_bicgstab_iteration(mspmv_handle_s *h, const TilePlan &plan, const TilePlan *splan, double *d_x, int L,
                                     int nblk, double tol)
{
    const BicgArgs a = bicg_args(h, d_x, L, tol);
    hipError_t e = launch_solver_product(h, plan, splan, h->d_p0, h->d_ap, L);  // V = A P
    if (e != hipSuccess)
        return e;
    return dispatch_L(L, [&](auto Lc) {
        constexpr int LL = decltype(Lc)::value;
        const dim3 grid(nblk), block(kBlock);
        hipLaunchKernelGGL((k_bicg_dot<LL>), grid, block, 0, h->stream, a);
        hipLaunchKernelGGL((k_bicg_s<LL, false>), grid, block, 0, h->stream, a);
        hipError_t el = hipGetLastError();
        if (el != hipSuccess)
            return el;
        if ((el = launch_solver_product(h, plan, splan, h->d_r, h->d_p1, L)) != hipSuccess)  // T = A s
            return el;
        hipLaunchKernelGGL((k_bicg_tdots<LL>), grid, block, 0, h->stream, a);
        hipLaunchKernelGGL((k_bicg_update<LL, false>), grid, block, 0, h->stream, a);
        hipLaunchKernelGGL((k_bicg_p<LL>), grid, block, 0, h->stream, a);
        return hipGetLastError();
    });
}

hipError_t launch_pbicgstab_iteration(mspmv_handle_s *h, mspmv_ilu0_s *ilu, const TilePlan &plan,
                                      const TilePlan *splan, double *d_x, int L, int nblk, double tol)
{
    BicgArgs a = bicg_args(h, d_x, L, tol);
    a.hat = ilu->d_hat;
    hipError_t e = tri_apply(ilu, h->d_p0, ilu->d_hat, L, h->d_ctrl, h->stream);  // Phat
    if (e != hipSuccess)
        return e;
    if ((e = launch_solver_product(h, plan, splan, ilu->d_hat, h->d_ap, L)) != hipSuccess)  // V = A Phat
        return e;
    return dispatch_L(L, [&](auto Lc) {
        constexpr int LL = decltype(Lc)::value;
        const dim3 grid(nblk), block(kBlock);
        hipLaunchKernelGGL((k_bicg_dot<LL>), grid, block, 0, h->stream, a);
        hipLaunchKernelGGL((k_bicg_s<LL, true>), grid, block, 0, h->stream, a);
        hipError_t el = hipGetLastError();
        if (el != hipSuccess)
            return el;
        if ((el = tri_apply(ilu, h->d_r, ilu->d_hat, L, h->d_ctrl, h->stream)) != hipSuccess)  // Shat (Phat is dead)
            return el;
        if ((el = launch_solver_product(h, plan, splan, ilu->d_hat, h->d_p1, L)) != hipSuccess)  // T = A Shat
            return el;
        hipLaunchKernelGGL((k_bicg_tdots<LL>), grid, block, 0, h->stream, a);
        hipLaunchKernelGGL((k_bicg_update<LL, true>), grid, block, 0, h->stream, a);
        hipLaunchKernelGGL((k_bicg_p<LL>), grid, block, 0, h->stream, a);
        return hipGetLastError();
    });
}

}  // namespace mspmv

// mspmv_blockcg.hip -- block conjugate gradient for SPD systems (Dubrulle's BCGrQ form of O'Leary's block CG):
// the streaming passes of one iteration and their launcher.  The L columns of the row-major n x L panels share ONE
// Krylov space: every iterate minimises over the sum of the columns' spaces, so the iteration count falls as L
// grows, and an iteration is still one product (launch_solver_product) and three streaming passes.  All small
// matrices are L x L, row-major; chol(G) is the upper factor zeta with G = zeta^T zeta.
//     init:  X = 0;  H = B^T B;  zeta = chol(H);  C = zeta;  W = B zeta^-1;  S = W;  bnorm_j = ||C e_j||_2 (0 -> 1)
//     iter:  Q = A S
//            G = S^T Q;  xi = G^-1 (by chol(G));  T = xi C                               k_bcg_gram
//            X += S T;  V = W - Q xi (in W's storage);  H = V^T V                        k_bcg_step
//            zeta = chol(H);  C <- zeta C;  rel_j = ||C e_j||_2 / bnorm_j;  stop test    k_bcg_step's last block
//            W = V zeta^-1;  S = W + S zeta^T                                            k_bcg_dir
// W keeps an orthonormal basis of the residual block R = W C, so ||R e_j|| = ||C e_j|| costs no sweep, and columns
// that converge at different speeds do not drive G or H singular.  The columns are coupled: no per-column masks,
// no per-column freeze.  The init is k_bcg_init (X = 0, W = B, H and its factor) and k_bcg_dir in its FIRST form
// (W = B zeta^-1, S = W).
//
// Thread <-> data (the split CG's, for_pairs): a thread owns the column pair (j, j + 1), j = 2 (index % (L/2)), of
// the rows it meets, so every wave instruction loads or stores 1 KB of consecutive panel (whole 128-B lines, 16-B
// vector accesses).  The 1 x L by L x L product of a row needs the row's other pairs, which the L/2 neighbouring
// lanes hold: they are read across lanes (__shfl inside the aligned group of L/2 lanes; a row never straddles a
// wave because L/2 divides 64).  The coefficient columns (j, j + 1) of the small matrices are loaded once per
// thread and stay in registers (the pair never changes: for_pairs).  L == 1: the "pair" is two rows of the one
// column and every small matrix is a scalar.
//
// Summation orders, all fixed (compiled with -ffp-contract=off: every a*b+c is two roundings):
//   * a row's product: sum_k row[k] M[k][j], k ascending, starting from the k = 0 product;
//   * a Gram entry G[k][j]: per thread over its rows in sweep order, then the xor butterfly over the lanes of a wave
//     that share the pair (offsets 32 .. L/2), the waves in order, and the blocks by reduce_slots at width L^2 (groups
//     of kSlotGroup in slot order, level by level);
//   * the last block's L x L algebra, out of LDS (bcg_chol, bcg_upper_inverse, bcg_matmul): the Cholesky row by row,
//     row k's entries as A[k][q] - sum_{p<k} U[p][k] U[p][q], p ascending, reading the UPPER triangle of the folded
//     matrix only (S^T Q is symmetric up to rounding; the lower triangle is ignored); the inverse of the factor by
//     back substitution per column, k ascending; every L x L product with k ascending.
// Breakdown is one rule: a Cholesky pivot <= 0 or non-finite, of H or of G, sets ctrl->done and ctrl->breakdown
// (kBcgBroke | matrix | pivot index) in that launch.
#include "mspmv_internal.h"
#include "mspmv_device.h"

#include <cmath>

namespace mspmv {

struct BcgArgs {
    long long n_elems;  // n * L
    double *x;
    double *w;          // the orthonormal residual basis W; between k_bcg_step and k_bcg_dir it holds V
    double *s;          // the search directions S
    const double *q;    // A S
    const double *b;    // init only
    const double *bb_in;  // warm init only: [2 L] B_j.B_j, then R0_j.R0_j (k_warm_residual)
    double *small;      // the small matrices (bcg_small_*), written by the folds' last blocks
    CgControl *ctrl;
    double *partials;   // [blocks][L^2] and the fold's levels
    unsigned *gtickets;
    double *hist;
    int hist_cap;
    double tol;
};

// h->d_bcg: five L x L matrices at stride L^2, then bnorm[L]
enum { kBcgC = 0, kBcgT = 1, kBcgXi = 2, kBcgZinv = 3, kBcgZt = 4, kBcgMats = 5 };
template <int L>
__device__ __forceinline__ double *bcg_small(const BcgArgs &a, int which)
{
    return a.small + (size_t)which * L * L;
}

// The row's L values from the L/2 lanes that hold its pairs (own = this lane's pair).  Called by whole rows only.
template <int L>
__device__ __forceinline__ void bcg_row(double2 own, double (&row)[L])
{
    constexpr int GL = L / 2;
    const int base = (int)(threadIdx.x & 63) & ~(GL - 1);
#pragma unroll
    for (int k = 0; k < GL; ++k) {
        row[2 * k] = __shfl(own.x, base + k);
        row[2 * k + 1] = __shfl(own.y, base + k);
    }
}

// Columns (j, j + 1) of the small matrix m into c[k] = {m[k][j], m[k][j + 1]}; L == 1: the scalar twice.
template <int L>
__device__ __forceinline__ void bcg_coef(const double *m, double2 (&c)[L])
{
    if constexpr (L == 1) {
        c[0] = make_double2(m[0], m[0]);
    } else {
        constexpr int GL = L / 2;
        const int j = 2 * (int)(((long long)blockIdx.x * kBlock + threadIdx.x) % GL);
#pragma unroll
        for (int k = 0; k < L; ++k)
            c[k] = *reinterpret_cast<const double2 *>(&m[k * L + j]);
    }
}

// {row . m[:, j], row . m[:, j + 1]}, k ascending; L == 1: the two rows' scalars times the scalar.
template <int L>
__device__ __forceinline__ double2 bcg_mul(double2 own, const double2 (&c)[L])
{
    if constexpr (L == 1) {
        return make_double2(own.x * c[0].x, own.y * c[0].y);
    } else {
        double row[L];
        bcg_row<L>(own, row);
        double2 r = make_double2(row[0] * c[0].x, row[0] * c[0].y);
#pragma unroll
        for (int k = 1; k < L; ++k) {
            r.x += row[k] * c[k].x;
            r.y += row[k] * c[k].y;
        }
        return r;
    }
}

// acc[k] += {u[k] v[j], u[k] v[j + 1]} for the row whose pairs are u and v (this lane's): the row's share of U^T V.
template <int L>
__device__ __forceinline__ void bcg_gram_add(double2 u, double2 v, double2 (&acc)[L])
{
    if constexpr (L == 1) {
        acc[0].x += u.x * v.x;
        acc[0].y += u.y * v.y;
    } else {
        double row[L];
        bcg_row<L>(u, row);
#pragma unroll
        for (int k = 0; k < L; ++k) {
            acc[k].x += row[k] * v.x;
            acc[k].y += row[k] * v.y;
        }
    }
}

// This block's L x L partial of a Gram matrix -> its partial row (agent scope, drained), then the fold over the
// blocks: true in the last block only, the totals in s_out[L^2].  s_g: [kBlock / 64][L * GL].
template <int L>
__device__ __forceinline__ bool bcg_fold(const BcgArgs &a, double2 (&acc)[L], double2 *s_g, double *s_colred,
                                         double *s_out, int *s_last)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < L; ++k) {
        if (L == 1)
            acc[k].x += acc[k].y;
#pragma unroll
        for (int off = 32; off >= GL; off >>= 1) {
            acc[k].x += __shfl_xor(acc[k].x, off);
            if (L > 1)
                acc[k].y += __shfl_xor(acc[k].y, off);
        }
        if (lane < GL)
            s_g[(wave * L + k) * GL + lane] = acc[k];
    }
    __syncthreads();
    double *row = a.partials + (size_t)blockIdx.x * L * L;
    for (int idx = tid; idx < L * GL; idx += kBlock) {  // idx = k * GL + pair
        double2 s = s_g[idx];
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) {
            s.x += s_g[w * L * GL + idx].x;
            s.y += s_g[w * L * GL + idx].y;
        }
        if (L == 1) {
            store_sc1(&row[0], s.x);
        } else {
            store_sc1(&row[2 * idx], s.x);
            store_sc1(&row[2 * idx + 1], s.y);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    return reduce_slots<L * L>(a.partials, a.gtickets, blockIdx.x, gridDim.x, s_colred, s_out, s_last, a.ctrl);
}

// ---- the last block's L x L algebra, out of LDS; every thread of the block calls ----
// Upper Cholesky factor of the symmetric matrix whose upper triangle s_a holds, in place (the strict lower triangle
// zeroed): row k is A[k][q] - sum_{p<k} U[p][k] U[p][q] (p ascending) for q >= k, its diagonal's root taken and the
// rest divided by it.  Returns the index of the first pivot that is <= 0 or non-finite, else -1.
template <int L>
__device__ __forceinline__ int bcg_chol(double *s_a, double *s_col, int *s_piv)
{
    const int tid = threadIdx.x;
    if (tid == 0)
        *s_piv = -1;
    __syncthreads();
    for (int k = 0; k < L; ++k) {
        if (tid >= k && tid < L) {
            double s = s_a[k * L + tid];
            for (int p = 0; p < k; ++p)
                s -= s_a[p * L + k] * s_a[p * L + tid];
            s_col[tid] = s;
        }
        __syncthreads();
        const double d = s_col[k];  // block-uniform
        if (!(d > 0.0) || !(d < HUGE_VAL)) {
            if (tid == 0)
                *s_piv = k;
            break;
        }
        const double r = sqrt(d);
        if (tid >= k && tid < L)
            s_a[k * L + tid] = tid == k ? r : s_col[tid] / r;
        __syncthreads();
    }
    __syncthreads();
    if (tid < L * L && tid / L > tid % L)
        s_a[tid] = 0.0;
    __syncthreads();
    return *s_piv;
}

// s_inv = U^-1 for the upper factor s_u: thread j solves U x = e_j backwards, each x_i = -(sum_{k=i+1..j} U[i][k]
// x_k) / U[i][i] with k ascending.
template <int L>
__device__ __forceinline__ void bcg_upper_inverse(const double *s_u, double *s_inv)
{
    const int j = threadIdx.x;
    if (j < L) {
        for (int i = j + 1; i < L; ++i)
            s_inv[i * L + j] = 0.0;
        s_inv[j * L + j] = 1.0 / s_u[j * L + j];
        for (int i = j - 1; i >= 0; --i) {
            double s = s_u[i * L + i + 1] * s_inv[(i + 1) * L + j];
            for (int k = i + 2; k <= j; ++k)
                s += s_u[i * L + k] * s_inv[k * L + j];
            s_inv[i * L + j] = -s / s_u[i * L + i];
        }
    }
    __syncthreads();
}

// out = a b (BT: a b^T), thread (p, q) summing k ascending from the k = 0 product.  out is neither a nor b.
template <int L, bool BT>
__device__ __forceinline__ void bcg_matmul(const double *a, const double *b, double *out)
{
    const int tid = threadIdx.x;
    if (tid < L * L) {
        const int p = tid / L, q = tid % L;
        double s = a[p * L] * (BT ? b[q * L] : b[q]);
        for (int k = 1; k < L; ++k)
            s += a[p * L + k] * (BT ? b[q * L + k] : b[k * L + q]);
        out[tid] = s;
    }
    __syncthreads();
}

// zeta's inverse and transpose for k_bcg_dir, from the factor in s_z (s_inv: scratch).
template <int L>
__device__ __forceinline__ void bcg_store_dir(const BcgArgs &a, const double *s_z, double *s_inv)
{
    const int tid = threadIdx.x;
    bcg_upper_inverse<L>(s_z, s_inv);
    if (tid < L * L) {
        bcg_small<L>(a, kBcgZinv)[tid] = s_inv[tid];
        bcg_small<L>(a, kBcgZt)[tid] = s_z[(tid % L) * L + tid / L];
    }
}

// X = 0, W = B (raw; k_bcg_dir<L, true> scales it), H = B^T B.  The last block: zeta = chol(H), C = zeta, bnorm, the
// control word reset.  A pivot failure (a zero or dependent right-hand-side column) ends the solve here, X = 0.
// WARM (mspmv_set_initial_guess): X kept, a.b = a.w holds R0 = B - A X0 (raw), so H = R0^T R0 and C = chol(H).
// Before the factor, the entry test on H's diagonal: every sqrt(H_jj) / ||B_j|| < tol ends the solve with 0
// iterations and no breakdown; otherwise a rank-deficient R0 (an exact column) is the pivot failure above, X as
// given.  bnorm_j = ||C e_j|| (||B_j|| / ||R0_j||), the ratio from k_warm_residual's two sums, which run in one
// order: with X0 = 0 they are equal, the ratio is exactly 1 and bnorm_j has the cold init's bits.
template <int L, bool WARM>
__global__ __launch_bounds__(kBlock) void k_bcg_init(BcgArgs a)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    __shared__ double2 s_g[(kBlock / 64) * L * GL];
    __shared__ double s_colred[kBlock];
    __shared__ double s_out[L * L];
    __shared__ double s_m[L * L];
    __shared__ double s_col[L];
    __shared__ int s_last, s_piv;
    const int tid = threadIdx.x;
    double2 acc[L];
#pragma unroll
    for (int k = 0; k < L; ++k)
        acc[k] = make_double2(0.0, 0.0);
    for_pairs<GL>(a.n_elems / 2, 0, [&](long long i) {
        const double2 b = reinterpret_cast<const double2 *>(a.b)[i];
        if (!WARM) {
            reinterpret_cast<double2 *>(a.x)[i] = make_double2(0.0, 0.0);
            reinterpret_cast<double2 *>(a.w)[i] = b;
        }
        bcg_gram_add<L>(b, b, acc);
    });
    if ((a.n_elems & 1) && blockIdx.x == 0 && tid == 0) {  // L == 1 with odd n
        const long long i = a.n_elems - 1;
        const double b = a.b[i];
        if (!WARM) {
            a.x[i] = 0.0;
            a.w[i] = b;
        }
        acc[0].x += b * b;
    }
    if (!bcg_fold<L>(a, acc, s_g, s_colred, s_out, &s_last))
        return;
    if (WARM) {
        if (tid < L) {
            const double bn = sqrt(a.bb_in[tid]);
            s_col[tid] = sqrt(s_out[tid * L + tid]) / (bn == 0.0 ? 1.0 : bn);
        }
        __syncthreads();
        bool all = true;
        for (int j = 0; j < L; ++j)
            all = all && s_col[j] < a.tol;  // a NaN ratio: not converged
        if (all) {
            if (tid == 0) {
                a.ctrl->iter = 0;
                a.ctrl->iters_out = 0;
                a.ctrl->done = 1;
                a.ctrl->breakdown = 0;
            }
            return;
        }
        __syncthreads();  // bcg_chol reuses s_col
    }
    const int piv = bcg_chol<L>(s_out, s_col, &s_piv);
    if (tid == 0) {
        a.ctrl->iter = 0;
        a.ctrl->iters_out = 0;
        a.ctrl->done = piv >= 0;
        a.ctrl->breakdown = piv >= 0 ? (kBcgBroke | piv) : 0;
    }
    if (piv >= 0)
        return;
    if (tid < L * L)
        bcg_small<L>(a, kBcgC)[tid] = s_out[tid];
    if (tid < L) {
        double s = s_out[tid] * s_out[tid];
        for (int p = 1; p < L; ++p)
            s += s_out[p * L + tid] * s_out[p * L + tid];
        double bn = sqrt(s);
        if (WARM)
            bn = bn * (sqrt(a.bb_in[tid]) / sqrt(a.bb_in[L + tid]));
        bcg_small<L>(a, kBcgMats)[tid] = bn == 0.0 ? 1.0 : bn;
    }
    bcg_store_dir<L>(a, s_out, s_m);
}

// G = S^T Q.  The last block: chol(G), xi = G^-1 = Gamma^-1 Gamma^-T, T = xi C.
template <int L>
__global__ __launch_bounds__(kBlock) void k_bcg_gram(BcgArgs a)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    __shared__ double2 s_g[(kBlock / 64) * L * GL];
    __shared__ double s_colred[kBlock];
    __shared__ double s_out[L * L];
    __shared__ double s_m[L * L];
    __shared__ double s_xi[L * L];
    __shared__ double s_col[L];
    __shared__ int s_last, s_piv;
    const int tid = threadIdx.x;
    if (a.ctrl->done)
        return;
    double2 acc[L];
#pragma unroll
    for (int k = 0; k < L; ++k)
        acc[k] = make_double2(0.0, 0.0);
    for_pairs<GL>(a.n_elems / 2, 0, [&](long long i) {
        const double2 s = reinterpret_cast<const double2 *>(a.s)[i];
        const double2 q = reinterpret_cast<const double2 *>(a.q)[i];
        bcg_gram_add<L>(s, q, acc);
    });
    if ((a.n_elems & 1) && blockIdx.x == 0 && tid == 0)
        acc[0].x += a.s[a.n_elems - 1] * a.q[a.n_elems - 1];
    if (!bcg_fold<L>(a, acc, s_g, s_colred, s_out, &s_last))
        return;
    const int piv = bcg_chol<L>(s_out, s_col, &s_piv);
    if (piv >= 0) {  // X is the iterate of the iterations completed so far
        if (tid == 0) {
            a.ctrl->done = 1;
            a.ctrl->breakdown = kBcgBroke | kBcgBrokeG | piv;
            a.ctrl->iters_out = a.ctrl->iter;
        }
        return;
    }
    bcg_upper_inverse<L>(s_out, s_m);
    bcg_matmul<L, true>(s_m, s_m, s_xi);
    if (tid < L * L) {
        bcg_small<L>(a, kBcgXi)[tid] = s_xi[tid];
        s_m[tid] = bcg_small<L>(a, kBcgC)[tid];
    }
    __syncthreads();
    bcg_matmul<L, false>(s_xi, s_m, s_out);
    if (tid < L * L)
        bcg_small<L>(a, kBcgT)[tid] = s_out[tid];
}

// X += S T, V = W - Q xi in W's storage, H = V^T V.  The last block: zeta = chol(H), C <- zeta C, the residual norms
// ||C e_j|| / bnorm_j, the history entry, the stop test and the iteration counter, zeta^-1 and zeta^T for k_bcg_dir.
// A pivot failure of H (an exactly converged direction) comes after X took this iteration's update, so the iteration
// counts as completed: its residual norms are sqrt((C^T H C)_jj), taken from H itself instead of its factor.
template <int L>
__global__ __launch_bounds__(kBlock) void k_bcg_step(BcgArgs a)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    __shared__ double2 s_g[(kBlock / 64) * L * GL];
    __shared__ double s_colred[kBlock];
    __shared__ double s_out[L * L];
    __shared__ double s_m[L * L];
    __shared__ double s_c[L * L];
    __shared__ double s_h[L * L];
    __shared__ double s_col[L];
    __shared__ int s_last, s_piv;
    const int tid = threadIdx.x;
    if (a.ctrl->done)
        return;
    double2 ct[L], cxi[L], acc[L];
    bcg_coef<L>(bcg_small<L>(a, kBcgT), ct);
    bcg_coef<L>(bcg_small<L>(a, kBcgXi), cxi);
#pragma unroll
    for (int k = 0; k < L; ++k)
        acc[k] = make_double2(0.0, 0.0);
    for_pairs<GL>(a.n_elems / 2, 0, [&](long long i) {
        const double2 s = reinterpret_cast<const double2 *>(a.s)[i];
        const double2 q = reinterpret_cast<const double2 *>(a.q)[i];
        double2 w = reinterpret_cast<double2 *>(a.w)[i];
        double2 x = reinterpret_cast<double2 *>(a.x)[i];
        const double2 st = bcg_mul<L>(s, ct);
        const double2 qx = bcg_mul<L>(q, cxi);
        x.x = x.x + st.x;
        x.y = x.y + st.y;
        w.x = w.x - qx.x;
        w.y = w.y - qx.y;
        reinterpret_cast<double2 *>(a.x)[i] = x;
        reinterpret_cast<double2 *>(a.w)[i] = w;
        bcg_gram_add<L>(w, w, acc);
    });
    if ((a.n_elems & 1) && blockIdx.x == 0 && tid == 0) {
        const long long i = a.n_elems - 1;
        a.x[i] = a.x[i] + a.s[i] * ct[0].x;
        const double v = a.w[i] - a.q[i] * cxi[0].x;
        a.w[i] = v;
        acc[0].x += v * v;
    }
    if (!bcg_fold<L>(a, acc, s_g, s_colred, s_out, &s_last))
        return;
    if (tid < L * L) {
        const int p = tid / L, q = tid % L;
        s_h[tid] = p <= q ? s_out[tid] : s_out[q * L + p];  // H, from its upper triangle
        s_c[tid] = bcg_small<L>(a, kBcgC)[tid];
    }
    __syncthreads();
    const int piv = bcg_chol<L>(s_out, s_col, &s_piv);
    if (piv >= 0) {
        bcg_matmul<L, false>(s_h, s_c, s_m);  // H C
        if (tid < L) {
            double s = s_c[tid] * s_m[tid];
            for (int p = 1; p < L; ++p)
                s += s_c[p * L + tid] * s_m[p * L + tid];
            s_col[tid] = sqrt(s) / bcg_small<L>(a, kBcgMats)[tid];
        }
    } else {
        bcg_matmul<L, false>(s_out, s_c, s_m);  // zeta C
        if (tid < L * L)
            bcg_small<L>(a, kBcgC)[tid] = s_m[tid];
        if (tid < L) {
            double s = s_m[tid] * s_m[tid];
            for (int p = 1; p < L; ++p)
                s += s_m[p * L + tid] * s_m[p * L + tid];
            s_col[tid] = sqrt(s) / bcg_small<L>(a, kBcgMats)[tid];
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int iter = a.ctrl->iter;
        double maxrel = 0.0;
        bool all = true;
        for (int j = 0; j < L; ++j) {
            const double rel = s_col[j];
            maxrel = maxrel < rel ? rel : maxrel;  // a NaN rel is skipped
            all = all && rel < a.tol;
        }
        if (a.hist && iter < a.hist_cap)
            a.hist[iter] = maxrel;
        if (piv >= 0) {
            a.ctrl->done = 1;
            a.ctrl->breakdown = kBcgBroke | piv;
            a.ctrl->iters_out = iter + 1;
        } else if (all) {
            a.ctrl->done = 1;
            a.ctrl->iters_out = iter + 1;
        }
        a.ctrl->iter = iter + 1;
    }
    if (piv < 0)
        bcg_store_dir<L>(a, s_out, s_h);
}

// W = V zeta^-1, S = W + S zeta^T; FIRST (the init): W = B zeta^-1, S = W.
template <int L, bool FIRST>
__global__ __launch_bounds__(kBlock) void k_bcg_dir(BcgArgs a)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    if (a.ctrl->done)
        return;
    double2 czi[L], czt[L];
    bcg_coef<L>(bcg_small<L>(a, kBcgZinv), czi);
    if (!FIRST)
        bcg_coef<L>(bcg_small<L>(a, kBcgZt), czt);
    for_pairs<GL>(a.n_elems / 2, 0, [&](long long i) {
        const double2 v = reinterpret_cast<double2 *>(a.w)[i];
        const double2 w = bcg_mul<L>(v, czi);
        double2 s = w;
        if (!FIRST) {
            const double2 sz = bcg_mul<L>(reinterpret_cast<double2 *>(a.s)[i], czt);
            s.x = w.x + sz.x;
            s.y = w.y + sz.y;
        }
        reinterpret_cast<double2 *>(a.w)[i] = w;
        reinterpret_cast<double2 *>(a.s)[i] = s;
    });
    if ((a.n_elems & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const long long i = a.n_elems - 1;
        const double w = a.w[i] * czi[0].x;
        a.w[i] = w;
        a.s[i] = FIRST ? w : w + a.s[i] * czt[0].x;
    }
}

static BcgArgs bcg_args(mspmv_handle_s *h, double *d_x, int L, double tol)
{
    BcgArgs a{};
    a.n_elems = (long long)h->m * L;
    a.x = d_x;
    a.w = h->d_r;
    a.s = h->d_p0;
    a.q = h->d_ap;
    a.small = h->d_bcg;
    a.ctrl = h->d_ctrl;
    a.partials = h->d_partials;
    a.gtickets = h->d_gtickets;
    a.hist = h->d_hist;
    a.hist_cap = h->hist_cap;
    a.tol = tol;
    return a;
}

hipError_t launch_bcg_init(mspmv_handle_s *h, const double *d_b, double *d_x, int L, double tol, int nblk, bool warm)
{
    BcgArgs a = bcg_args(h, d_x, L, tol);
    a.b = warm ? h->d_r : d_b;
    a.bb_in = warm ? h->d_warm : nullptr;
    return dispatch_L(L, [&](auto Lc) {
        constexpr int LL = decltype(Lc)::value;
        if (warm)
            hipLaunchKernelGGL((k_bcg_init<LL, true>), dim3(nblk), dim3(kBlock), 0, h->stream, a);
        else
            hipLaunchKernelGGL((k_bcg_init<LL, false>), dim3(nblk), dim3(kBlock), 0, h->stream, a);
        hipLaunchKernelGGL((k_bcg_dir<LL, true>), dim3(nblk), dim3(kBlock), 0, h->stream, a);
        return hipGetLastError();
    });
}

hipError_t launch_bcg_iteration(mspmv_handle_s *h, const TilePlan &plan, const TilePlan *splan, double *d_x, int L,
                                int nblk, double tol)
{
    const BcgArgs a = bcg_args(h, d_x, L, tol);
    hipError_t e = launch_solver_product(h, plan, splan, h->d_p0, h->d_ap, L);  // Q = A S
    if (e != hipSuccess)
        return e;
    return dispatch_L(L, [&](auto Lc) {
        constexpr int LL = decltype(Lc)::value;
        const dim3 grid(nblk), block(kBlock);
        hipLaunchKernelGGL((k_bcg_gram<LL>), grid, block, 0, h->stream, a);
        hipLaunchKernelGGL((k_bcg_step<LL>), grid, block, 0, h->stream, a);
        hipLaunchKernelGGL((k_bcg_dir<LL, false>), grid, block, 0, h->stream, a);
        return hipGetLastError();
    });
}

}  // namespace mspmv

// mspmv_color.hip -- the triangular solves of a multi-colour ILU(0) or IC(0) factor (mspmv_ilu0_create_colored,
// mspmv_ic0_create_colored): one launch per colour, stream order the only dependency mechanism.
//
// The factor is that of Ap = P A P^T with the rows of a colour contiguous (mspmv_color.cpp).  Rows of one colour
// share no entry, so a row of L reads only rows of earlier colours and a row of U (or L^T) only rows of later ones:
// when colour c's launch starts, everything it reads was written by launches that have finished.  No pending
// pattern, no fill, no polling, no stall status, and no wave per row: a row is served by max(1, L / 2) lanes, each
// owning one column pair (one column at L = 1) of the panel, so a workgroup covers 256 / max(1, L / 2) rows of the
// colour's range and a 5-point stencil's rows of 2-4 entries waste nothing.
//
// Exactness.  A lane walks its row's off-diagonal entries in CSR order and sums the products a_ij x_j the way the
// numpy restatement of the tests does (tests/test_ilu0.py TriPlan: np.add.reduceat over the row's products): the
// first product plus the pairwise sum of the rest, where the pairwise sum of n values is
//     n < 8      the values added in order, starting from the first;
//     n <= 128   eight running sums r[j] = v[j] + v[8 + j] + v[16 + j] + ..., folded
//                ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the n % 8 trailing values added in order;
//     n > 128    the pairwise sums of the first n2 = (n / 2) - (n / 2) % 8 values and of the rest, added.
// Up to three entries that is the plain sequential sum.  Then x_i = b_i - s (ILU(0)'s L, unit diagonal implied),
// (b_i - s) / u_ii (U, L^T: the diagonal first in the row) or (b_i - s) / l_ii (IC(0)'s L: the diagonal last in
// the row, the sum over the entries before it); a row without off-diagonal entries takes b_i or b_i / d.  Built
// with -ffp-contract=off, so every product and every sum rounds once, and the solve equals TriPlan's bit for bit.
// The cost of that: a long row (a hub row sits alone in its colour) is summed by its max(1, L / 2) lanes alone,
// one entry after the other -- a launch of one row as long as the matrix.  Rows past 129 entries take the LONG
// instantiation (the split above on a small per-lane stack); the host picks it per colour.
#include "mspmv_internal.h"
#include "mspmv_device.h"

namespace mspmv {

constexpr int kPwBlock = 128;  // the pairwise sum's largest unsplit block

__device__ __forceinline__ double2 add2(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }

// The column pair g of row r of an n x L panel (L == 1: the one value, in .x).
template <int L>
__device__ __forceinline__ double2 load_cols(const double *p, int r, int g)
{
    if constexpr (L == 1)
        return make_double2(p[r], 0.0);
    else
        return reinterpret_cast<const double2 *>(p + (size_t)r * L)[g];
}
template <int L>
__device__ __forceinline__ void store_cols(double *p, int r, int g, double2 v)
{
    if constexpr (L == 1)
        p[r] = v.x;
    else
        reinterpret_cast<double2 *>(p + (size_t)r * L)[g] = v;
}

// The products of a row's entries [k, ...) with the solved rows they name.
template <int L>
struct RowProducts {
    const int *ci;
    const double *va;
    const double *x;
    int g;
    __device__ __forceinline__ double2 operator()(int k) const
    {
        const double a = va[k];
        const double2 v = load_cols<L>(x, ci[k], g);
        return make_double2(a * v.x, a * v.y);
    }
};

// Pairwise sum of the n <= kPwBlock products from k on (n >= 1).
template <int L>
__device__ __forceinline__ double2 pw_block(const RowProducts<L> &prod, int k, int n)
{
    if (n < 8) {
        double2 r = prod(k);
        for (int i = 1; i < n; ++i)
            r = add2(r, prod(k + i));
        return r;
    }
    double2 r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
        r[j] = prod(k + j);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            r[j] = add2(r[j], prod(k + i + j));
    }
    double2 res = add2(add2(add2(r[0], r[1]), add2(r[2], r[3])), add2(add2(r[4], r[5]), add2(r[6], r[7])));
    for (; i < n; ++i)
        res = add2(res, prod(k + i));
    return res;
}

// Pairwise sum of any n >= 1 products: the halving above, depth first.  A pending half and a pending addition per
// level: n < 2^31 and blocks of 128 keep the work stack under 50 entries and the value stack under 25.
template <int L>
__device__ __noinline__ double2 pw_long(const RowProducts<L> &prod, int k, int n)
{
    int wk[56], wn[56];  // work: n > 0 a range to sum, n < 0 add the two newest values
    double2 val[28];
    int wt = 1, vt = 0;
    wk[0] = k;
    wn[0] = n;
    while (wt > 0) {
        --wt;
        const int s = wk[wt], c = wn[wt];
        if (c < 0) {
            --vt;
            val[vt - 1] = add2(val[vt - 1], val[vt]);
        } else if (c <= kPwBlock) {
            val[vt++] = pw_block<L>(prod, s, c);
        } else {
            int n2 = c / 2;
            n2 -= n2 % 8;
            wk[wt] = 0, wn[wt++] = -1;
            wk[wt] = s + n2, wn[wt++] = c - n2;
            wk[wt] = s, wn[wt++] = n2;
        }
    }
    return val[0];
}

// The triangle a launch solves.
enum TriForm {
    kLowerUnit,  // ILU(0)'s L: strictly lower entries, unit diagonal implied
    kUpper,      // U or L^T: the diagonal is the row's first entry
    kLowerDiag,  // IC(0)'s L: the diagonal is the row's last entry
    kLowerTurn   // kLowerDiag on the apply's last colour, whose rows of L^T hold the diagonal alone: the backward
                 // sweep's division runs here too, y = (r - s) / d, z = y / d, two roundings as in the two launches
};

// Rows [row0, row1) of one colour.  PERM (the apply): the forward sweep reads b at perm[i] (A's ordering) and
// writes x at i (the colour ordering); the backward sweep reads and writes x at i -- b is x there, in place -- and
// also writes out at perm[i]; kLowerTurn writes z at both.  Without PERM: b, x at i, out unused.
// b and x may be the same panel (no __restrict__): a row reads x only at rows of other colours.
template <int L, TriForm T, bool PERM, bool LONG>
__global__ __launch_bounds__(kBlock) void k_trsv_color(const int *__restrict__ ro, const int *__restrict__ ci,
                                                       const double *__restrict__ va, int row0, int row1,
                                                       const int *__restrict__ perm, const double *b, double *x,
                                                       double *out, const CgControl *ctrl)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    constexpr bool UPPER = T == kUpper, LDIAG = T == kLowerDiag || T == kLowerTurn;
    static_assert(T != kLowerTurn || PERM, "the fused colour is the apply's");
    if (ctrl->done)  // set only by earlier launches: uniform here
        return;
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    const long long row = row0 + t / GL;
    if (row >= row1)
        return;
    const int i = (int)row, g = (int)(t % GL);
    int k = ro[i];
    int k1 = ro[i + 1];
    double d = 1.0;
    if (UPPER)
        d = va[k++];
    if (LDIAG)
        d = va[--k1];
    const int src = (PERM && !UPPER) ? perm[i] : i;
    double2 xi = load_cols<L>(b, src, g);
    const int m = k1 - k;
    if (m > 0) {
        const RowProducts<L> prod{ci, va, x, g};
        double2 s = prod(k);
        if (m > 1) {
            if (LONG && m - 1 > kPwBlock)
                s = add2(s, pw_long<L>(prod, k + 1, m - 1));
            else
                s = add2(s, pw_block<L>(prod, k + 1, m - 1));
        }
        xi = make_double2(xi.x - s.x, xi.y - s.y);
    }
    if (UPPER || LDIAG)
        xi = make_double2(xi.x / d, xi.y / d);
    if (T == kLowerTurn)
        xi = make_double2(xi.x / d, xi.y / d);
    store_cols<L>(x, i, g, xi);
    if ((UPPER || T == kLowerTurn) && PERM)
        store_cols<L>(out, perm[i], g, xi);
}

// One colour's launch.
template <int L, TriForm T, bool PERM>
static void color_sweep(const TriFactor *t, int c, const double *b, double *x, double *out, const CgControl *ctrl,
                        hipStream_t s)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    constexpr bool UPPER = T == kUpper;
    const int row0 = t->color_off[c], row1 = t->color_off[(size_t)c + 1];
    const long long threads = (long long)(row1 - row0) * GL;
    const dim3 grid((unsigned)((threads + kBlock - 1) / kBlock)), block(kBlock);
    const int *ro = UPPER ? t->d_uro : t->d_lro, *ci = UPPER ? t->d_uci : t->d_lci;
    const double *va = UPPER ? t->d_uva : t->d_lva;
    dispatch_bool((UPPER ? t->umax[c] : t->lmax[c]) - 1 > kPwBlock, [&](auto lg) {
        hipLaunchKernelGGL((k_trsv_color<L, T, PERM, decltype(lg)::value>), grid, block, 0, s, ro, ci, va, row0, row1,
                           t->d_perm, b, x, out, ctrl);
    });
}

hipError_t launch_color_trsv(const TriFactor *t, bool upper, const double *d_b, double *d_x, int L,
                             const CgControl *ctrl, hipStream_t s)
{
    const int C = t->num_colors;
    return dispatch_L(L, [&](auto Lc) {
        constexpr int LL = decltype(Lc)::value;
        for (int c = 0; c < C; ++c) {
            if (upper)
                color_sweep<LL, kUpper, false>(t, C - 1 - c, d_b, d_x, nullptr, ctrl, s);
            else if (t->l_diag)
                color_sweep<LL, kLowerDiag, false>(t, c, d_b, d_x, nullptr, ctrl, s);
            else
                color_sweep<LL, kLowerUnit, false>(t, c, d_b, d_x, nullptr, ctrl, s);
        }
        return hipGetLastError();
    });
}

hipError_t launch_color_apply(const TriFactor *t, const double *d_src, double *d_dst, int L, const CgControl *ctrl,
                              hipStream_t s)
{
    const int C = t->num_colors;
    double *y = t->d_y;
    return dispatch_L(L, [&](auto Lc) {
        constexpr int LL = decltype(Lc)::value;
        if (t->l_diag) {  // IC(0): 2 C - 1 launches, the turn-around colour fused
            for (int c = 0; c < C - 1; ++c)
                color_sweep<LL, kLowerDiag, true>(t, c, d_src, y, nullptr, ctrl, s);
            color_sweep<LL, kLowerTurn, true>(t, C - 1, d_src, y, d_dst, ctrl, s);
            for (int c = C - 2; c >= 0; --c)
                color_sweep<LL, kUpper, true>(t, c, y, y, d_dst, ctrl, s);
            return hipGetLastError();
        }
        for (int c = 0; c < C; ++c)
            color_sweep<LL, kLowerUnit, true>(t, c, d_src, y, nullptr, ctrl, s);
        for (int c = C - 1; c >= 0; --c)
            color_sweep<LL, kUpper, true>(t, c, y, y, d_dst, ctrl, s);
        return hipGetLastError();
    });
}

}  // namespace mspmv

// mspmv_warm.hip -- the warm start's one pass (mspmv_set_initial_guess, MSPMV_X0_CALLER) and the fused true
// residual (mspmv_dresidual_dev): R = B - W for W = A X already in memory, with B.B and R.R per column from the same
// sweep.  A warm solve enqueues W = A X0 on the path its own products take, then this pass, then its init in the
// warm instantiation (k_cg_init, k_bicg_init, k_bcg_init), which takes R0 where the cold one takes B, keeps X and
// sets b_norm from the B.B handed over here.
// Orders, all fixed: the grid, the sweep (for_pairs, first chunk to last) and the per-block column-pair reduction are
// the cold inits'; the two sums close under ONE round of tickets, each folded at width L in reduce_slots' order
// (warm_fold2), so B.B has the bits the cold init's own B.B has, and with X0 = 0 (W = 0, R0 = B) so has R.R.
// Compiled with -ffp-contract=off like every kernel here: every a*b+c is two roundings.
#include "mspmv_internal.h"
#include "mspmv_device.h"

namespace mspmv {

struct WarmArgs {
    long long n_elems;  // m * L
    const double *b;
    const double *w;    // A X
    double *r;          // B - A X (null: the norms alone)
    double *partials;   // two regions of partials_capacity(blocks, L): B.B's rows, then R.R's at +part2
    size_t part2;
    unsigned *gtickets;
    double *out;        // [2 L]: B_j.B_j, then R_j.R_j
    CgControl *ctrl;    // a ticket fault is raised in ctrl->fault
};

// reduce_slots for two [slots][L] partial arrays under one round of tickets: the group's last arriver folds both,
// each by fold_cols<L> in slot order -- per column the order reduce_slots<L> gives either array alone.  True in the
// last block only, the totals in s_out[0 .. L) and s_out[L .. 2 L).
template <int L>
__device__ __forceinline__ bool warm_fold2(double *p0, double *p1, unsigned *tickets, int slot, int nslots,
                                           double *s_tmp, double *s_out, int *s_flag, CgControl *ctrl)
{
    const int tid = threadIdx.x;
    size_t lvl = 0;
    int idx = slot, count = nslots;
    for (;;) {
        const int g = idx / kSlotGroup;
        const int ngroups = (count + kSlotGroup - 1) / kSlotGroup;
        const int gsize = min(kSlotGroup, count - g * kSlotGroup);
        unsigned *tk = &tickets[(size_t)g * kTicketStride];
        if (tid == 0)
            *s_flag = take_ticket<false>(tk, gsize, ctrl);
        __syncthreads();
        if (!*s_flag)
            return false;
        fold_cols<L>(p0 + lvl + (size_t)g * kSlotGroup * L, gsize, s_tmp, s_out);
        fold_cols<L>(p1 + lvl + (size_t)g * kSlotGroup * L, gsize, s_tmp, s_out + L);
        if (tid == 0)
            __hip_atomic_store(tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ngroups == 1)
            return true;
        const size_t next = lvl + (size_t)count * L;
        if (tid < 2 * L) {
            store_sc1(&(tid < L ? p0 : p1)[next + (size_t)g * L + tid % L], s_out[tid]);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        tickets += (size_t)ngroups * kTicketStride;
        lvl = next;
        idx = g;
        count = ngroups;
    }
}

template <int L>
__global__ __launch_bounds__(kBlock) void k_warm_residual(WarmArgs a)
{
    constexpr int GL = L > 1 ? L / 2 : 1;
    __shared__ double2 s_red2[kBlock / 64][GL];
    __shared__ double s_colred[kBlock];
    __shared__ double s_out[2 * L];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    double2 bb = make_double2(0.0, 0.0), rr = make_double2(0.0, 0.0);
    for_pairs<GL>(a.n_elems / 2, 0, [&](long long i) {
        const double2 b = reinterpret_cast<const double2 *>(a.b)[i];
        const double2 w = reinterpret_cast<const double2 *>(a.w)[i];
        const double2 r = make_double2(b.x - w.x, b.y - w.y);
        if (a.r)
            reinterpret_cast<double2 *>(a.r)[i] = r;
        bb.x += b.x * b.x;
        bb.y += b.y * b.y;
        rr.x += r.x * r.x;
        rr.y += r.y * r.y;
    });
    if ((a.n_elems & 1) && blockIdx.x == 0 && tid == 0) {  // L == 1 with odd m
        const long long i = a.n_elems - 1;
        const double b = a.b[i];
        const double r = b - a.w[i];
        if (a.r)
            a.r[i] = r;
        bb.x += b * b;
        rr.x += r * r;
    }
    colpair_block_reduce<L>(bb, s_red2, a.partials + (size_t)blockIdx.x * L);
    colpair_block_reduce<L>(rr, s_red2, a.partials + a.part2 + (size_t)blockIdx.x * L);
    if (!warm_fold2<L>(a.partials, a.partials + a.part2, a.gtickets, blockIdx.x, gridDim.x, s_colred, s_out, &s_last,
                       a.ctrl))
        return;
    if (tid < 2 * L)
        a.out[tid] = s_out[tid];
}

// R = B - W with the column sums into h->d_warm ([2 L]), on h's stream: nblk blocks, the handle's partials (sized
// for rows 2 L wide by the caller) and tickets (zero on entry).  d_R null: the sums alone.
hipError_t launch_warm_residual(mspmv_handle_s *h, const double *d_B, const double *d_W, double *d_R, int L, int nblk)
{
    WarmArgs a{};
    a.n_elems = (long long)h->m * L;
    a.b = d_B;
    a.w = d_W;
    a.r = d_R;
    a.partials = h->d_partials;
    a.part2 = partials_capacity((size_t)nblk, L);
    a.gtickets = h->d_gtickets;
    a.out = h->d_warm;
    a.ctrl = h->d_ctrl;
    return dispatch_L(L, [&](auto Lc) {
        hipLaunchKernelGGL((k_warm_residual<decltype(Lc)::value>), dim3(nblk), dim3(kBlock), 0, h->stream, a);
        return hipGetLastError();
    });
}

}  // namespace mspmv

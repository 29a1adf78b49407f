// mspmv_kernels.hip -- hand-written gfx950 (CDNA4) kernels for merge-path CSR SpMV/SpMM, their
// plan-building kernels and their launchers (the CG passes above them: mspmv_cg_passes.hip).  Compiled with -ffp-contract=off: every a*b+c is two roundings, as
// in the reference built for the x86-64 baseline ISA, so rows that no tile/thread boundary
// splits are bit-identical to SpmvGold (cpu_spmv.cpp:241-265).
//
// Algorithm (Merrill & Garland merge-path, re-derived for 64-lane waves):
//   * the (row-end-offsets x nnz-index) merge path is cut into tiles of `tile_items` merge
//     items at setup (k_merge_coords + k_snap, once per matrix -- the matrix is immutable);
//   * one 256-thread workgroup per tile stages the tile's row end offsets and its
//     products val*x[col] (SpMV) or its (col, val) pairs (SpMM) in LDS with fully
//     coalesced loads, then every thread (SpMV) or every group of L/2 lanes (SpMM, one
//     double2 of the row-major panel per lane) runs its own merge-path search in LDS and
//     walks an equal share of merge items;
//   * rows split between threads are closed in LDS in thread order; rows split between
//     tiles (only inside rows longer than the snap distance) are closed by the tile that
//     completes them, in tile order (close_split_rows).  All reductions are fixed-order: results are run-to-run deterministic.
//   * tiles are dealt XCD-contiguously (blocks b and b+8 share an XCD), so each XCD's L2
//     sees one contiguous band of x / X.
#include "mspmv_internal.h"
#include "mspmv_device.h"

#include <algorithm>
#include <type_traits>
#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace mspmv {

// ------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------

template <typename... KArgs, typename... Args>
static void ggl(void (*kernel)(KArgs...), dim3 grid, dim3 block, hipStream_t s, Args... args)
{
    hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
}

// Streamed-once matrix arrays: nontemporal loads (don't displace x / X from the caches).
template <bool NT, typename T>
__device__ __forceinline__ T ld_stream(const T *p)
{
    if (NT)
        return __builtin_nontemporal_load(p);
    return *p;
}
typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v2i_t __attribute__((ext_vector_type(2)));
template <bool NT>
__device__ __forceinline__ int4 ld_stream(const int4 *p)
{
    if (NT) {
        const v4i_t t = __builtin_nontemporal_load(reinterpret_cast<const v4i_t *>(p));
        return make_int4(t.x, t.y, t.z, t.w);
    }
    return *p;
}
template <bool NT>
__device__ __forceinline__ double2 ld_stream(const double2 *p)
{
    if (NT) {
        const v2d_t t = __builtin_nontemporal_load(reinterpret_cast<const v2d_t *>(p));
        return make_double2(t.x, t.y);
    }
    return *p;
}

// Merge-path search (cpu_spmv.cpp:208-235 semantics) over an LDS copy of the tile's row
// end offsets, stored relative to the tile's first nonzero; list B is 0..b_len-1.
__device__ __forceinline__ void lds_search(int d, const int *s_rowend, int a_len, int b_len, int &x, int &y)
{
    int lo = d - b_len > 0 ? d - b_len : 0;
    int hi = d < a_len ? d : a_len;
    while (lo < hi) {
        const int pivot = (lo + hi) >> 1;
        if (s_rowend[pivot] <= d - pivot - 1)
            lo = pivot + 1;
        else
            hi = pivot;
    }
    x = lo;
    y = d - lo;
}

// ------------------------------------------------------------------------------------------
// partition: the reference's partition coordinates and the tile plan boundaries
// ------------------------------------------------------------------------------------------
__global__ void k_merge_coords(const int *__restrict__ row_offsets, int m, int nnz, long long step, int num_parts,
                               int2 *__restrict__ out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > num_parts)
        return;
    const long long total = (long long)m + nnz;
    long long dl = step * (long long)t;
    const int d = (int)(dl < total ? dl : total);
    const int *a = row_offsets + 1;
    int lo = d - nnz > 0 ? d - nnz : 0;
    int hi = d < m ? d : m;
    while (lo < hi) {
        const int pivot = (lo + hi) >> 1;
        if (a[pivot] <= d - pivot - 1)
            lo = pivot + 1;
        else
            hi = pivot;
    }
    out[t] = make_int2(lo < m ? lo : m, d - lo);
}

__global__ void k_snap(const int *__restrict__ row_offsets, int m, int2 *__restrict__ b,
                       unsigned char *__restrict__ split, int T, int snap)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > T)
        return;
    int2 c = b[t];
    unsigned char s = 0;
    if (t > 0 && t < T && c.x < m) {
        const int start = row_offsets[c.x];
        if (c.y - start <= snap)
            c.y = start;  // row entered by <= snap nonzeros: the completing tile takes it whole
        else
            s = 1;        // deep inside a long row: exact merge coordinate, carry crosses it
    }
    b[t] = c;
    split[t] = s;
}

// 16-bit column offsets, one workgroup per tile: the tile's column range (block min / max), and
// when it spans < 65536 columns, cols16[k] = col[k] - colbase[t] for the tile's nonzeros.
__global__ __launch_bounds__(kBlock) void k_pack_cols16(const int *__restrict__ cols, const int2 *__restrict__ bounds,
                                                        int *__restrict__ colbase, unsigned short *__restrict__ cols16)
{
    __shared__ int s_min[kBlock / 64], s_max[kBlock / 64];
    const int t = blockIdx.x, tid = threadIdx.x;
    const int n0 = bounds[t].y, n1 = bounds[t + 1].y;
    int lo = 0x7fffffff, hi = -1;
    for (int k = n0 + tid; k < n1; k += kBlock) {
        const int c = cols[k];
        lo = min(lo, c);
        hi = max(hi, c);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off));
        hi = max(hi, __shfl_xor(hi, off));
    }
    if ((tid & 63) == 0) {
        s_min[tid >> 6] = lo;
        s_max[tid >> 6] = hi;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        lo = min(lo, s_min[w]);
        hi = max(hi, s_max[w]);
    }
    const int base = (n1 > n0 && hi - lo < 65536) ? lo : -1;
    if (tid == 0)
        colbase[t] = base;
    if (base >= 0)
        for (int k = n0 + tid; k < n1; k += kBlock)
            cols16[k] = (unsigned short)(cols[k] - base);
}

// Per-tile column dictionary (plan time, single-RHS plans): one workgroup per
// tile sorts the tile's column ids in LDS (bitonic, N = power of two >= the tile's nonzeros),
// keeps the distinct ones in ascending order -> dict[n0 + d], d < ndict[t] (stored in the tile's
// own nonzero range: ndict <= nnzt), and rewrites every nonzero as its dictionary position ->
// idx16[k].  The kernel then gathers each distinct x once per tile instead of once per nonzero.
// ratio < 0: a multi-RHS plan (k_spmm_tile parks the distinct panel rows in LDS): every tile
// whose nonzeros repeat its distinct columns at least twice and has at most dmax of them takes
// its dictionary, without the single-RHS line test.
template <int N>
__global__ __launch_bounds__(kBlock) void k_build_dict(const int *__restrict__ cols, const int2 *__restrict__ bounds,
                                                       int *__restrict__ dict, int *__restrict__ ndict,
                                                       unsigned short *__restrict__ idx16, int ratio, int dmax)
{
    __shared__ int keys[N];
    __shared__ int uniq[N];
    __shared__ int s_scan[kBlock];
    const int t = blockIdx.x, tid = threadIdx.x;
    const int n0 = bounds[t].y, nz = bounds[t + 1].y - n0;
    // Cache lines one gather instruction touches (64 consecutive entries, 16 doubles per 128-B
    // line), summed over the tile: first direct (nonzeros in CSR order, as the kernel stripes
    // them); a tile below 1 line per 2 nonzeros keeps direct gathers and skips the sort.
    constexpr int C = N / kBlock;
    int ld = 0;
    for (int c = 0; c < C; ++c) {
        const int i = tid * C + c;
        if (i < nz)
            ld += ((i & 63) == 0 || (cols[n0 + i] >> 4) != (cols[n0 + i - 1] >> 4)) ? 1 : 0;
    }
    s_scan[tid] = ld;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if (tid < off)
            s_scan[tid] += s_scan[tid + off];
        __syncthreads();
    }
    const int lines_direct = s_scan[0];
    // ratio >= 100 (MSPMV_SPMV_DICT=100, lab A/B): every tile takes its dictionary
    if (ratio == 0 || nz == 0 || (ratio > 0 && ratio < 100 && 2 * lines_direct < nz)) {
        if (tid == 0)
            ndict[t] = 0;
        return;
    }
    __syncthreads();
    for (int i = tid; i < N; i += kBlock)
        keys[i] = i < nz ? cols[n0 + i] : 0x7fffffff;
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N; i += kBlock) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const int a = keys[i], b = keys[ixj];
                    if ((a > b) == ((i & k) == 0)) {
                        keys[i] = b;
                        keys[ixj] = a;
                    }
                }
            }
            __syncthreads();
        }
    // distinct keys: thread tid scans its contiguous chunk [tid*C, (tid+1)*C)
    int cnt = 0;
    for (int c = 0; c < C; ++c) {
        const int i = tid * C + c;
        cnt += (i < nz && (i == 0 || keys[i] != keys[i - 1])) ? 1 : 0;
    }
    s_scan[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {  // inclusive Hillis-Steele scan
        const int v = tid >= off ? s_scan[tid - off] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    int pos = s_scan[tid] - cnt;
    for (int c = 0; c < C; ++c) {
        const int i = tid * C + c;
        if (i < nz && (i == 0 || keys[i] != keys[i - 1]))
            uniq[pos++] = keys[i];
    }
    const int nu = s_scan[kBlock - 1];
    __syncthreads();
    // ... then through the sorted dictionary.  The dictionary is taken only where direct gathers
    // are line-bound (>= 1 line per 2 nonzeros: scattered columns) and sorting saves >= 1/4 of
    // the lines; elsewhere (FEM blocks, stencils: ~0.2 lines per nonzero, served by L1/L2) its
    // LDS round trip measured a wash or a loss, and on random columns sorting saves nothing.
    int lu = 0;
    for (int c = 0; c < C; ++c) {
        const int i = tid * C + c;
        if (i < nu)
            lu += ((i & 63) == 0 || (uniq[i] >> 4) != (uniq[i - 1] >> 4)) ? 1 : 0;
    }
    s_scan[tid] = lu;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if (tid < off)
            s_scan[tid] += s_scan[tid + off];
        __syncthreads();
    }
    const int lines_dict = s_scan[0];
    const bool use = ratio >= 100 ? true : ratio > 0 ? 4 * lines_dict <= 3 * lines_direct : (nu <= dmax && 2 * nu <= nz);
    if (tid == 0)
        ndict[t] = use ? nu : 0;
    if (!use)
        return;
    for (int d = tid; d < nu; d += kBlock)
        dict[n0 + d] = uniq[d];
    for (int i = tid; i < nz; i += kBlock) {
        const int c = cols[n0 + i];
        int lo = 0, hi = nu - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (uniq[mid] < c)
                lo = mid + 1;
            else
                hi = mid;
        }
        idx16[n0 + i] = (unsigned short)lo;
    }
}

// ---- node blocks (plan time, single-RHS plans) --------------------------------------------
// FEM matrices store several unknowns per mesh node (pwtk: 6 DOF), and every row of a node lists
// the same columns.  A tile whose rows come in such runs -- consecutive rows whose column lists
// are prefixes of one list P (equal lists included; a row shortened by the matrix edge too) --
// stages them "column-owner" style: lane j reads P[j] once, gathers x[P[j]] once and multiplies
// it into every row of the run.  Only P's 16-bit column offsets cross HBM (1/h of the tile's
// column stream) and there is one gather per distinct (run, column) instead of one per nonzero.
// The products land in the same LDS slots as the striped staging writes, so the reduction --
// and every result bit -- is unchanged.
//
// Descriptor of one run chunk (16 B; at most kBlkMax per tile, tile t's at blk[t * stride ..], the
// plan's stride being the smallest of 8, 16, 32, 64 that holds every tile's set; the chunk's pattern
// columns sit once more in a 128-B slot of their own, k_fill_pcols, which is where the kernels read them):
//   x: vofs (nonzero offset of the run's first row in the tile, bits 0-15) | j0 (first pattern
//      column of this chunk, 16-23) | wc (chunk width <= 64, 24-31)
//   y: h (rows, 1..8, bits 0-3) | p (row holding P, 4-6) | nd (descriptor count, in entry 0 only,
//      8-15; 0 = the tile stages the plain way) | rofs (the run's first row in the tile, 16-31)
//   z, w: the h row lengths, 8 bits each (rows of a run are <= 255 long)
constexpr int kBlkMax = 64;  // descriptors a tile may have (the plan stores them at a stride of 8, 16, 32 or 64)
constexpr int kBlkRows = 8;
// (kBlkRunRows, mspmv_internal.h: rows per run)
// (kBlkTileChunks, mspmv_internal.h: the chunks of a tile the LDS-staged and column-owner paths of
// k_spmv_tile take -- one round of its four waves, more measured slower than striped staging; tiles
// of up to kBlkPlanChunks run only in the column-pair kernel, which loops over rounds.)

__device__ __forceinline__ int blk_len(const uint4 &d, int i)
{
    return (int)(((i < 4 ? d.z : d.w) >> (8 * (i & 3))) & 255u);
}

// One thread per tile.  A tile qualifies when it holds whole rows only (no split boundary), is on
// the 16-bit column stream, fits in kBlkMax chunks, and its runs pay (below).  (Runs tolerating one
// row with one extra pattern column -- imperfect FEM rows -- measured 24.1 vs 24.4 us on the pwtk
// shape with 1 % such rows, and cost the regular shape: not kept, r04e.)
__global__ void k_build_blocks(const int *__restrict__ row_offsets, const int *__restrict__ cols,
                               const int2 *__restrict__ bounds, const unsigned char *__restrict__ split,
                               const int *__restrict__ colbase, int num_tiles, uint4 *__restrict__ blk,
                               int max_chunks)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= num_tiles)
        return;
    uint4 *out = blk + (size_t)t * kBlkMax;
    out[0] = make_uint4(0, 0, 0, 0);  // entry 0 (with the count) is written last, on success only
    uint4 d0 = make_uint4(0, 0, 0, 0);
    const int2 b0 = bounds[t], b1 = bounds[t + 1];
    const int r0 = b0.x, r1 = b1.x, n0 = b0.y, n1 = b1.y;
    if (split[t] || split[t + 1] || colbase[t] < 0 || n1 <= n0 || row_offsets[r0] != n0 || row_offsets[r1] != n1)
        return;
    int nd = 0, sum_w = 0, nruns = 0;
    int r = r0;
    while (r < r1) {
        const int g = r, gs = row_offsets[g];
        int p = g, plen = row_offsets[g + 1] - gs;
        unsigned lens[2] = {0u, 0u};
        int h = 0;
        for (; r < r1 && h < kBlkRunRows; ++r, ++h) {
            const int s = row_offsets[r], len = row_offsets[r + 1] - s;
            if (len > 255)
                return;
            if (h > 0) {  // a prefix of P, or P a prefix of it
                const int ps = row_offsets[p], m = min(len, plen);
                bool same = true;
                for (int q = 0; q < m && same; ++q)
                    same = cols[s + q] == cols[ps + q];
                // a row that would widen a pattern of <= 64 columns past 64 starts a new run: the run
                // stays one chunk (a register run tile) -- spmv_runs_decide's host restatement relies on it
                if (!same || (len > 64 && plen <= 64))
                    break;
                if (len > plen) {
                    p = r;
                    plen = len;
                }
            }
            lens[h >> 2] |= (unsigned)len << (8 * (h & 3));
        }
        sum_w += plen;
        ++nruns;
        const int vofs = gs - n0;
        for (int j0 = 0; j0 < plen || (j0 == 0 && plen == 0); j0 += 64) {
            if (nd == kBlkMax || j0 > 255)
                return;
            const int wc = min(64, plen - j0);
            const uint4 dd = make_uint4((unsigned)vofs | ((unsigned)j0 << 16) | ((unsigned)wc << 24),
                                        (unsigned)h | ((unsigned)(p - g) << 4) | ((unsigned)(g - r0) << 16),
                                        lens[0], lens[1]);
            if (nd == 0)
                d0 = dd;
            else
                out[nd] = dd;
            ++nd;
            if (plen == 0)
                break;
        }
    }
    // Pays only when (measured, tools/lab/narrow_probe.py): runs share columns (pattern columns
    // <= 3/5 of the nonzeros: mean run height >= ~1.7), are wide (mean pattern >= 32 columns: a
    // run's value loads use one lane per column, against 64 per load in the striped staging), and
    // the 4 waves take the tile in ONE round of two chunks each (nd <= 8): a second round waits
    // for the first's sums.  2-D Kronecker FEM matrices with 3, 4 and 6 unknowns per node (15-30
    // columns, ~11-20 runs per tile) ran 3.1x, 2.0x and 1.2x slower on node blocks than striped;
    // the pwtk shape (53 columns, ~7 runs per tile) 1.14x faster.  (Shifted runs -- rows whose columns
    // are the previous row's plus one, the 27-point stencil's x-lines -- in a 16-lane column-pair form
    // measured slower than the striped staging on the nlpkkt120 size: 266-268 vs 220-224 us, r04d.)
    if (5 * sum_w > 3 * (n1 - n0) || sum_w < 32 * nruns || nd > max_chunks)
        return;
    d0.y |= (unsigned)nd << 8;
    out[0] = d0;
}

// Pattern-column slots (TilePlan::d_pcols), one wave per descriptor slot of the repacked plan: chunk
// di of tile t copies its wc offsets cols16[n0 + vofs + pstart + j0 ..] into its 128-B slot and repeats
// the last one up to 64.  Slots without a chunk (and chunks of no column) keep the caller's zeros.
__global__ __launch_bounds__(kBlock) void k_fill_pcols(const uint4 *__restrict__ blk, int stride,
                                                       const int2 *__restrict__ bounds,
                                                       const unsigned short *__restrict__ cols16, int num_tiles,
                                                       unsigned short *__restrict__ pcols)
{
    const long long slot = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int t = (int)(slot / stride), di = (int)(slot % stride);
    if (t >= num_tiles)
        return;
    const int nd = (int)((blk[(size_t)t * stride].y >> 8) & 255u);
    if (di >= nd)
        return;
    const uint4 d = blk[(size_t)t * stride + di];
    const int vofs = d.x & 0xffff, j0 = (d.x >> 16) & 255, wc = d.x >> 24;
    const int h = d.y & 15, p = (d.y >> 4) & 7;
    if (wc == 0)
        return;
    int pstart = 0;
    for (int i = 0; i < p && i < h; ++i)
        pstart += blk_len(d, i);
    pcols[(size_t)slot * 64 + lane] = cols16[(size_t)bounds[t].y + vofs + pstart + j0 + min(lane, wc - 1)];
}

// Node-block records (TilePlan::d_recs, layout at blk_rec_encode), one thread per descriptor slot of
// the repacked plan, after k_fill_pcols: a register run tile's chunk di puts its descriptor and the
// column-runs of its slot's pattern into record blk_rec_pos(di); its slots without a chunk take the
// tile's count alone.  Other tiles keep the caller's zeros.
__global__ __launch_bounds__(kBlock) void k_fill_recs(const uint4 *__restrict__ blk, int stride,
                                                      const unsigned short *__restrict__ pcols, int num_tiles,
                                                      unsigned *__restrict__ recs, int *__restrict__ counts)
{
    const long long slot = (long long)blockIdx.x * kBlock + threadIdx.x;
    const int t = (int)(slot / stride), di = (int)(slot % stride);
    if (t >= num_tiles)
        return;
    const uint4 *tb = blk + (size_t)t * stride;
    const int nd = (int)((tb[0].y >> 8) & 255u);
    bool reg = nd > 0;  // the kernel's former test: every chunk starts at pattern column 0
    for (int i = 0; i < nd; ++i)
        reg = reg && ((tb[i].x >> 16) & 255u) == 0;
    if (!reg)
        return;
    unsigned *out = recs + ((size_t)t * stride + blk_rec_pos(di)) * kRecDwords;
    if (di >= nd) {
        out[1] = (unsigned)nd << 8;
        return;
    }
    const uint4 d = tb[di];
    unsigned ent[kRecEntries];
    const bool fits = blk_rec_encode(pcols + (size_t)slot * 64, (int)(d.x >> 24), ent);
    atomicAdd(&counts[fits ? 0 : 1], 1);
    out[0] = d.x;
    out[1] = (d.y & ~0xff80u) | ((unsigned)nd << 8) | (fits ? 0u : kRecEscape);
    out[2] = d.z;
    out[3] = d.w;
    for (int e = 0; e < kRecEntries; ++e)
        out[4 + e] = ent[e];
}

// Per-tile choice of the in-tile reduction (one thread per tile, at plan time; gl = lanes per
// nonzero: 1 for SpMV, L/2 column-pair lanes for SpMM).  The tile's row segments -- its complete rows plus the trailing partial row of a
// split boundary -- are either summed by row groups of G = 2^lg lanes (mode lg + 1) or, when
// segment lengths are too uneven for that, by the per-thread merge walk (mode 0).  Cost model
// in latency steps of the slowest group: ceil(segments / groups) rounds of the longest
// segment's reads (SpMV: ceil(longest / G) LDS reads; SpMM: gather batches) plus the shuffle
// fold; the cheapest G wins if its cost is within max_cost (about the walk it replaces: IPT
// reads plus an 11-step search and two barriers for SpMV, IPTG/4 gather chunks for SpMM).
__global__ void k_tile_modes(const int *__restrict__ row_offsets, const int2 *__restrict__ bounds,
                             const unsigned char *__restrict__ split, int num_tiles, int gl, int max_cost,
                             int lanes, unsigned char *__restrict__ modes)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= num_tiles)
        return;
    const int2 b0 = bounds[t], b1 = bounds[t + 1];
    const int nrows = b1.x - b0.x;
    const bool tail = split[t + 1] != 0;
    const int nseg = nrows + (tail ? 1 : 0);
    int longest = 0, prev = b0.y;
    for (int r = 0; r < nrows; ++r) {
        const int e = row_offsets[b0.x + 1 + r];
        longest = max(longest, e - prev);
        prev = e;
    }
    if (tail)
        longest = max(longest, b1.y - prev);
    int best = 0, best_cost = max_cost + 1;
    for (int lg = 0; (gl << lg) <= 64; ++lg) {  // a row group stays inside one wave
        const int groups = lanes / (gl << lg), G = 1 << lg;
        const int rounds = (nseg + groups - 1) / groups;
        const int per_lane = (longest + G - 1) / G;
        // SpMV: LDS product reads, one step each, plus a 3-step shuffle per fold level.
        // SpMM: panel-row gathers in batches of 8 (about 4 steps of latency per batch).
        const int cost = gl == 1 ? rounds * (per_lane + 3 * lg) : rounds * (4 * ((per_lane + 7) / 8) + lg);
        if (cost < best_cost) {
            best_cost = cost;
            best = lg + 1;
        }
    }
    modes[t] = best_cost <= max_cost ? (unsigned char)best : (unsigned char)0;
}

// ------------------------------------------------------------------------------------------
// tile kernels
// ------------------------------------------------------------------------------------------
struct TileArgs {
    const int *__restrict__ row_offsets;
    const int *__restrict__ cols;
    const double *__restrict__ vals;
    const double *__restrict__ x;      // SpMV/SpMM: x / X.   CG: {r, p_old} interleaved (cg_rp)
    const double *__restrict__ xr;     // MODE 2: the rows' own x (row R at xr[R * ld]) for x.(Ax) --
                                       // x itself unless the handle is a row range of x's rows
    const double *__restrict__ p_old;  // (unused by the single-RHS CG: p_old rides with r in x)
    double *__restrict__ xsol;         // CG (MODE 1): the solution; iteration k applies x += alpha_{k-1} p_{k-1}
                                       // to the tile's rows (cg1_lag_*)
    double *__restrict__ p_new;        // CG: the {r, p} buffer of the next iteration; p = r + beta p_old
                                       // is written for the tile's rows at p_new[2 R + 1] (cg_pstore)
    double *__restrict__ y;            // SpMV/SpMM: y / Y.   CG: Ap
    const int2 *__restrict__ bounds;
    const unsigned char *__restrict__ split;
    const unsigned char *__restrict__ rmode;  // per-tile in-tile reduction (k_tile_modes)
    double *__restrict__ carry_val;    // [tile][L] split-row partials, agent-scope stores (close_split_rows)
    const int4 *fix;                   // TilePlan::d_fix / d_fix_cnt (null: the plan splits no row)
    unsigned *fix_cnt;
    unsigned *fault;                   // where a ticket overrun is raised (ticket_arrive): the CG's control word,
                                       // else the handle's fault word (mspmv_check_faults)
    double *head_val;                  // [tile][L]: the first row of a tile that completes a split row
    double *head_pub;                  // [tile][L]: the same, republished with agent scope (close_split_rows)
    double *y0;                        // per tile (set by the kernel): where row 0 of the tile goes --
                                       // y's row, or head_val when the tile completes a split row
    int num_tiles;
    CgScalars *scal;                   // CG: per-column scalars
    CgControl *ctrl;                   // CG: iteration control
    const unsigned char *conv;         // CG: per-column converged flags
    double *partials;                  // CG: per-slot partial dots [slot][L], then level 2 [group][L]
    unsigned *gtickets;                // CG: per-group tickets of reduce_slots (self-resetting)
    double *dot_out;                   // MODE 2: the reduced x.(Ax) per column [L]
    int m;                             // rows (row_offsets holds m + 1 entries)
    // MODE 1 (single-RHS pipelined CG): the previous update's r.r partials (summed by every
    // workgroup), the iteration parity, the stop test and the residual history
    const double *part_in;
    int n_part_in;
    int parity;
    double tol;
    double *hist;
    int hist_cap;
    // single-RHS plans: per-tile 16-bit column offsets (TilePlan::d_colbase / d_cols16; null: off)
    const int *colbase;
    const unsigned short *cols16;
    // single-RHS plans with node blocks (TilePlan::d_blk, k_build_blocks; null: off); all_reg:
    // every tile reduces in registers (host side: launch k_spmv_blk)
    const uint4 *blk;
    int blk_stride;
    int all_reg;
    // ... the chunks' pattern columns, one 128-B slot per descriptor slot (TilePlan::d_pcols)
    const unsigned short *pcols;
    // ... descriptor and pattern as one 64-B record per descriptor slot (TilePlan::d_recs)
    const unsigned *recs;
    // single-RHS plans with column dictionaries (TilePlan::d_dict; null: off)
    const int *dict;
    const int *ndict;
    const unsigned short *idx16;
    // SpMM: leading dimension of the x / y panels in doubles (L for whole panels; a column
    // chunk of a wider panel otherwise, mspmv_dspmm with L outside {1, 2, 4, 8, 16})
    int ld;
    // single-RHS tile kernel: load the tile's row ends with its stream (1) instead of after the
    // staging (0) -- one dependent round trip fewer per tile (SpmvTuning::early_re)
    int early_re;
    int blk_rows_max;  // node-block plans: the tallest run (TilePlan::blk_rows_max; k_spmm_blk's KR)
    unsigned long long *stamps;  // k_spmv_tile STAMP (diagnostic): [tile][kTileStamps]
    int tb;            // threads sharing one tile (the plan's lanes: 256, or 64 for one-wave SpMV plans)
    int blk_spmv;      // the plain SpMV runs k_spmv_blk on this plan (TilePlan::blk_spmv; mixed plans too)
    int n;             // columns (x holds n entries)
};

// Tile-kernel modes.
//   0: y = A x.
//   1: fused CG step: gather p = r + beta p_old, Ap = A p, write p for the tile's rows,
//      p.Ap by linearity, last block sets alpha (single GPU).
//   2: y = A x plus x.y over the rows (by linearity), last block writes dot_out (the
//      row-sharded CG, whose x = [p_own | p_halo] was updated and exchanged beforehand).
enum : int { kModeSpmv = 0, kModeCg = 1, kModeDot = 2 };

// Single-RHS pipelined CG keeps r and p interleaved, {r_i, p_i} per row (16 B): the fused
// p = r + beta p_old gather at every nonzero's column is one 16-B load instead of two 8-B loads
// on separate cache lines (the same operands, so the same rounding).  Two such buffers
// alternate by iteration parity: the SpMV reads {r_k, p_{k-1}} and writes p_k into the other
// one, the update reads r_k here and p_k there and writes r_{k+1} next to p_k.
__device__ __forceinline__ double2 cg_rp(const TileArgs &a, long long i)
{
    return reinterpret_cast<const double2 *>(a.x)[i];
}
__device__ __forceinline__ void cg_pstore(const TileArgs &a, long long i, double p) { a.p_new[2 * i + 1] = p; }

// LDS slot of tile-local product k: an XOR swizzle inside each aligned group of 8 doubles,
// so walkers 8 products apart hit different banks, while staging writes and row-group reads
// (consecutive k) stay conflict-free -- no padding, so the tile fits a smaller LDS footprint.
__device__ __forceinline__ int pslot(int k) { return k ^ ((k >> 3) & 7); }

// Stage products val*x[col] (or val*(r + beta p)[col] for CG) of the tile's nonzeros
// [n0, n0+nnzt) into LDS.  Striped: lane l of round j takes nonzero l + 256 j, so each
// gather instruction reads x at 64 CONSECUTIVE nonzeros' columns (runs of neighbouring
// columns share cache lines) -- measured 1.4x faster than 16-byte-per-lane blocked loads,
// whose gathers scatter over 4x more lines.  Every round's loads and gathers are issued
// before any is consumed (indices past the tile clamp to its last nonzero).
// Barrier over the threads that share a tile: the workgroup, or (one-wave workgroups) the wave,
// whose LDS accesses retire in order -- only compiler reordering has to be fenced.
template <int TB>
__device__ __forceinline__ void tile_sync()
{
    if (TB == 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

template <int NJ, bool CG>
struct StageRegs {
    int c[NJ];
    double v[NJ];
    double xv[NJ];
    double pv[CG ? NJ : 1];
};
template <int NJ, bool CG, bool NT, int TB = kBlock>
__device__ __forceinline__ void stage_issue(const TileArgs &a, int n0, int nnzt, int colbase, StageRegs<NJ, CG> &st)
{
    if (colbase >= 0) {  // block-uniform: the tile's 16-bit column offsets
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            st.c[j] = colbase + (int)ld_stream<NT>(a.cols16 + n0 + min((int)threadIdx.x + j * TB, nnzt - 1));
    } else {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            st.c[j] = ld_stream<NT>(a.cols + n0 + min((int)threadIdx.x + j * TB, nnzt - 1));
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        st.v[j] = ld_stream<NT>(a.vals + n0 + min((int)threadIdx.x + j * TB, nnzt - 1));
    if constexpr (CG) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const double2 v = cg_rp(a, st.c[j]);
            st.xv[j] = v.x;
            st.pv[j] = v.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            st.xv[j] = a.x[st.c[j]];
    }
}
template <int NJ, bool CG, int TB = kBlock>
__device__ __forceinline__ void stage_store(const StageRegs<NJ, CG> &st, int nnzt, double beta, double *s_prod)
{
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = (int)threadIdx.x + j * TB;
        double x = st.xv[j];
        if (CG)
            x = x + beta * st.pv[j];
        if (k < nnzt)
            s_prod[pslot(k)] = st.v[j] * x;
    }
}
// Grouped staging (plain SpMV on the 16-bit stream, W = 2: pairs):
// thread tid takes the ABSOLUTE nonzero groups q0 + tid + TB u of W consecutive nonzeros (q0 =
// n0 / W), each one aligned W*8-B value load (W/2 16-B loads) and one aligned W*2-B column load --
// 2/W of the striped form's column loads and 1/2 of its value loads for the same bytes (the stream
// instructions, not its bytes, are what the tile kernel spends here: the nlpkkt120-size SpMV ran
// 5 % faster with pairs, r03q).  Elements of a group outside the tile gather x[colbase] (always a
// valid column) and are not stored.  A tile with a group more than NP * TB (a start off the
// W-grid at the nominal size) issues one extra round (block-uniform).
// Measured and not kept (r03af, r03r): quads (W = 4) 245 vs 223 us and one 16-B x load per
// consecutive pair 261 vs 220 us at the nlpkkt120 size.
constexpr int kGroupW = 2;
typedef unsigned v2u_t __attribute__((ext_vector_type(2)));
template <int NP, int W>
struct GroupRegs {
    unsigned c[NP][W / 2];  // two 16-bit column offsets per word
    double2 v[NP][W / 2];
    double x[NP][W];
};
template <int NP, int W, bool NT, int TB>
__device__ __forceinline__ void group_issue(const TileArgs &a, int n0, int nnzt, int colbase, int ubase,
                                            GroupRegs<NP, W> &st)
{
    const int q0 = n0 / W, qlast = (n0 + nnzt - 1) / W;
    const double2 *v2 = reinterpret_cast<const double2 *>(a.vals);
#pragma unroll
    for (int u = 0; u < NP; ++u) {
        const int q = min(q0 + (int)threadIdx.x + TB * (ubase + u), qlast);
        if constexpr (W == 2) {
            st.c[u][0] = ld_stream<NT>(reinterpret_cast<const unsigned *>(a.cols16) + q);
        } else {
            const v2u_t *c4 = reinterpret_cast<const v2u_t *>(a.cols16);
            const v2u_t cc = NT ? __builtin_nontemporal_load(c4 + q) : c4[q];
            st.c[u][0] = cc.x;
            st.c[u][1] = cc.y;
        }
#pragma unroll
        for (int h = 0; h < W / 2; ++h)
            st.v[u][h] = ld_stream<NT>(v2 + (size_t)q * (W / 2) + h);
    }
#pragma unroll
    for (int u = 0; u < NP; ++u) {
        const int q = min(q0 + (int)threadIdx.x + TB * (ubase + u), qlast);
        const int k0 = W * q - n0;
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const int off = (int)((st.c[u][e >> 1] >> (16 * (e & 1))) & 0xffffu);
            const bool in = k0 + e >= 0 && k0 + e < nnzt;
            st.x[u][e] = a.x[colbase + (in ? off : 0)];
        }
    }
}
template <int NP, int W, int TB>
__device__ __forceinline__ void group_store(const GroupRegs<NP, W> &st, int n0, int nnzt, int ubase, double *s_prod)
{
    const int q0 = n0 / W, qlast = (n0 + nnzt - 1) / W;
#pragma unroll
    for (int u = 0; u < NP; ++u) {
        const int q = q0 + (int)threadIdx.x + TB * (ubase + u);
        if (q > qlast)
            continue;
        const int k0 = W * q - n0;
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const double v = (e & 1) ? st.v[u][e >> 1].y : st.v[u][e >> 1].x;
            if (k0 + e >= 0 && k0 + e < nnzt)
                s_prod[pslot(k0 + e)] = v * st.x[u][e];
        }
    }
}

template <int NJ, bool CG, bool NT>
__device__ __forceinline__ void stage_products(const TileArgs &a, int n0, int nnzt, double beta, double *s_prod)
{
    StageRegs<NJ, CG> st;
    stage_issue<NJ, CG, NT>(a, n0, nnzt, -1, st);
    stage_store<NJ, CG>(st, nnzt, beta, s_prod);
}

// Dictionary staging (plain SpMV, plans built with MSPMV_SPMV_DICT=1): the tile's distinct
// columns are gathered once each (DJ per thread in flight, clamped), parked in LDS, and every
// nonzero's product reads its x there through its 16-bit dictionary position.  The products are
// the same values as the direct path (val * x[col]), so results are bit-identical to it.
template <int NJ, bool NT, int TB>
__device__ __forceinline__ void dict_stage(const TileArgs &a, double *s_prod, int nd, int n0, int nnzt)
{
    constexpr int DJ = 3;
    const int tid = threadIdx.x;
    int ix[NJ];
    double v[NJ];
    int dc[DJ];
    double dx[DJ];
#pragma unroll
    for (int u = 0; u < DJ; ++u)
        dc[u] = ld_stream<NT>(a.dict + n0 + min(tid + u * TB, nd - 1));
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        ix[j] = ld_stream<NT>(a.idx16 + n0 + min(tid + j * TB, nnzt - 1));
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        v[j] = ld_stream<NT>(a.vals + n0 + min(tid + j * TB, nnzt - 1));
#pragma unroll
    for (int u = 0; u < DJ; ++u)
        dx[u] = a.x[dc[u]];
    double *s_x = s_prod;  // nd <= nnzt: the dictionary's x fits the product slots
#pragma unroll
    for (int u = 0; u < DJ; ++u)
        if (tid + u * TB < nd)
            s_x[tid + u * TB] = dx[u];
    for (int d = tid + DJ * TB; d < nd; d += TB)  // rare: > DJ * TB distinct columns
        s_x[d] = a.x[a.dict[n0 + d]];
    tile_sync<TB>();
    double pr[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        pr[j] = v[j] * s_x[ix[j]];
    tile_sync<TB>();
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = tid + j * TB;
        if (k < nnzt)
            s_prod[pslot(k)] = pr[j];
    }
}

// Node-block staging (k_build_blocks): wave w takes the tile's run chunks w, w + 4, ..., two per
// round.  Per chunk, lane l owns pattern column j = j0 + l: one 16-bit column offset of row P,
// one gather (x, or CG's {r, p}), and the values of that column in every row of the run that is
// long enough -- all of a round's loads issued before any is consumed.  The products
// val * x[col] (CG: val * (r + beta p)) go to the tile's usual LDS slots.  `head` runs once
// between the first round's loads and its products (CG: stop test + beta, as the striped path).
template <bool CG>
struct BlkRegs {
    int c[2];
    double v[2][kBlkRows];
    double xv[2];
    double pv[CG ? 2 : 1];
};

__device__ __forceinline__ uint4 blk_read(const uint4 &bd, int di)
{
    return make_uint4((unsigned)__builtin_amdgcn_readlane((int)bd.x, di),
                      (unsigned)__builtin_amdgcn_readlane((int)bd.y, di),
                      (unsigned)__builtin_amdgcn_readlane((int)bd.z, di),
                      (unsigned)__builtin_amdgcn_readlane((int)bd.w, di));
}

// Chunk di of tile t: its slot of pattern columns (TileArgs::pcols; position l is pattern column
// j0 + l).  The address needs neither the tile's bounds nor the descriptor.
__device__ __forceinline__ const unsigned short *blk_slot(const TileArgs &a, int t, int di)
{
    return a.pcols + ((size_t)t * a.blk_stride + di) * 64;
}

template <bool CG, bool NT, int TB, typename Head>
__device__ __forceinline__ void blk_stage(const TileArgs &a, int t, const uint4 &bd, int nd, int n0, int colbase,
                                          double *s_prod, double &beta, Head &&head)
{
    constexpr int NW = TB / 64;  // waves sharing the tile
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int round = 0; round * 2 * NW < nd; ++round) {
        BlkRegs<CG> st;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int di = wave + NW * (2 * round + s);
            st.c[s] = 0;
#pragma unroll
            for (int i = 0; i < kBlkRows; ++i)
                st.v[s][i] = 0.0;
            if (di < nd) {  // wave-uniform
                const uint4 d = blk_read(bd, di);
                const int vofs = d.x & 0xffff, j0 = (d.x >> 16) & 255, wc = d.x >> 24;
                const int h = d.y & 15;
                const int j = j0 + lane;
                int start = 0;
#pragma unroll
                for (int i = 0; i < kBlkRows; ++i) {
                    const int len = blk_len(d, i);
                    if (i < h && j < len)
                        st.v[s][i] = ld_stream<NT>(a.vals + n0 + vofs + start + j);
                    start += i < h ? len : 0;
                }
                if (lane < wc)
                    st.c[s] = colbase + (int)ld_stream<NT>(blk_slot(a, t, di) + lane);
            }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if constexpr (CG) {
                const double2 v = cg_rp(a, st.c[s]);
                st.xv[s] = v.x;
                st.pv[s] = v.y;
            } else {
                st.xv[s] = a.x[st.c[s]];
            }
        }
        if (round == 0 && !head())
            return;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int di = wave + NW * (2 * round + s);
            if (di < nd) {
                const uint4 d = blk_read(bd, di);
                const int vofs = d.x & 0xffff, j0 = (d.x >> 16) & 255;
                const int h = d.y & 15;
                const int j = j0 + lane;
                double x = st.xv[s];
                if (CG)
                    x = x + beta * st.pv[s];
                int start = 0;
#pragma unroll
                for (int i = 0; i < kBlkRows; ++i) {
                    const int len = blk_len(d, i);
                    if (i < h && j < len)
                        s_prod[pslot(vofs + start + j)] = st.v[s][i] * x;
                    start += i < h ? len : 0;
                }
            }
        }
    }
}

// Sum of 8 per-lane values over the wave by a reduce-scatter butterfly (xor 32, 16, 8 halve the
// values each lane carries, then xor 4, 2, 1 finish): lanes 8i .. 8i+7 end up holding row i's
// total (i = lane >> 3).  10 double shuffles for 8 sums instead of 48 for 8 full butterflies;
// the order is fixed, so results are bit-for-bit reproducible.
__device__ __forceinline__ double rows8_sum(const double (&p)[kBlkRows])
{
    const int lane = threadIdx.x & 63;
    const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
    double q4[4], q2[2];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        q4[k] = (b5 ? p[k + 4] : p[k]) + __shfl_xor(b5 ? p[k] : p[k + 4], 32);
#pragma unroll
    for (int k = 0; k < 2; ++k)
        q2[k] = (b4 ? q4[k + 2] : q4[k]) + __shfl_xor(b4 ? q4[k] : q4[k + 2], 16);
    double v = (b3 ? q2[1] : q2[0]) + __shfl_xor(b3 ? q2[0] : q2[1], 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

// rows8_sum over the 32 lanes of a half-wave: row i's total lands in lanes 4i .. 4i + 3 of the
// half (i = (lane & 31) >> 2).  Shuffles with xor <= 16 never cross the halves, so the two halves
// fold two different runs with the same 10 shuffles.
__device__ __forceinline__ double rows8_sum32(const double (&p)[kBlkRows])
{
    const int lane = threadIdx.x & 63;
    const bool b4 = lane & 16, b3 = lane & 8, b2 = lane & 4;
    double q4[4], q2[2];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        q4[k] = (b4 ? p[k + 4] : p[k]) + __shfl_xor(b4 ? p[k] : p[k + 4], 16);
#pragma unroll
    for (int k = 0; k < 2; ++k)
        q2[k] = (b3 ? q4[k + 2] : q4[k]) + __shfl_xor(b3 ? q4[k] : q4[k + 2], 8);
    double v = (b2 ? q2[1] : q2[0]) + __shfl_xor(b2 ? q2[0] : q2[1], 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

// The half-wave's record of a round (TilePlan::d_recs): lane l of each half loads dword l & 15 of the
// record of the half's run slot, ONE 4-B load and one 64-B half line per half, the two halves of a
// wave sharing a line (blk_rec_pos).  Unconditional: every slot of a tile exists (di < blk_stride, a
// multiple of the 8 run slots of a round), and its address takes only t and the lane, so the load
// goes out with the tile's header and IS its descriptor.
template <bool NT>
__device__ __forceinline__ unsigned blk_pair_rec(const TileArgs &a, int t, int round)
{
    const int lane = threadIdx.x & 63;
    const int slot = 8 * round + 2 * (int)(threadIdx.x >> 6) + (lane >> 5);  // blk_rec_pos(wave + 4 (2 round + half))
    return ld_stream<NT>(a.recs + ((size_t)t * a.blk_stride + slot) * kRecDwords + (lane & 15));
}

// Plain SpMV form of blk_rows with column PAIRS: each half-wave owns one run per round and its lane
// l owns pattern columns 2l and 2l + 1, so a row of the run arrives in ONE 16-B load per lane (half
// the value-load instructions of column-owner lanes; the loads may be 8-B aligned only -- gfx9's
// unaligned access mode), and one rows8_sum32 folds both halves' runs (half the shuffles).  A
// lane's two products are added before the half-wave tree: a fixed order, so rows stay
// reproducible and within the reordering bound (mode 255).  Column-owner lanes instead: pwtk shape
// 24.98 vs 22.6-23.1 us (r03t).  Pattern columns in consecutive pairs take ONE 16-B x load per lane.
// Descriptor and pattern columns come from the half's record (rec, blk_pair_rec) by cross-lane
// reads inside the half; nd is the tile's count, which every record carries.
template <bool NT, int KR>
__device__ __forceinline__ void blk_rows_pair(const TileArgs &a, int t, unsigned rec, int nd, int r0, int n0,
                                              int colbase)
{
    constexpr int NW = kBlock / 64;
    const int lane = threadIdx.x & 63;
    const int half = lane >> 5, hl = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int round = 0; round * 2 * NW < nd; ++round) {
        if (round > 0)  // round 0's came with the header
            rec = blk_pair_rec<NT>(a, t, round);
        const int di = wave + NW * (2 * round + half);
        const bool valid = di < nd;  // else the record holds the count alone: no row, no column-run
        auto dword = [&](int k) { return (unsigned)__shfl((int)rec, (lane & 32) + k); };
        const uint4 d = make_uint4(dword(0), dword(1), dword(2), dword(3));
        const int vofs = d.x & 0xffff, wc = d.x >> 24;
        const int h = d.y & 15, rofs = d.y >> 16;
        double2 v[KR];
        bool in0[KR], in1[KR];
        int start = 0;
#pragma unroll
        for (int i = 0; i < KR; ++i) {
            const int len = blk_len(d, i);
            in0[i] = valid && i < h && 2 * hl < len;
            in1[i] = valid && i < h && 2 * hl + 1 < len;
            v[i] = make_double2(0.0, 0.0);
            if (in0[i])
                v[i] = ld_stream<NT>(reinterpret_cast<const double2 *>(a.vals + n0 + vofs + start + 2 * hl));
            start += i < h ? len : 0;
        }
        // the lane's two pattern columns, positions 2 hl and 2 hl + 1 of the record's column-runs
        // (positions past the chunk repeat its last column, a record without a chunk gives the tile's
        // column base): the second is the first plus one unless it opens the next column-run.  Then
        // ONE 16-B x load (8-B aligned at worst) for an adjacent pair -- FEM nodes list their
        // unknowns consecutively, so nearly every lane's pair is -- and a second load only in lanes
        // whose pair is not (an exec-masked load, skipped when no lane needs it).
        // The load starts at n - 2 at most and picks its half (the last column sits at n - 1 at most).
        const int q = max(min(2 * hl, wc - 1), 0);
        int e;
        const unsigned E = blk_rec_find([&](int i) { return dword(4 + i); }, q, e);
        const unsigned En = dword(4 + min(e + 1, kRecEntries - 1));
        int c0 = colbase + (int)((E & 0xffffu) + (unsigned)q - (E >> 24));
        int c1 = c0 + 1;
        if (2 * hl + 1 < wc && 2 * hl + 1 == (int)((E >> 24) + ((E >> 16) & 255u)))
            c1 = colbase + (int)(En & 0xffffu);
        if (d.y & kRecEscape) {
            // more column-runs than a record holds: both 16-bit offsets in ONE 4-B load from the
            // pattern row in cols16 (2-B aligned at worst; the second belongs to the next position,
            // in bounds by the stream's padding, and is replaced when the lane has one column)
            const int p = (d.y >> 4) & 7;
            int pstart = 0;
#pragma unroll
            for (int i = 0; i < KR - 1; ++i)
                pstart += i < p ? blk_len(d, i) : 0;
            unsigned cc = 0u;
            if (2 * hl < wc)
                cc = ld_stream<NT>(reinterpret_cast<const unsigned *>(a.cols16 + n0 + vofs + pstart + 2 * hl));
            c0 = colbase + (int)(cc & 0xffffu);
            c1 = 2 * hl + 1 < wc ? colbase + (int)(cc >> 16) : c0 + 1;
        }
        const int base = min(c0, a.n - 2);
        const double2 xx = *reinterpret_cast<const double2 *>(a.x + base);
        const double x0 = base == c0 ? xx.x : xx.y;
        double x1 = xx.y;  // c1 == c0 + 1 <= n - 1: base == c0
        if (c1 != c0 + 1)
            x1 = a.x[c1];
        double pr[kBlkRows];
#pragma unroll
        for (int i = 0; i < kBlkRows; ++i)
            pr[i] = i < KR ? (in0[i] ? v[i].x * x0 : 0.0) + (in1[i] ? v[i].y * x1 : 0.0) : 0.0;
        const double sum = rows8_sum32(pr);
        const int myrow = hl >> 2;
        if (valid && (hl & 3) == 0 && myrow < h)
            a.y[r0 + rofs + myrow] = sum;
    }
}

// Node-block tiles whose runs are at most 64 columns wide (one chunk each: FEM node rows) skip
// LDS altogether: lane j of the run's wave holds the products of pattern column j in every row
// of the run, rows8_sum folds them across the wave, and lane 8i stores row i (y; CG: p for the
// row, p.Ap; dot mode: x.(Ax)).  No row-end staging, no barrier, no LDS round trip -- the
// tile's life is its loads plus a few shuffles.  Rows are summed by a fixed lane tree, so they
// are reproducible and within 2 (len+1) eps (|A||x|)_i of the sequential CSR-order sum
// (mspmv_tile_modes reports these tiles as 255).
template <int MODE, bool NT, int TB, typename Head>
__device__ __forceinline__ void blk_rows(const TileArgs &a, int t, const uint4 &bd, int nd, int r0, int n0,
                                         int colbase, double &beta, double &dot, Head &&head)
{
    constexpr bool CG = MODE == kModeCg;
    constexpr int NW = TB / 64;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int myrow = lane >> 3;  // the run row this lane stores (lanes 8i)
    for (int round = 0; round * 2 * NW < nd; ++round) {
        BlkRegs<CG> st;
        double2 ro[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int di = wave + NW * (2 * round + s);
            st.c[s] = 0;
            ro[s] = make_double2(0.0, 0.0);
#pragma unroll
            for (int i = 0; i < kBlkRows; ++i)
                st.v[s][i] = 0.0;
            if (di < nd) {  // wave-uniform
                const uint4 d = blk_read(bd, di);
                const int vofs = d.x & 0xffff, wc = d.x >> 24;
                const int h = d.y & 15, rofs = d.y >> 16;
                int start = 0;
#pragma unroll
                for (int i = 0; i < kBlkRows; ++i) {
                    const int len = blk_len(d, i);
                    if (i < h && lane < len)
                        st.v[s][i] = ld_stream<NT>(a.vals + n0 + vofs + start + lane);
                    start += i < h ? len : 0;
                }
                if (lane < wc)
                    st.c[s] = colbase + (int)ld_stream<NT>(blk_slot(a, t, di) + lane);
                if (MODE != kModeSpmv && (lane & 7) == 0 && myrow < h) {
                    const int R = r0 + rofs + myrow;
                    if constexpr (CG)
                        ro[s] = cg_rp(a, R);
                    else
                        ro[s].x = a.xr[R];
                }
            }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if constexpr (CG) {
                const double2 v = cg_rp(a, st.c[s]);
                st.xv[s] = v.x;
                st.pv[s] = v.y;
            } else {
                st.xv[s] = a.x[st.c[s]];
            }
        }
        if (round == 0 && !head())
            return;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int di = wave + NW * (2 * round + s);
            if (di < nd) {
                const uint4 d = blk_read(bd, di);
                const int h = d.y & 15, rofs = d.y >> 16;
                double x = st.xv[s];
                if (CG)
                    x = x + beta * st.pv[s];
                double pr[kBlkRows];
#pragma unroll
                for (int i = 0; i < kBlkRows; ++i)
                    pr[i] = (i < h && lane < blk_len(d, i)) ? st.v[s][i] * x : 0.0;
                const double sum = rows8_sum(pr);
                if ((lane & 7) == 0 && myrow < h) {
                    const int R = r0 + rofs + myrow;
                    a.y[R] = sum;
                    if constexpr (CG) {
                        const double pn = ro[s].x + beta * ro[s].y;
                        cg_pstore(a, R, pn);
                        dot += pn * sum;
                    } else if constexpr (MODE == kModeDot) {
                        dot += ro[s].x * sum;
                    }
                }
            }
        }
    }
}

// Per-tile LDS of the single-RHS kernels.  Products and row ends share one buffer: a tile
// holds nrows + nnzt <= MAXI items, so the nnzt products (slots [0, nnzt) rounded up to the
// swizzle group) followed by the nrows int row ends always fit in MAXI + 8 doubles.
template <int IPT, int TB = kBlock>
struct SpmvSmem {
    static constexpr int TILE = TB * IPT;
    static constexpr int MAXI = TILE + TILE / kSnapDiv;
    static constexpr int MAXJ = (MAXI + TB - 1) / TB;
    double prod[MAXI + 8];
    double red[TB / 64];
    int last;
    __device__ __forceinline__ int *rowend(int nnzt) { return reinterpret_cast<int *>(prod + ((nnzt + 7) & ~7)); }
    // Once a tile's walk has consumed its products and row ends, the walkers' closing pass
    // (row ends reached, carries) reuses the front of prod as scratch: no separate arrays, so a
    // workgroup's LDS is the product buffer alone (18.5 KB at IPT = 8: 8 workgroups per CU).
    __device__ __forceinline__ double *scratch_val() { return prod; }
    __device__ __forceinline__ int *scratch_row() { return reinterpret_cast<int *>(prod + TB); }
    static_assert(MAXI + 8 >= TB + TB / 2, "scratch must fit the product buffer");
};

// Everything after staging, for one tile whose products and row ends are in LDS: one merge
// search per walker, the register walk, in-tile carries, the cross-tile carry, the row
// stores and (CG) the p.Ap contribution.  Called uniformly by all 256 threads; ends with the
// LDS free for the next tile.
template <int IPT, int MODE, int TB = kBlock, bool FIX = true>
__device__ __forceinline__ void walk_tile(const TileArgs &a, SpmvSmem<IPT, TB> &sm, int t, int r0, int n0, int nrows,
                                          int nnzt, bool tail, double beta, double &dot)
{
    constexpr int MAXJ = SpmvSmem<IPT, TB>::MAXJ;
    const int tid = threadIdx.x;
    const int *rend = sm.rowend(nnzt);
    const int items = nrows + nnzt;
    const int ipt = (items + TB - 1) / TB;
    const int d0 = min(tid * ipt, items);
    int cx, cy, ex = nrows, ey = nnzt;
    lds_search(d0, rend, nrows, nnzt, cx, cy);
    // The walker's end is the next walker's start: searched here too (no LDS exchange, so the
    // workgroup needs no scratch arrays beside the product buffer).
    if (tid + 1 < TB)
        lds_search(min(d0 + ipt, items), rend, nrows, nnzt, ex, ey);
    // Does this thread's first row hold nonzeros that earlier threads of the tile consumed?
    const bool need_cin = (cx < ex) && (cy > (cx == 0 ? 0 : rend[cx - 1]));
    // This walker's products, read from LDS up front (independent reads, no dependent chain).
    double pr[MAXJ];
    if (ey > cy) {
#pragma unroll
        for (int j = 0; j < MAXJ; ++j)
            pr[j] = sm.prod[pslot(min(cy + j, ey - 1))];
    }
    auto write_row = [&](int row, double val) {
        const int R = r0 + row;
        *(FIX && row == 0 ? a.y0 : &a.y[R]) = val;
        if (MODE == kModeCg) {
            const double2 v = cg_rp(a, R);
            const double pn = v.x + beta * v.y;
            cg_pstore(a, R, pn);
            dot += pn * val;
        } else if (MODE == kModeDot) {
            dot += a.xr[R] * val;
        }
    };
    double run = 0.0;
    bool first = true, pend = false;
    int prow = 0;
    double pval = 0.0;
    int next_end = cx < ex ? rend[cx] : 0x7fffffff;  // end of the row being accumulated
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const int k = cy + j;
        if (k < ey) {
            while (next_end <= k) {
                if (first && need_cin) {
                    pend = true;
                    prow = cx;
                    pval = run;
                } else {
                    write_row(cx, run);
                }
                first = false;
                run = 0.0;
                ++cx;
                next_end = cx < ex ? rend[cx] : 0x7fffffff;
            }
            run += pr[j];
        }
    }
    while (cx < ex) {
        if (first && need_cin) {
            pend = true;
            prow = cx;
            pval = run;
        } else {
            write_row(cx, run);
        }
        first = false;
        run = 0.0;
        ++cx;
    }
    tile_sync<TB>();  // every walker is done with the products and row ends: scratch may reuse them
    int *s_row = sm.scratch_row();
    double *s_val = sm.scratch_val();
    s_row[tid] = ex;
    s_val[tid] = run;
    tile_sync<TB>();
    if (pend) {  // close the row begun by earlier threads, summing their carries in thread order
        int j0 = tid - 1;
        while (j0 > 0 && s_row[j0 - 1] == prow)
            --j0;
        double acc = s_val[j0];
        for (int u = j0 + 1; u < tid; ++u)
            acc += s_val[u];
        write_row(prow, acc + pval);
    }
    if (tid == TB - 1 && tail) {  // the tile's trailing partial row -> carry
        int j0 = TB - 1;
        while (j0 > 0 && s_row[j0 - 1] == nrows)
            --j0;
        double acc = s_val[j0];
        for (int u = j0 + 1; u < TB; ++u)
            acc += s_val[u];
        store_sc1(&a.carry_val[t], acc);
        const int R = r0 + nrows;
        if (MODE == kModeCg) {
            const double2 v = cg_rp(a, R);
            dot += (v.x + beta * v.y) * acc;
        }
        else if (MODE == kModeDot)
            dot += a.xr[R] * acc;
    }
    tile_sync<TB>();  // LDS free for the next tile
}

// Row-group reduction of one tile whose products and row ends are in LDS (mode lg + 1 of
// k_tile_modes): groups of G = 2^lg lanes take the tile's row segments round-robin; lane j of
// a group sums products j, j+G, ... of the segment in order from 0.0, then a fixed xor
// butterfly folds the group.  G = 1 is the sequential CSR-order sum of SpmvGold
// (cpu_spmv.cpp:241-265), bit for bit.  A few instructions per product, against the walk's
// merge search and per-item row-end test, for tiles whose rows are alike.
// The group's lane 0 stores the row (G = 1: thread r stores row r, one coalesced store per
// round, as a staged store would be); no LDS beyond the product buffer.  xr / pr: r and p_old
// (CG) or x (dot mode) of row r0 + tid, loaded by the caller for tid <= nrows -- the operands
// of the rows a G = 1 thread owns first; other rows load their own.
template <int IPT, int MODE, int TB = kBlock, bool FIX = true>
__device__ __forceinline__ void group_tile(const TileArgs &a, SpmvSmem<IPT, TB> &sm, int t, int r0, int nrows,
                                           int nnzt, bool tail, double beta, double &dot, int lg, double xr,
                                           double pr)
{
    const int G = 1 << lg;
    const int tid = threadIdx.x;
    const int *rend = sm.rowend(nnzt);
    const int lane = tid & (G - 1);
    const int nseg = nrows + (tail ? 1 : 0);
    auto seg_sum = [&](int r) {
        const int s0 = r == 0 ? 0 : rend[r - 1];
        const int e = r < nrows ? rend[r] : nnzt;
        double v = 0.0;
        int k = s0 + lane;
        for (; k + 3 * G < e; k += 4 * G) {  // four independent LDS reads in flight
            const double p0 = sm.prod[pslot(k)], p1 = sm.prod[pslot(k + G)];
            const double p2 = sm.prod[pslot(k + 2 * G)], p3 = sm.prod[pslot(k + 3 * G)];
            v += p0;
            v += p1;
            v += p2;
            v += p3;
        }
        for (; k < e; k += G)
            v += sm.prod[pslot(k)];
        for (int off = G >> 1; off > 0; off >>= 1)
            v += __shfl_xor(v, off);
        return v;
    };
    for (int r = tid >> lg; r < nseg; r += TB >> lg) {  // uniform within a group
        const double v = seg_sum(r);
        if (lane != 0)
            continue;
        const int R = r0 + r;
        double ox = xr, op = pr;  // the row's operands: preloaded when r is this thread's own row
        if (MODE != kModeSpmv && r != tid) {
            if constexpr (MODE == kModeCg) {
                const double2 w = cg_rp(a, R);
                ox = w.x;
                op = w.y;
            } else {
                ox = a.xr[R];
            }
        }
        if (r < nrows) {
            *(FIX && r == 0 ? a.y0 : &a.y[R]) = v;
            if (MODE == kModeCg) {
                const double pn = ox + beta * op;
                cg_pstore(a, R, pn);
                dot += pn * v;
            } else if (MODE == kModeDot) {
                dot += ox * v;
            }
        } else {  // the trailing partial row -> carry (close_split_rows adds the row's carries in order)
            store_sc1(&a.carry_val[t], v);
            if (MODE == kModeCg)
                dot += (ox + beta * op) * v;
            else if (MODE == kModeDot)
                dot += ox * v;
        }
    }
    tile_sync<TB>();  // LDS free for the next tile
}

// One tile's reduction, by its plan-time mode (a.rmode[t]); tail = a.split[t + 1].
template <int IPT, int MODE, int TB = kBlock, bool FIX = true>
__device__ __forceinline__ void reduce_tile(const TileArgs &a, SpmvSmem<IPT, TB> &sm, int t, int r0, int n0, int nrows,
                                            int nnzt, int mode, bool tail, double beta, double &dot, double xr,
                                            double pr)
{
    if (mode == 0)
        walk_tile<IPT, MODE, TB, FIX>(a, sm, t, r0, n0, nrows, nnzt, tail, beta, dot);
    else
        group_tile<IPT, MODE, TB, FIX>(a, sm, t, r0, nrows, nnzt, tail, beta, dot, mode - 1, xr, pr);
}

// x[r0 + tid] (dot mode), or r and p_old at r0 + tid (CG), for the row-group epilogue, tid <= nrows.
template <int MODE>
__device__ __forceinline__ void row_operands(const TileArgs &a, int r0, int nrows, double &xr, double &pr)
{
    xr = pr = 0.0;
    if (MODE != kModeSpmv && (int)threadIdx.x <= nrows) {
        const int R = min(r0 + (int)threadIdx.x, a.m - 1);
        if constexpr (MODE == kModeCg) {
            const double2 v = cg_rp(a, R);
            xr = v.x;
            pr = v.y;
        } else {
            xr = a.xr[R];
        }
    }
}

// Dot-mode epilogue (split multi-RHS / row-sharded CG): this block's x.(Ax) partial ->
// partials[slot], a plain store; k_fold_dot (a later launch) sums the partials in tile order.
template <typename SM>
__device__ __forceinline__ void dot_epilogue(const TileArgs &a, SM &sm, int slot, double dot)
{
    const double tsum = block_sum(dot, sm.red);
    if (threadIdx.x == 0)
        a.partials[slot] = tsum;
}

// Pipelined single-RHS CG, deferred solution update.  x += alpha_{k-1} p_{k-1} (AxpySingle,
// single_strategy.hpp:143-144, the same expression) is applied by iteration k's SpMV to the rows of
// its tile instead of by the update kernel of iteration k-1: the SpMV already holds p_{k-1} for
// those rows (it rides in the {r, p} buffer it reads), so the update kernel no longer reads p and
// x or writes x.  The last pending term is applied by k_cg1_xflush after the loop.  The operands of
// the tile's first rows are loaded at entry (one row per thread); alpha_{k-1} is scal[0].alpha.
struct CgLag {
    double x, p, alpha;
    int k;
};

template <int TB>
__device__ __forceinline__ void cg1_lag_load(const TileArgs &a, int r0, int nrows, CgLag &g)
{
    const int i = threadIdx.x;
    g.k = a.ctrl->iter_par[a.parity];  // the iteration cg1_head runs (not written by this launch)
    g.alpha = a.scal[0].alpha;
    g.x = g.p = 0.0;
    if (i < nrows) {
        g.x = a.xsol[r0 + i];
        g.p = a.x[2 * (size_t)(r0 + i) + 1];
    }
}

template <int TB>
__device__ __forceinline__ void cg1_lag_store(const TileArgs &a, int r0, int nrows, const CgLag &g)
{
    if (g.k < 1)  // iteration 0: x = 0 and nothing is pending
        return;
    const int i = threadIdx.x;
    if (i < nrows)
        a.xsol[r0 + i] = g.x + g.alpha * g.p;
    for (int j = i + TB; j < nrows; j += TB) {  // tiles of more rows than threads (empty rows)
        const size_t R = (size_t)r0 + j;
        a.xsol[R] = a.xsol[R] + g.alpha * a.x[2 * R + 1];
    }
}

// Pipelined single-RHS CG tail of the SpMV: this tile's p.Ap partial, for the update kernel
// to sum (folded by group tickets only beyond kConsumeTile tiles).
template <typename SM>
__device__ __forceinline__ void cg1_publish(const TileArgs &a, SM &sm, int slot, int nslots, double dot)
{
    const double tsum = block_sum(dot, sm.red);
    if (nslots <= kConsumeTile) {  // the update kernel sums them: the launch boundary orders the store
        if (threadIdx.x == 0)
            a.partials[slot] = tsum;
        return;
    }
    if (threadIdx.x == 0) {  // a ticket tree folds them: publish at agent scope, drained
        store_sc1(&a.partials[slot], tsum);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    publish_partials<1>(a.partials, a.gtickets, slot, nslots, kConsumeTile, sm.prod, sm.red, &sm.last, a.ctrl);
}

// Single right-hand side, one tile per workgroup of TB threads.  TILE = TB*IPT merge items
// nominal, up to 1.125*TILE after snapping.  CG: gathers p = r + beta*p_old on the fly
// (UpdatePSingle, single_strategy.hpp:89-97, fused into the SpMV), writes p for its rows, Ap, and
// p.Ap by linearity.  TB = 64 (one-wave workgroups, SpMV only): every wave owns its tile, so no
// workgroup barrier ties a wave's progress to its siblings' gather latencies.
// BLK = false: the plan has no node-block tiles (a.blk null), and the kernel is compiled without
// their staging paths -- the pipelined CG's form then needs far fewer registers (their run arrays
// set its VGPR count, so more workgroups fit per CU).
// FIX: the plan splits rows (close_split_rows); plans that split none -- FEM, CFD, stencils -- run
// the form without it (fewer SGPRs: 8 workgroups per CU).
// STAMP (diagnostic instantiation only, mspmv_spmv_tile_stamps): thread 0 records wall_clock64() at the
// tile's phase boundaries into a.stamps[t * kTileStamps + i]: 0 entry, 1 stream and gathers issued, 2 the
// staged products in LDS (stream and gathers landed), 3 row ends in LDS (after the barrier), 4 rows
// reduced and stored; slot 5 holds the CU (HW_ID) that ran the tile.
constexpr int kTileStamps = 6;
template <int IPT, int MODE, bool NT, int TB = kBlock, bool BLK = true, bool FIX = true, bool STAMP = false>
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(STAMP ? 8 : 1))) void k_spmv_tile(TileArgs a)
{
    static_assert(TB == kBlock || MODE == kModeSpmv, "one-wave tiles run the plain SpMV only");
    constexpr bool CG = MODE == kModeCg;
    constexpr int TILE = SpmvSmem<IPT, TB>::TILE;
    constexpr int MAXJ = SpmvSmem<IPT, TB>::MAXJ;
    __shared__ SpmvSmem<IPT, TB> sm;
    const int tid = threadIdx.x;
    // CG: stop flag loaded now, tested after the stream and gathers are issued (see k_spmm_tile)
    const int stopped = (MODE != kModeSpmv || a.ctrl) ? a.ctrl->done : 0;  // MODE 0: a CG's plain SpMM
    const int t = xcd_tile(blockIdx.x, a.num_tiles);
    auto stamp = [&](int i) {
        if constexpr (STAMP) {
            if (tid == 0) {
                if (i == 0) {
                    unsigned hw;
                    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
                    a.stamps[(size_t)t * kTileStamps + 5] = hw;
                }
                a.stamps[(size_t)t * kTileStamps + i] = wall_clock64();
            }
        }
    };
    stamp(0);
    const int2 b0 = a.bounds[t];
    const int2 b1 = a.bounds[t + 1];
    const int r0 = b0.x, n0 = b0.y;
    const int nrows = b1.x - r0;
    const int nnzt = b1.y - n0;
    const int re_pre = a.early_re ? a.row_offsets[min(r0 + 1 + tid, a.m)] : 0;  // TileArgs::early_re
    const int4 fx = FIX ? load_fix(a, t) : make_int4(-1, 0, 0, 0);  // split rows (node-block tiles have none)
    if constexpr (FIX)
        a.y0 = fx.z > 0 ? a.head_val + t : a.y + r0;
    double beta = 0.0;
    bool go = true;
    // CG: the update's r.r partials are loaded first; summed (-> stop test, beta) once this
    // tile's stream and gathers are in flight.  Block-uniform, as is every branch on nnzt.
    PartRegs<CG ? kUpdateMaxBlocks / kBlock : 1> pin;
    CgLag lag{};
    if constexpr (CG) {
        part_load(a.part_in, a.n_part_in, pin);
        cg1_lag_load<TB>(a, r0, nrows, lag);
    }
    auto head = [&]() {  // the stop flag is tested before cg1_head records anything
        if (stopped)
            go = false;
        else if constexpr (CG)
            go = cg1_head(a, part_sum(pin, sm.red), beta);
    };
    const int colbase = a.cols16 ? a.colbase[t] : -1;
    // node-block descriptors of this tile, loaded beside its bounds (entry 0 holds the count)
    uint4 bd = make_uint4(0u, 0u, 0u, 0u);
    if (BLK && a.blk && (tid & 63) < a.blk_stride)
        bd = a.blk[(size_t)t * a.blk_stride + (tid & 63)];
    int nblk = (BLK && a.blk) ? (int)(((unsigned)__builtin_amdgcn_readfirstlane((int)bd.y) >> 8) & 255u) : 0;
    if (nblk > kBlkTileChunks)  // more than one round of runs: striped staging here (k_spmv_blk takes them)
        nblk = 0;
    bool staged = false;
    // every run one chunk wide (block-uniform: each wave holds all descriptors): no LDS at all
    const bool blk_reg = BLK && nblk > 0 && __ballot((tid & 63) < nblk && ((bd.x >> 16) & 255u) != 0) == 0;
    if constexpr (BLK) if (blk_reg) {
        double dot = 0.0;
        blk_rows<MODE, NT, TB>(a, t, bd, nblk, r0, n0, colbase, beta, dot, [&]() {
            head();
            return go;
        });
        if (!go)
            return;
        if constexpr (MODE == kModeCg) {
            cg1_lag_store<TB>(a, r0, nrows, lag);
            cg1_publish(a, sm, t, a.num_tiles, dot);
        } else if constexpr (MODE == kModeDot) {
            dot_epilogue(a, sm, t, dot);
        }
        return;
    }
    if (BLK && nblk > 0) {
        blk_stage<CG, NT, TB>(a, t, bd, nblk, n0, colbase, sm.prod, beta, [&]() {
            head();
            return go;
        });
        staged = true;
    } else if constexpr (MODE == kModeSpmv) {
        const int nd = a.dict ? a.ndict[t] : 0;  // > 0: this tile gathers through its dictionary
        if (nd > 0) {
            if (nnzt <= TILE)
                dict_stage<IPT, NT, TB>(a, sm.prod, nd, n0, nnzt);
            else
                dict_stage<MAXJ, NT, TB>(a, sm.prod, nd, n0, nnzt);
            staged = true;
        }
    }
    if (staged) {
    } else if (MODE == kModeSpmv && colbase >= 0 && nnzt > 0 && nnzt <= TILE) {
        constexpr int W = kGroupW;
        constexpr int NP = (TILE / TB + W - 1) / W;
        GroupRegs<NP, W> st;
        group_issue<NP, W, NT, TB>(a, n0, nnzt, colbase, 0, st);
        stamp(1);
        head();
        if (go) {
            group_store<NP, W, TB>(st, n0, nnzt, 0, sm.prod);
            if ((n0 + nnzt - 1) / W - n0 / W + 1 > NP * TB) {  // a start off the W-grid at the nominal size
                GroupRegs<1, W> ex;
                group_issue<1, W, NT, TB>(a, n0, nnzt, colbase, NP, ex);
                group_store<1, W, TB>(ex, n0, nnzt, NP, sm.prod);
            }
        }
    } else if (nnzt > 0 && nnzt <= TILE) {  // the common case: no snapped-in extra nonzeros
        StageRegs<IPT, CG> st;
        stage_issue<IPT, CG, NT, TB>(a, n0, nnzt, colbase, st);
        stamp(1);
        head();
        if (go)
            stage_store<IPT, CG, TB>(st, nnzt, beta, sm.prod);
    } else if (nnzt > TILE) {
        StageRegs<MAXJ, CG> st;
        stage_issue<MAXJ, CG, NT, TB>(a, n0, nnzt, colbase, st);
        head();
        if (go)
            stage_store<MAXJ, CG, TB>(st, nnzt, beta, sm.prod);
    } else {
        head();
    }
    if (!go)
        return;
    if constexpr (STAMP) {  // the staged products' stores are out (LDS): stamp after they complete
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        stamp(2);
    }
    // Row ends: issued with the stream by default (TileArgs::early_re; with the pair staging 1-2 %
    // faster, r03ah/r03ai -- with the old striped staging it had measured +0.9 us on pwtk), or here.
    int *rend = sm.rowend(nnzt);
    if (a.early_re) {
        if (tid < nrows)
            rend[tid] = re_pre - n0;
        for (int i = tid + TB; i < nrows; i += TB)  // rare: more rows than threads
            rend[i] = a.row_offsets[r0 + 1 + i] - n0;
    } else {
        for (int i = tid; i < nrows; i += TB)
            rend[i] = a.row_offsets[r0 + 1 + i] - n0;
    }
    tile_sync<TB>();
    stamp(3);
    double dot = 0.0;
    double xr, pr;
    row_operands<MODE>(a, r0, nrows, xr, pr);
    reduce_tile<IPT, MODE, TB, FIX>(a, sm, t, r0, n0, nrows, nnzt, a.rmode[t], a.split[t + 1] != 0, beta, dot, xr, pr);
    if constexpr (STAMP) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the rows' stores have left
        stamp(4);
    }
    if constexpr (FIX)
        close_split_rows<TB>(a, t, fx, 1, 1);
    if constexpr (MODE == kModeCg) {
        cg1_lag_store<TB>(a, r0, nrows, lag);
        cg1_publish(a, sm, t, a.num_tiles, dot);
    } else if constexpr (MODE == kModeDot) {
        dot_epilogue(a, sm, t, dot);
    }
}

// Register fallback of the plain node-block SpMV for the tiles of a mixed plan that are not register
// run tiles (rows outside any run pattern, patterns wider than 64 columns, split boundaries): groups
// of G lanes take the tile's row segments round-robin (its whole rows, then the trailing partial row
// of a split boundary), lane j of a group sums products j, j + G, ... of its segment in order, a
// fixed xor butterfly folds the group and its lane 0 stores the row (the
// trailing partial row: the tile's carry, which the completing tile adds, close_split_rows).  No LDS, so the kernel keeps its
// register-only occupancy.  G is the smallest power of two with 4 G >= the tile's mean segment
// length.  Reproducible, and within the 2 (len+1) eps (|A||x|)_i reordering bound of the CSR-order
// sum (mspmv_tile_modes reports these tiles as 255).
template <bool NT>
__device__ __forceinline__ void tile_rows_reg(const TileArgs &a, int t, int r0, int n0, int colbase)
{
    const int2 b1 = a.bounds[t + 1];
    const int nrows = b1.x - r0, nnzt = b1.y - n0;
    const int nseg = nrows + (a.split[t + 1] ? 1 : 0);
    if (nseg == 0)
        return;
    const int mean = (nnzt + nseg - 1) / nseg;
    int lg = 0;
    while (lg < 6 && (4 << lg) < mean)
        ++lg;
    const int G = 1 << lg;
    const int lane = threadIdx.x & (G - 1);
    auto col = [&](int k) {
        return colbase >= 0 ? colbase + (int)ld_stream<NT>(a.cols16 + n0 + k) : ld_stream<NT>(a.cols + n0 + k);
    };
    for (int r = (int)threadIdx.x >> lg; r < nseg; r += kBlock >> lg) {  // uniform within a group
        const int s0 = r == 0 ? 0 : a.row_offsets[r0 + r] - n0;
        const int e = r < nrows ? a.row_offsets[r0 + r + 1] - n0 : nnzt;
        double v = 0.0;
        for (int k = s0 + lane; k < e; k += G)
            v += ld_stream<NT>(a.vals + n0 + k) * a.x[col(k)];
        for (int off = G >> 1; off > 0; off >>= 1)
            v += __shfl_xor(v, off);
        if (lane == 0) {
            if (r < nrows)
                *(r == 0 ? a.y0 : &a.y[r0 + r]) = v;
            else
                store_sc1(&a.carry_val[t], v);
        }
    }
}

// Single right-hand side, node-block plans (FEM matrices such as pwtk): the tile kernel without any
// LDS staging (only the CG / dot-mode epilogue's 2 KB), so occupancy is set by registers alone -- 8
// workgroups (32 waves) per CU instead of the 7 that k_spmv_tile's 22.6 KB of LDS allow.  Plain SpMV
// (MODE 0, column pairs): register run tiles through blk_rows_pair, every other tile of the plan
// through tile_rows_reg, so a plan whose tiles are mostly node blocks runs here whole (blk_spmv).
// Dot mode: plans whose EVERY tile is a register run tile, the per-tile work of k_spmv_tile's
// blk_rows path.
struct BlkSmem {
    double red[kBlock / 64];
    double cval[kBlock];
    int last;
};

// FB (plain SpMV): the plan has tiles that are not register run tiles, so the register fallback is
// compiled in; without it the kernel takes 64 SGPRs, with it 88 -- and 256-thread workgroups are
// admitted 8 per CU only up to .sgpr_count 80 (7 at 82-96, MI355X_MICROARCH.md "Residency"), so plans
// of run tiles only keep the lean form.
template <int MODE, bool NT, int KR = kBlkRows, bool FB = false>
__global__ __launch_bounds__(kBlock) void k_spmv_blk(TileArgs a)
{
    constexpr bool CG = MODE == kModeCg;
    __shared__ BlkSmem sm;
    const int tid = threadIdx.x;
    const int stopped = (MODE != kModeSpmv || a.ctrl) ? a.ctrl->done : 0;  // MODE 0: a CG's plain SpMM
    const int t = xcd_tile(blockIdx.x, a.num_tiles);
    const int2 b0 = a.bounds[t];
    const int colbase = a.colbase[t];
    const uint4 bd =
        (tid & 63) < a.blk_stride ? a.blk[(size_t)t * a.blk_stride + (tid & 63)] : make_uint4(0u, 0u, 0u, 0u);
    const int nblk = (int)(((unsigned)__builtin_amdgcn_readfirstlane((int)bd.y) >> 8) & 255u);
    double beta = 0.0, dot = 0.0;
    bool go = true;
    PartRegs<CG ? kUpdateMaxBlocks / kBlock : 1> pin;
    if constexpr (CG)
        part_load(a.part_in, a.n_part_in, pin);
    if constexpr (MODE == kModeSpmv && KR <= 6) {  // taller runs: 73 VGPRs, column owners
        // round 0's records, issued with the header: descriptor and pattern columns in one load, so the
        // tile's chain is header -> x, as long as the values' header -> rows (a tile without runs reads
        // its zeroed records and drops them)
        const unsigned rec = blk_pair_rec<NT>(a, t, 0);
        // ... all of it consumed here, ahead of the exits below: left alone, the compiler sinks the
        // bounds and the record behind the stop test, one round trip each
        asm volatile("" ::"s"(b0.x), "s"(b0.y), "s"(colbase), "v"(rec));
        if (stopped)
            return;
        // the tile's descriptor count, in every record (lane 1: dword 1 of the first half's); 0 unless
        // the tile is a register run tile (k_fill_recs)
        const int nrec = (int)(((unsigned)__builtin_amdgcn_readlane((int)rec, 1) >> 8) & 255u);
        if constexpr (FB) {
            if (nrec == 0) {
                const int4 fx = load_fix(a, t);
                a.y0 = fx.z > 0 ? a.head_val + t : a.y + b0.x;
                tile_rows_reg<NT>(a, t, b0.x, b0.y, a.cols16 ? colbase : -1);
                close_split_rows<kBlock>(a, t, fx, 1, 1);
                return;
            }
        }
        blk_rows_pair<NT, KR>(a, t, rec, nrec, b0.x, b0.y, colbase);
        return;
    }
    blk_rows<MODE, NT, kBlock>(a, t, bd, nblk, b0.x, b0.y, colbase, beta, dot, [&]() {
        if (stopped)
            go = false;
        else if constexpr (CG)
            go = cg1_head(a, part_sum(pin, sm.red), beta);
        return go;
    });
    if (!go)
        return;
    if constexpr (MODE == kModeCg)
        cg1_publish(a, sm, t, a.num_tiles, dot);
    else if constexpr (MODE == kModeDot)
        dot_epilogue(a, sm, t, dot);
}

// Row-group reduction of one multi-RHS tile (mode lgp + 1): a row group is GL column-pair
// lanes x Gp = 2^lgp nonzero lanes.  Lane (c, j) of a group sums, for its columns 2c, 2c+1,
// the products of nonzeros j, j+Gp, ... of the row in order from 0.0 (four panel-row gathers
// in flight), a fixed xor butterfly over j folds the group, and j = 0 writes the row.
// Gp = 1 is the row-by-row CSR-order sum of the reference's row-split SpMM, bit for bit.
// DICT: s_col holds each nonzero's position in the tile's column dictionary and the panel rows
// are read from s_panel (parked there by k_spmm_tile) -- the same operands, the same sums.
// Dot mode (MODE 2) of the row-group SpMM tiles: the x.(Ax) contribution of the tile's whole rows
// is taken after the row loop, from the Ap rows the workgroup has just stored and the rows' own x
// (both contiguous nrows x L slices, L2-resident: x[R] is a column of row R), instead of holding
// each row's x and the running dot in registers through the gathers -- the dot mode then needs
// no more registers than the plain SpMM, so it keeps the plain kernel's occupancy.

template <int L, bool DICT = false, bool FIX = true>
__device__ __forceinline__ void spmm_group_rows(const TileArgs &a, const int *s_col, const double *s_val,
                                                const int *rend, int t, int r0, int nrows, int nnzt, int lgp,
                                                const double2 *s_panel = nullptr)
{
    constexpr int GL = L / 2;
    const int Gp = 1 << lgp;
    const int tid = threadIdx.x;
    const int lane = tid % GL;
    const int sub = (tid / GL) & (Gp - 1);
    const int W = GL << lgp;
    const bool tail = a.split[t + 1] != 0;
    const int nseg = nrows + (tail ? 1 : 0);
    auto panel = [&](int c) {
        if constexpr (DICT)
            return s_panel[c * GL + lane];
        else
            return *reinterpret_cast<const double2 *>(a.x + (size_t)c * a.ld + 2 * lane);
    };
    for (int r = tid / W; r < nseg; r += kBlock / W) {  // uniform within a group
        const int s0 = r == 0 ? 0 : rend[r - 1];
        const int e = r < nrows ? rend[r] : nnzt;
        double2 acc = make_double2(0.0, 0.0);
        int k = s0 + sub;
        // batches of 8 panel-row gathers in flight per lane (the SpMM is gather-latency bound:
        // bytes in flight per CU set its rate), then 4, then singles; sums stay in order
        for (; k + 7 * Gp < e; k += 8 * Gp) {
            double v[8];
            double2 xv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                v[u] = s_val[k + u * Gp];
                xv[u] = panel(s_col[k + u * Gp]);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                acc.x += v[u] * xv[u].x;
                acc.y += v[u] * xv[u].y;
            }
        }
        // the rest (< 8 per lane) as ONE batch, not a chain of single round trips: indices past
        // the row clamp to its last nonzero and their products are skipped by a select (acc
        // starts at +0.0 and never becomes -0.0, so adding +0.0 instead is the identity: the
        // sums stay bit-identical)
        auto rest = [&](auto nb) {
            constexpr int NB = decltype(nb)::value;
            double v[NB];
            double2 xv[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int kk = min(k + u * Gp, e - 1);
                v[u] = s_val[kk];
                xv[u] = panel(s_col[kk]);
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const bool on = k + u * Gp < e;
                acc.x += on ? v[u] * xv[u].x : 0.0;
                acc.y += on ? v[u] * xv[u].y : 0.0;
            }
        };
        if (k + 3 * Gp < e)
            rest(std::integral_constant<int, 8>{});
        else if (k < e)
            rest(std::integral_constant<int, 4>{});
        for (int off = Gp >> 1; off > 0; off >>= 1) {
            acc.x += __shfl_xor(acc.x, off * GL);
            acc.y += __shfl_xor(acc.y, off * GL);
        }
        if (sub == 0) {
            const size_t off = (size_t)(r0 + r) * a.ld + 2 * lane;
            if (r < nrows)
                // nontemporal: Y does not displace the panel X from the caches (nlpkkt120 size, L = 8:
                // 476 -> 450 us per SpMM, r04n)
                __builtin_nontemporal_store(v2d_t{acc.x, acc.y},
                                            reinterpret_cast<v2d_t *>(FIX && r == 0 ? a.y0 + 2 * lane : a.y + off));
            else  // the trailing partial row -> carry (close_split_rows adds the row's carries in order)
                store_sc1_2(a.carry_val + (size_t)t * L + 2 * lane, acc);
        }
    }
}

// Multi right-hand side (L = 2..16, row-major panels).  A group of L/2 lanes owns one merge
// walk; each lane keeps a double2 of the L running totals (running_total[L],
// merge_based.hpp:84-127).  TILE = (256/(L/2)) groups * IPTG items.
// Workgroups per CU the multi-RHS tile's LDS allows, capped at 7: the register budget is pinned
// to it (the dot mode would otherwise need 90 VGPRs and fall to 5 workgroups at L = 8).
constexpr int spmm_waves_per_eu(int L, int IPTG, bool DICT = false)
{
    const int items = (kBlock / (L / 2)) * IPTG;
    const int lds = 16 * (items + items / kSnapDiv) + 6144 + (DICT ? spmm_dict_bytes(L) : 0);  // + s_crow, s_cval, s_red2
    const int w = 163840 / lds;
    return w < 1 ? 1 : w > 7 ? 7 : w;
}

// DICT: tiles with a column dictionary (multi-RHS plans, k_build_dict) gather each distinct
// panel row once, coalesced (the dictionary is sorted: neighbouring columns share lines), into
// LDS, and the row groups read the panel there: at L = 16 a FEM-blocked tile repeats each of
// its columns ~6 times.  Walk-mode tiles and tiles without one gather directly.  Measured
// (pwtk shape): L = 16 130 -> 102 us; at L = 4 and 8 it lost (47 -> 55, 63 -> 67 us; the
// 27-point nlpkkt120 size at L = 8 505 -> 590 us: the extra dependent round trip and the
// occupancy the 16 KB panel costs outweigh 64-B gathers), so only L = 16 plans build one.
// (Grouped staging, 4 nonzeros per lane: measured even, CG multi L = 8 0.915-0.920 vs 0.914 ms per
// iteration, r03z -- not kept.)
template <int L, int IPTG, int MODE, bool NT, bool DICT = false, bool FIX = true>  // FIX: as k_spmv_tile's
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(spmm_waves_per_eu(L, IPTG, DICT)))) void
k_spmm_tile(TileArgs a)
{
    static_assert(MODE != kModeCg, "multi-RHS CG runs the split iteration (MODE 2)");
    constexpr int GL = L / 2;
    constexpr int NG = kBlock / GL;
    constexpr int TILE = NG * IPTG;
    constexpr int MAXI = TILE + TILE / kSnapDiv;
    constexpr int MAXJ = (MAXI + NG - 1) / NG;
    constexpr int STG = (MAXI + kBlock - 1) / kBlock;
    __shared__ int s_rowend[MAXI];
    __shared__ int s_col[MAXI];
    __shared__ double s_val[MAXI];
    __shared__ int s_crow[NG];
    __shared__ double2 s_cval[NG * GL];
    __shared__ double2 s_red2[kBlock / 64][GL];
    constexpr int DMAX = DICT ? spmm_dict_max(L) : 1;
    constexpr int DJ = (DMAX + NG - 1) / NG;  // dictionary entries per lane group (4)
    __shared__ double2 s_panel[DICT ? DMAX * GL : 1];

    const int tid = threadIdx.x;
    const int g = tid / GL;
    const int lane = tid % GL;
    // CG: the stop flag is loaded now and tested once the tile's stream is in flight, so the
    // flag's round trip does not delay every workgroup's first load (MODE 2 writes only the
    // scratch Ap and partials: a stopped solve only needs the work skipped, not fenced)
    const int stopped = (MODE != kModeSpmv || a.ctrl) ? a.ctrl->done : 0;  // MODE 0: a CG's plain SpMM
    const int t = xcd_tile(blockIdx.x, a.num_tiles);
    const int2 b0 = a.bounds[t];
    const int2 b1 = a.bounds[t + 1];
    const int r0 = b0.x, n0 = b0.y;
    const int nrows = b1.x - r0;
    const int nnzt = b1.y - n0;
    const int items = nrows + nnzt;
    const int rmode = a.rmode[t];
    __shared__ int4 s_fix;  // parked in LDS until the epilogue: no registers held through the tile
    if constexpr (FIX) {
        if (tid == 0)
            s_fix = a.fix ? a.fix[t] : make_int4(-1, 0, 0, 0);
        a.y0 = a.fix && __builtin_amdgcn_readfirstlane(a.fix[t].z) > 0 ? a.head_val + (size_t)t * L
                                                                        : a.y + (size_t)r0 * a.ld;
    }
    int nd = 0;  // > 0: this tile reads its panel rows from s_panel
    if constexpr (DICT) {
        nd = a.ndict[t];
        if (nd > DMAX || rmode == 0)
            nd = 0;
    }
    int dcol[DJ];
    if constexpr (DICT) {  // the dictionary's columns first: the panel gathers wait on them
#pragma unroll
        for (int u = 0; u < DJ; ++u)
            dcol[u] = nd > 0 ? a.dict[n0 + min(g + u * NG, nd - 1)] : 0;
    }

    // Every round's loads are issued before any is stored to LDS (indices clamped into the
    // tile), the first round of row ends with them: one memory round trip per tile, not STG.
    const int re0 = a.row_offsets[min(r0 + 1 + min(tid, max(nrows - 1, 0)), a.m)];  // clamped: always issued
    if (!DICT && nnzt > 0) {  // block-uniform: aligned pairs (one 8-B column load and one 16-B value load
                              // per two nonzeros: half the stream instructions; pairs straddling the
                              // tile's ends load a neighbour's element and skip its store)
        constexpr int STG2 = (MAXI / 2 + 1 + kBlock - 1) / kBlock;
        const int q0 = n0 >> 1, qlast = (n0 + nnzt - 1) >> 1;
        int2 cp[STG2];
        double2 vp[STG2];
#pragma unroll
        for (int j = 0; j < STG2; ++j) {
            const int q = min(q0 + tid + j * kBlock, qlast);
            const v2i_t c = NT ? __builtin_nontemporal_load(reinterpret_cast<const v2i_t *>(a.cols) + q)
                               : reinterpret_cast<const v2i_t *>(a.cols)[q];
            cp[j] = make_int2(c.x, c.y);
        }
#pragma unroll
        for (int j = 0; j < STG2; ++j)
            vp[j] = ld_stream<NT>(reinterpret_cast<const double2 *>(a.vals) + min(q0 + tid + j * kBlock, qlast));
#pragma unroll
        for (int j = 0; j < STG2; ++j) {
            const int q = q0 + tid + j * kBlock;
            const int k = 2 * q - n0;
            if (q <= qlast) {
                if (k >= 0) {
                    s_col[k] = cp[j].x;
                    s_val[k] = vp[j].x;
                }
                if (k + 1 < nnzt) {
                    s_col[k + 1] = cp[j].y;
                    s_val[k + 1] = vp[j].y;
                }
            }
        }
    }
    if (DICT && nnzt > 0) {  // block-uniform
        int cst[STG];
        double vst[STG];
        if (DICT && nd > 0) {
#pragma unroll
            for (int j = 0; j < STG; ++j)
                cst[j] = (int)ld_stream<NT>(a.idx16 + n0 + min(tid + j * kBlock, nnzt - 1));
        } else {
#pragma unroll
            for (int j = 0; j < STG; ++j)
                cst[j] = ld_stream<NT>(a.cols + n0 + min(tid + j * kBlock, nnzt - 1));
        }
#pragma unroll
        for (int j = 0; j < STG; ++j)
            vst[j] = ld_stream<NT>(a.vals + n0 + min(tid + j * kBlock, nnzt - 1));
        if constexpr (DICT) {
            if (nd > 0) {  // each distinct panel row once: lane group g takes entries g, g + NG, ...
                double2 pv[DJ];
#pragma unroll
                for (int u = 0; u < DJ; ++u)
                    pv[u] = *reinterpret_cast<const double2 *>(a.x + (size_t)dcol[u] * a.ld + 2 * lane);
#pragma unroll
                for (int u = 0; u < DJ; ++u)
                    if (g + u * NG < nd)
                        s_panel[(g + u * NG) * GL + lane] = pv[u];
            }
        }
#pragma unroll
        for (int j = 0; j < STG; ++j) {
            const int k = tid + j * kBlock;
            if (k < nnzt) {
                s_col[k] = cst[j];
                s_val[k] = vst[j];
            }
        }
    }
    if (tid < nrows)
        s_rowend[tid] = re0 - n0;
    for (int i = kBlock + tid; i < nrows; i += kBlock)  // rare: > 256 rows in the tile
        s_rowend[i] = a.row_offsets[r0 + 1 + i] - n0;
    __syncthreads();
    if (stopped)
        return;

    double2 dot = make_double2(0.0, 0.0);
    if (rmode != 0) {
        if (DICT && nd > 0)
            spmm_group_rows<L, true, FIX>(a, s_col, s_val, s_rowend, t, r0, nrows, nnzt, rmode - 1, s_panel);
        else
            spmm_group_rows<L, false, FIX>(a, s_col, s_val, s_rowend, t, r0, nrows, nnzt, rmode - 1);
    } else {
    const int ipt = (items + NG - 1) / NG;
    const int d0 = min(g * ipt, items);
    const int d1 = min(d0 + ipt, items);
    int cx, cy, ex, ey;
    lds_search(d0, s_rowend, nrows, nnzt, cx, cy);
    lds_search(d1, s_rowend, nrows, nnzt, ex, ey);
    const bool need_cin = (cx < ex) && (cy > (cx == 0 ? 0 : s_rowend[cx - 1]));

    auto write_row = [&](int row, double2 val) {
        __builtin_nontemporal_store(v2d_t{val.x, val.y},  // nontemporal, as spmm_group_rows' row stores
                                    reinterpret_cast<v2d_t *>(FIX && row == 0 ? a.y0 + 2 * lane
                                                                              : a.y + (size_t)(r0 + row) * a.ld + 2 * lane));
    };

    double2 run = make_double2(0.0, 0.0);
    bool first = true, pend = false;
    int prow = 0;
    double2 pval = make_double2(0.0, 0.0);
    // The walk in chunks of WJ items: each chunk's panel rows are gathered together (WJ
    // independent 16-B loads in flight, indices clamped so every load is issued), then walked.
    constexpr int WJ = 4;
#pragma unroll
    for (int j0 = 0; j0 < MAXJ; j0 += WJ) {
        if (cy + j0 >= ey)
            break;
        double2 xr[WJ];
        double vv[WJ];
#pragma unroll
        for (int jj = 0; jj < WJ; ++jj) {
            const int k = min(cy + j0 + jj, ey - 1);
            vv[jj] = s_val[k];
            xr[jj] = *reinterpret_cast<const double2 *>(a.x + (size_t)s_col[k] * a.ld + 2 * lane);
        }
#pragma unroll
        for (int jj = 0; jj < WJ; ++jj) {
            const int k = cy + j0 + jj;
            if (j0 + jj < MAXJ && k < ey) {
                while (cx < ex && s_rowend[cx] <= k) {
                    if (first && need_cin) {
                        pend = true;
                        prow = cx;
                        pval = run;
                    } else {
                        write_row(cx, run);
                    }
                    first = false;
                    run = make_double2(0.0, 0.0);
                    ++cx;
                }
                run.x += vv[jj] * xr[jj].x;
                run.y += vv[jj] * xr[jj].y;
            }
        }
    }
    while (cx < ex) {
        if (first && need_cin) {
            pend = true;
            prow = cx;
            pval = run;
        } else {
            write_row(cx, run);
        }
        first = false;
        run = make_double2(0.0, 0.0);
        ++cx;
    }
    if (lane == 0)
        s_crow[g] = ex;
    s_cval[g * GL + lane] = run;
    __syncthreads();

    if (pend) {
        int j0 = g - 1;
        while (j0 > 0 && s_crow[j0 - 1] == prow)
            --j0;
        double2 acc = s_cval[j0 * GL + lane];
        for (int u = j0 + 1; u < g; ++u) {
            const double2 c = s_cval[u * GL + lane];
            acc.x += c.x;
            acc.y += c.y;
        }
        acc.x += pval.x;
        acc.y += pval.y;
        write_row(prow, acc);
    }
    if (g == NG - 1 && a.split[t + 1]) {
        int j0 = NG - 1;
        while (j0 > 0 && s_crow[j0 - 1] == nrows)
            --j0;
        double2 acc = s_cval[j0 * GL + lane];
        for (int u = j0 + 1; u < NG; ++u) {
            const double2 c = s_cval[u * GL + lane];
            acc.x += c.x;
            acc.y += c.y;
        }
        store_sc1_2(a.carry_val + (size_t)t * L + 2 * lane, acc);
    }
    }  // merge walk

    if (MODE == kModeDot) {
        // the tile's whole Ap rows, stored above by its own waves (either path): drained, then
        // visible to the workgroup after the barrier (one CU, and no wave read these lines before).
        // Pair e = (row e / GL, columns 2 (e % GL) + {0, 1}); kBlock % GL == 0, so a thread always
        // takes its own column pair `lane`, as the in-loop dot does.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // The trailing partial row (a carry, added to the row by the tile completing it) counts by
        // linearity: its x times the carry this tile stored.  (The row this tile completes is read
        // before close_split_rows adds the earlier tiles' carries to it: they count in their tiles.)
        const int npair = (nrows + (a.split[t + 1] ? 1 : 0)) * GL;
        for (int e = tid; e < npair; e += kBlock) {
            const int row = e / GL;
            const size_t off = (size_t)(r0 + row) * a.ld + 2 * lane;
            const double2 ap = *reinterpret_cast<const double2 *>(
                row < nrows ? (FIX && row == 0 ? a.y0 + 2 * lane : a.y + off) : a.carry_val + (size_t)t * L + 2 * lane);
            const double2 xx = *reinterpret_cast<const double2 *>(a.xr + off);
            dot.x += xx.x * ap.x;
            dot.y += xx.y * ap.y;
        }
    }
    if (MODE != kModeSpmv) {
        // Reduce the per-lane column partials over the groups (lanes with equal tid % GL).
#pragma unroll
        for (int off = 32; off >= GL; off >>= 1) {
            dot.x += __shfl_xor(dot.x, off);
            dot.y += __shfl_xor(dot.y, off);
        }
        if ((tid & 63) < GL)
            s_red2[tid >> 6][lane] = dot;
        __syncthreads();
        if (tid < GL) {
            double2 tsum = s_red2[0][tid];
#pragma unroll
            for (int w = 1; w < kBlock / 64; ++w) {
                tsum.x += s_red2[w][tid].x;
                tsum.y += s_red2[w][tid].y;
            }
            // plain stores: k_fold_dot (a later launch) sums the tiles' partials
            a.partials[(size_t)t * L + 2 * tid] = tsum.x;
            a.partials[(size_t)t * L + 2 * tid + 1] = tsum.y;
        }
    }
    if constexpr (FIX)
        close_split_rows<kBlock>(a, t, s_fix, L, a.ld);  // (s_fix: written before the staging barrier)
}

// ---- node-block SpMM (plans whose every single-RHS tile is a register node-block tile) --------
// Y = A X for L right-hand sides on the single-RHS plan's tiles and run descriptors.  A wave takes
// one run (<= 64 pattern columns) at a time; its lanes form 64/(L/2) column groups of L/2 lanes
// (one double2 of the panel row each).  Per pass a group owns pattern column j: it gathers panel
// row X[P[j]] ONCE and multiplies it into all h rows of the run, so the L2 -> CU gather traffic is
// one panel row per (run, column) instead of one per nonzero (1/6 of it on the pwtk shape).  The
// run's values and P arrive by coalesced loads (lane j holds column j) and reach the column groups
// by shuffles; the h row sums are folded across the groups by a reduce-scatter and group i stores
// row i (L/2 lanes x 16 B, contiguous).  No LDS, no carries (node-block tiles hold whole rows).
template <int GL>
__device__ __forceinline__ double2 rows8_sum2(const double2 (&p)[kBlkRows])
{
    const int lane = threadIdx.x & 63;
    const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
    auto sx = [](double2 v, int off) { return make_double2(__shfl_xor(v.x, off), __shfl_xor(v.y, off)); };
    auto add = [](double2 u, double2 v) { return make_double2(u.x + v.x, u.y + v.y); };
    double2 q4[4], q2[2];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        q4[k] = add(b5 ? p[k + 4] : p[k], sx(b5 ? p[k] : p[k + 4], 32));
#pragma unroll
    for (int k = 0; k < 2; ++k)
        q2[k] = add(b4 ? q4[k + 2] : q4[k], sx(b4 ? q4[k] : q4[k + 2], 16));
    double2 v = add(b3 ? q2[1] : q2[0], sx(b3 ? q2[0] : q2[1], 8));
#pragma unroll
    for (int off = 4; off >= GL; off >>= 1)  // column groups inside the 8-lane row slot
        v = add(v, sx(v, off));
    return v;
}

// Waves per SIMD k_spmm_blk is compiled for: 8 (<= 64 VGPRs; with the pass fence below the L = 16
// kernel takes 60 and spills nothing).  Unconstrained the straight-line passes take 82 VGPRs (6
// waves): pwtk L = 16 58.5 vs 51-52 us hot at 8 waves (r03g).  The instantiations that fit 64 VGPRs
// without spilling (plain SpMM, runs of <= 6 rows, L >= 4); the others (L = 2, 8-row runs, dot
// mode) stay unconstrained rather than spill.
constexpr int spmm_blk_waves(int L, int MODE, int KR) { return MODE == 0 && KR <= 6 && L >= 4 ? 8 : 1; }
// KR: the plan's tallest run (rows of one node, <= kBlkRows); KR = 6 (6-DOF FEM such as pwtk)
// holds fewer accumulator and value registers than 8.
template <int L, int MODE, bool NT, int KR = kBlkRows>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(spmm_blk_waves(L, MODE, KR)))) void
k_spmm_blk(TileArgs a)
{
    static_assert(MODE != kModeCg, "multi-RHS CG runs the split iteration (MODE 2)");
    constexpr int GL = L / 2;      // lanes per panel row
    constexpr int NGW = 64 / GL;   // column groups per wave = pattern columns per pass
    // passes whose gathers are in flight together, measured on the pwtk shape: with the values in
    // registers (before LDSV) 4 was best at L = 16 and 2 at L = 4, 8 (r02z); with LDSV 2 is best at
    // every width (L = 16: 72.4-73.1 vs 74.4-74.8 us at 4 and 89.4 at 8; L = 4: 40-41 vs 50-51 and
    // 65 us; r02ah).  Fused multiply-adds instead of the guarded mul + add measured slower.
    // straight-line passes (r03g, pwtk, hot): L = 16 PB 2 50.9-51.7 us vs PB 1 53.4-54.6; L = 8 PB 1
    // 43.0-43.4 vs 43.6-45.6; L = 4 PB 1 37.3 vs 40.5-41.7
    constexpr int PB = L >= 16 ? 2 : 1;
    __shared__ double2 s_red2[MODE == kModeDot ? kBlock / 64 : 1][GL];
    // each wave parks its run's values (row-major, [row][column]) and pattern columns in its own LDS
    // slice, and a pass reads v[i][j] there (one broadcast read per (pass, row)) instead of holding
    // the rows in registers and shuffling them (two bpermutes per (pass, row)): r02ag
    __shared__ __attribute__((aligned(16))) double s_v[kBlock / 64][kBlkRows][64];
    __shared__ int s_c[kBlock / 64][64];
    const int stopped = (MODE != kModeSpmv || a.ctrl) ? a.ctrl->done : 0;  // MODE 0: a CG's plain SpMM
    const int tid = threadIdx.x, lane = tid & 63;
    const int g = lane / GL, c = lane % GL;
    const int t = xcd_tile(blockIdx.x, a.num_tiles);
    const int2 b0 = a.bounds[t];
    const int r0 = b0.x, n0 = b0.y;
    const int colbase = a.colbase[t];
    const uint4 bd = lane < a.blk_stride ? a.blk[(size_t)t * a.blk_stride + lane] : make_uint4(0u, 0u, 0u, 0u);
    const int nd = (int)(((unsigned)__builtin_amdgcn_readfirstlane((int)bd.y) >> 8) & 255u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    double2 dot = make_double2(0.0, 0.0);
    // lane j: P[j] and the run's values in column j of chunk di, one coalesced load per row
    auto fetch = [&](int di, int &cj, double (&vr)[KR]) {
        const uint4 d = blk_read(bd, di);
        const int vofs = d.x & 0xffff, wc = d.x >> 24;
        const int h = d.y & 15;
        int start[KR];
        int acc_s = 0;
#pragma unroll
        for (int i = 0; i < KR; ++i) {
            start[i] = acc_s;
            acc_s += i < h ? blk_len(d, i) : 0;
        }
        cj = lane < wc ? colbase + (int)ld_stream<NT>(blk_slot(a, t, di) + lane) : 0;
#pragma unroll
        for (int i = 0; i < KR; ++i)
            vr[i] = (i < h && lane < blk_len(d, i)) ? ld_stream<NT>(a.vals + n0 + vofs + start[i] + lane) : 0.0;
    };
    for (int di = wave; di < nd && !stopped; di += kBlock / 64) {  // wave-uniform
        const uint4 d = blk_read(bd, di);
        const int wc = d.x >> 24;
        const int h = d.y & 15, rofs = d.y >> 16;
        {  // wave-private slice: the wave's LDS operations stay in order
            int colj;
            double vrow[KR];
            fetch(di, colj, vrow);
            s_c[wave][lane] = colj;
#pragma unroll
            for (int i = 0; i < KR; ++i)  // rows >= h too (0.0 from fetch): the passes read every row
                s_v[wave][i][lane] = vrow[i];
            __builtin_amdgcn_wave_barrier();
        }
        const int ri = lane >> 3;  // the run row this lane's slot stores
        const bool store = (lane & 7) < GL && ri < h;
        double2 xx = make_double2(0.0, 0.0);  // dot mode: the stored row's own x, issued early
        if (MODE == kModeDot && store)
            xx = *reinterpret_cast<const double2 *>(a.xr + (size_t)(r0 + rofs + ri) * a.ld + 2 * c);
        double2 acc[kBlkRows];  // rows KR.. stay 0.0 (compile-time constants: no registers)
#pragma unroll
        for (int i = 0; i < kBlkRows; ++i)
            acc[i] = make_double2(0.0, 0.0);
        // Straight-line passes: every LDS read and gather of a pass is unconditional, so a pass has
        // ONE dependent LDS round trip (its column indices) and one gather round trip, not one per
        // row (the per-row branches serialised six LDS round trips per pass: passes took 6 of a
        // chunk's 8.6 us, r03e stamps).  Lanes past the chunk width hold column 0 (a valid panel
        // row); rows >= h hold 0.0 (fetch) and are never stored.
        int minlen = 64;
#pragma unroll
        for (int i = 0; i < KR; ++i)
            minlen = i < h ? min(minlen, blk_len(d, i)) : minlen;
        int pb = 0;
        // groups of PB passes whose columns all lie in every row of the run: in-place fused
        // multiply-adds, no select, no merge of paths (the accumulators stay in place)
        for (; (pb + PB) * NGW <= minlen; pb += PB) {  // wave-uniform
            int cq[PB];
#pragma unroll
            for (int q = 0; q < PB; ++q)
                cq[q] = s_c[wave][((pb + q) * NGW + g) & 63];
            double2 xv[PB];
#pragma unroll
            for (int q = 0; q < PB; ++q)
                xv[q] = *reinterpret_cast<const double2 *>(a.x + (size_t)cq[q] * a.ld + 2 * c);
#pragma unroll
            for (int q = 0; q < PB; ++q) {
                const int j = (pb + q) * NGW + g;
#pragma unroll
                for (int i = 0; i < KR; ++i) {
                    const double v = s_v[wave][i][j & 63];
                    acc[i].x = __builtin_fma(v, xv[q].x, acc[i].x);
                    acc[i].y = __builtin_fma(v, xv[q].y, acc[i].y);
                }
                // pass q + 1's value reads stay behind pass q's FMAs: without the fence the
                // compiler hoists them and the kernel no longer fits 64 VGPRs (8 waves)
                asm volatile("" ::: "memory");
            }
        }
        // the remaining passes one at a time, each product kept or skipped by a select (the
        // reference's products exactly: a non-finite panel entry in a column a shorter row lacks
        // never reaches that row)
        for (; pb * NGW < wc; ++pb) {  // wave-uniform
            const int j = pb * NGW + g;
            const int cq = s_c[wave][j & 63];
            const double2 xv = *reinterpret_cast<const double2 *>(a.x + (size_t)cq * a.ld + 2 * c);
#pragma unroll
            for (int i = 0; i < KR; ++i) {
                const double v = s_v[wave][i][j & 63];
                const bool on = i < h && j < blk_len(d, i);
                acc[i].x += on ? v * xv.x : 0.0;
                acc[i].y += on ? v * xv.y : 0.0;
            }
        }
        const double2 row = rows8_sum2<GL>(acc);
        if (store) {
            *reinterpret_cast<double2 *>(a.y + (size_t)(r0 + rofs + ri) * a.ld + 2 * c) = row;
            if (MODE == kModeDot) {
                dot.x += xx.x * row.x;
                dot.y += xx.y * row.y;
            }
        }
    }
    if constexpr (MODE == kModeDot) {
        if (stopped)
            return;
        // this tile's x.(Ax) per column: lanes of one column pair (equal c) over the wave, then
        // the waves in order; a plain store (k_fold_dot sums the tiles' partials in a later launch)
#pragma unroll
        for (int off = 32; off >= GL; off >>= 1) {
            dot.x += __shfl_xor(dot.x, off);
            dot.y += __shfl_xor(dot.y, off);
        }
        if (lane < GL)
            s_red2[tid >> 6][lane] = dot;
        __syncthreads();
        if (tid < GL) {
            double2 tsum = s_red2[0][tid];
#pragma unroll
            for (int w = 1; w < kBlock / 64; ++w) {
                tsum.x += s_red2[w][tid].x;
                tsum.y += s_red2[w][tid].y;
            }
            a.partials[(size_t)t * L + 2 * tid] = tsum.x;
            a.partials[(size_t)t * L + 2 * tid + 1] = tsum.y;
        }
    }
}

// Cache flush between cold calls: by default a READ sweep of a buffer larger than the L2s and
// the 256 MiB Infinity Cache, so the measured kernel finds its data evicted and the caches full
// of clean lines.  A write sweep (MSPMV_FLUSH=write, the first flush of every buffer) leaves them
// full of dirty lines instead, whose write-back the measured kernel then pays as it evicts them
// (measured: the cant-shaped SpMV 31.5 us after a write sweep against 15.5 us hot).
__global__ void k_flush(double *p, long long n, double v)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        p[i] = v;
}
// STREAM-like read of n2 16-byte words (the practical HBM ceiling the roofline is read against,
// SURVEY 8(d)): grid-stride, four nontemporal 16-B loads in flight per thread per step.
// The practical HBM read ceiling (bench `roofline.measured_read_GBps`): every workgroup streams ONE
// contiguous slice of the buffer with nontemporal 16-B loads, two register stages of 8 loads per
// lane in flight.  Measured on MI355X (tools/read_ceiling.hip, r03b), 1 GiB per launch: 6.89-6.90
// TB/s for this shape at 4 or 8 workgroups per CU, against 5.5-5.6 TB/s for the grid-stride loop
// used before (which every workgroup walks across the whole buffer) and 6.4-6.7 TB/s for LDS-DMA.
__global__ __launch_bounds__(kBlock) void k_stream_read(const double2 *p, long long n2, double *sink)
{
    constexpr int U = 8;
    const long long per = (n2 + gridDim.x - 1) / gridDim.x;
    const long long b = (long long)blockIdx.x * per;
    const long long e = b + per < n2 ? b + per : n2;
    const long long step = (long long)kBlock * U;
    auto ld = [&](long long i) { return i < e ? ld_stream<true>(p + i) : make_double2(0.0, 0.0); };
    double acc = 0.0;
    double2 t0[U], t1[U];
    long long i = b + threadIdx.x;
#pragma unroll
    for (int u = 0; u < U; ++u)
        t0[u] = ld(i + u * kBlock);
    for (i += step; i < e + step; i += 2 * step) {
#pragma unroll
        for (int u = 0; u < U; ++u)
            t1[u] = ld(i + u * kBlock);
#pragma unroll
        for (int u = 0; u < U; ++u)
            acc += t0[u].x + t0[u].y;
#pragma unroll
        for (int u = 0; u < U; ++u)
            t0[u] = ld(i + step + u * kBlock);
#pragma unroll
        for (int u = 0; u < U; ++u)
            acc += t1[u].x + t1[u].y;
    }
    if (acc == -1.0)  // never (the buffer holds zeros): keeps the loads live without a store
        *sink = acc;
}

hipError_t launch_stream_read(const double *p, size_t bytes, int num_cus, hipStream_t s)
{
    const long long n2 = (long long)(bytes / 16);
    hipLaunchKernelGGL(k_stream_read, dim3((unsigned)std::max(1, num_cus * 4)), dim3(kBlock), 0, s,
                       reinterpret_cast<const double2 *>(p), n2, const_cast<double *>(p));
    return hipGetLastError();
}

__global__ void k_flush_read(const double *p, long long n, double *sink)
{
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        acc += __builtin_nontemporal_load(p + i);
    if (acc == -1.0)  // never (the buffer holds +1.0): keeps the loads live without a store
        *sink = acc;
}

// ------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------

// Tuning.  The shipped values are the measured best; variants measured and not kept are listed in
// DESIGN.md with their session tags.  Two switches stay, each with a GPU parity test of both
// settings: MSPMV_SPMV_BLOCKS=0 (no node blocks in single-RHS plans; test_gpu_blocks.py) and
// MSPMV_SPMM_BLK=0 (multi-RHS products on their own L-wide tiles instead of the node-block SpMM;
// test_gpu_blocks.py, test_gpu_dist.py).  Read once per process.
constexpr int kSpmvIpt = 8;     // merge items per thread of the single-RHS tiles (tile = 256 x 8)
constexpr int kSpmvRgCost = 48; // k_tile_modes budget for single-RHS row-group tiles
struct Switches {
    bool blocks = true;
    bool spmm_blk = true;
};
static const Switches &switches()
{
    static const Switches w = [] {
        Switches v;
        if (const char *e = getenv("MSPMV_SPMV_BLOCKS"))
            v.blocks = atoi(e) != 0;
        if (const char *e = getenv("MSPMV_SPMM_BLK"))
            v.spmm_blk = atoi(e) != 0;
        return v;
    }();
    return w;
}

int spmv_items_per_thread() { return kSpmvIpt; }

// SpMM tile depth: measured best 8 items per lane group for L <= 4 (fem-blocked pwtk shape,
// L = 4: 55.6 vs 74.8 us at 16), 24 for L = 8 (nlpkkt120 shape, L = 8: 1,536-item tiles of ~55 stencil
// rows -- one round of the 64 row groups -- 439 us vs 467 at 16, 455 at 28, 550 at 32, r04ai; pwtk
// shape flat) and 32 for L = 16 (cant shape: 39.2 -> 28.0 us -- half the tile start-ups at 6
// workgroups per CU instead of 7, r04aa).
constexpr int spmm_iptg_for(int L) { return L >= 16 ? 32 : L >= 8 ? 24 : 8; }

// Resident workgroups per CU of a kBlock-thread kernel from its own resources on gfx950: 160 KiB
// of LDS per CU, 512 VGPRs per SIMD lane (granule 8), at most 8 waves per SIMD, 4 SIMDs.
static int gfx950_blocks_per_cu(const void *fn)
{
    hipFuncAttributes fa{};
    if (hipFuncGetAttributes(&fa, fn) != hipSuccess)
        return 0;
    const int waves_per_block = kBlock / 64;
    const int vgpr = std::max(8, (fa.numRegs + 7) & ~7);
    const int waves_simd = std::min(8, 512 / vgpr);
    int by_waves = 4 * waves_simd / waves_per_block;
    int by_lds = fa.sharedSizeBytes > 0 ? (int)(160 * 1024 / fa.sharedSizeBytes) : by_waves;
    return std::max(0, std::min(by_waves, by_lds));
}

// Slots of the striped single-RHS tile kernels: the SpMV and the pipelined CG (its form without node
// blocks; FEM plans run the node-block kernels, whose tile counts are not near a generation
// boundary), from the kernels' own LDS / VGPR use (the runtime's occupancy query is the fallback
// without attributes).
int spmv_tile_blocks_per_cu()
{
    static const int occ = [] {
        const void *ks = (const void *)k_spmv_tile<kSpmvIpt, kModeSpmv, false, kBlock, true, false>;
        const void *kc = (const void *)k_spmv_tile<kSpmvIpt, kModeCg, false, kBlock, false>;
        const int c = std::min(gfx950_blocks_per_cu(ks), gfx950_blocks_per_cu(kc));
        if (c > 0)
            return c;
        int a = 0, b = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_spmv_tile<kSpmvIpt, kModeSpmv, false, kBlock, true, false>,
                                                         kBlock, 0) !=
                hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_spmv_tile<kSpmvIpt, kModeCg, false, kBlock, false>,
                                                         kBlock, 0) != hipSuccess)
            return 0;
        return std::min(a, b);
    }();
    return occ;
}

int tile_items_for(int L)
{
    if (L == 1)
        return kBlock * kSpmvIpt;
    return (kBlock / (L / 2)) * spmm_iptg_for(L);
}

hipError_t launch_merge_coords(const int *d_row_offsets, int m, int nnz, long long diag_step, int num_parts,
                               int2 *d_out, hipStream_t s)
{
    const int n = num_parts + 1;
    hipLaunchKernelGGL(k_merge_coords, dim3((n + 255) / 256), dim3(256), 0, s, d_row_offsets, m, nnz, diag_step,
                       num_parts, d_out);
    return hipGetLastError();
}

hipError_t launch_pack_cols16(const int *d_cols, const int2 *d_bounds, int num_tiles, int *d_colbase,
                              unsigned short *d_cols16, hipStream_t s)
{
    hipLaunchKernelGGL(k_pack_cols16, dim3(num_tiles), dim3(kBlock), 0, s, d_cols, d_bounds, d_colbase, d_cols16);
    return hipGetLastError();
}

bool spmv_blocks_enabled() { return switches().blocks; }
bool spmm_blk_enabled() { return switches().spmm_blk; }

hipError_t launch_build_blocks(const int *d_row_offsets, const int *d_cols, const int2 *d_bounds,
                               const unsigned char *d_split, const int *d_colbase, int num_tiles, uint4 *d_blk,
                               hipStream_t s, int max_chunks)
{
    static_assert(kBlkMax == kBlkPerTile, "descriptor capacity");
    if (num_tiles <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_build_blocks, dim3((num_tiles + 127) / 128), dim3(128), 0, s, d_row_offsets, d_cols, d_bounds,
                       d_split, d_colbase, num_tiles, d_blk, max_chunks);
    return hipGetLastError();
}

hipError_t launch_fill_pcols(const uint4 *d_blk, int blk_stride, const int2 *d_bounds,
                             const unsigned short *d_cols16, int num_tiles, unsigned short *d_pcols, hipStream_t s)
{
    if (num_tiles <= 0)
        return hipSuccess;
    const long long slots = (long long)num_tiles * blk_stride;  // blk_stride is a multiple of kBlock / 64
    hipLaunchKernelGGL(k_fill_pcols, dim3((unsigned)(slots / (kBlock / 64))), dim3(kBlock), 0, s, d_blk, blk_stride,
                       d_bounds, d_cols16, num_tiles, d_pcols);
    return hipGetLastError();
}

hipError_t launch_fill_recs(const uint4 *d_blk, int blk_stride, const unsigned short *d_pcols, int num_tiles,
                            unsigned *d_recs, int *d_counts, hipStream_t s)
{
    if (num_tiles <= 0)
        return hipSuccess;
    const long long slots = (long long)num_tiles * blk_stride;
    hipLaunchKernelGGL(k_fill_recs, dim3((unsigned)((slots + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d_blk,
                       blk_stride, d_pcols, num_tiles, d_recs, d_counts);
    return hipGetLastError();
}

// multi: an L-wide plan (dictionaries of at most spmm_dict_max(L) entries: what its kernel parks in
// LDS; the kernel checks the limit again)
hipError_t launch_build_dict(const int *d_cols, const int2 *d_bounds, int num_tiles, int max_items, int *d_dict,
                             int *d_ndict, unsigned short *d_idx16, hipStream_t s, bool multi, int L)
{
    const int ratio = multi ? -1 : 1;
    const int dmax = multi ? spmm_dict_max(L) : 1 << 30;
    if (max_items <= 4096)
        hipLaunchKernelGGL(k_build_dict<4096>, dim3(num_tiles), dim3(kBlock), 0, s, d_cols, d_bounds, d_dict, d_ndict,
                           d_idx16, ratio, dmax);
    else if (max_items <= 8192)
        hipLaunchKernelGGL(k_build_dict<8192>, dim3(num_tiles), dim3(kBlock), 0, s, d_cols, d_bounds, d_dict, d_ndict,
                           d_idx16, ratio, dmax);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_snap(const int *d_row_offsets, int m, int2 *d_bounds, unsigned char *d_split, int num_tiles,
                       int snap, hipStream_t s)
{
    const int n = num_tiles + 1;
    hipLaunchKernelGGL(k_snap, dim3((n + 255) / 256), dim3(256), 0, s, d_row_offsets, m, d_bounds, d_split,
                       num_tiles, snap);
    return hipGetLastError();
}

hipError_t launch_tile_modes(const int *d_row_offsets, const int2 *d_bounds, const unsigned char *d_split,
                             int num_tiles, int L, unsigned char *d_modes, hipStream_t s, int lanes_in)
{
    if (num_tiles == 0)
        return hipSuccess;
    // SpMM budget: twice the walk's gather chunks (4 steps each) plus its search
    const int cost = L == 1 ? kSpmvRgCost : 2 * (4 * (spmm_iptg_for(L) / 4) + 2);
    const int lanes = L == 1 ? lanes_in : kBlock;  // threads sharing one tile
    hipLaunchKernelGGL(k_tile_modes, dim3((num_tiles + 255) / 256), dim3(256), 0, s, d_row_offsets, d_bounds, d_split,
                       num_tiles, L == 1 ? 1 : L / 2, cost, lanes, d_modes);
    return hipGetLastError();
}

static TileArgs make_args(const mspmv_handle_s *h, const TilePlan &plan, const double *X, double *Y, int L)
{
    TileArgs a{};
    a.row_offsets = h->d_row_offsets;
    a.m = h->m;
    a.cols = h->d_cols;
    a.vals = h->d_vals;
    a.x = X;
    a.xr = X;
    a.y = Y;
    a.bounds = plan.d_bounds;
    a.split = plan.d_split;
    a.rmode = plan.d_modes[l_index(L)];
    a.carry_val = plan.d_carry_val;
    a.fix = plan.num_carries ? plan.d_fix : nullptr;  // split rows: closed by the tile kernels
    a.fix_cnt = plan.d_fix_cnt;
    a.fault = h->d_fault;
    a.head_val = plan.d_carry_val + (size_t)std::max(plan.num_tiles, 1) * plan.carry_L;
    a.head_pub = a.head_val + (size_t)std::max(plan.num_tiles, 1) * plan.carry_L;
    a.num_tiles = plan.num_tiles;
    if (L == 1 || plan.d_blk) {  // L > 1 on a node-block plan: k_spmm_blk (plan_for_L picked it)
        a.colbase = plan.d_colbase;
        a.cols16 = plan.d_cols16;
        a.blk = plan.d_blk;
        a.blk_stride = plan.blk_stride;
        a.pcols = plan.d_pcols;
        a.recs = plan.d_recs;
        // L > 1 runs the node-block plan only while k_spmm_blk is enabled (all_node_blocks' gate, mspmv_plan.hip): L = 2
        // shares the single-RHS tile size, so without this the switched-off plan would still be all-reg
        a.all_reg = plan.d_blk && plan.num_tiles_reg == plan.num_tiles && (L == 1 || spmm_blk_enabled());
        a.blk_spmv = L == 1 && plan.blk_spmv;
        a.blk_rows_max = plan.blk_rows_max;
    }
    a.dict = plan.d_dict;
    a.ndict = plan.d_ndict;
    a.idx16 = plan.d_idx16;
    a.ld = L;
    a.early_re = L == 1 ? 1 : 0;
    a.tb = L == 1 ? plan.lanes : kBlock;
    a.n = h->n;
    return a;
}

// Which tile-kernel instantiation a launch runs: decided once, by pick_tile_kernel; launch_tile launches from it
// and tile_kernel_name spells it.  Fields a kernel has no argument for keep the values set here.
enum TileKind : int { kTileNone, kSpmvTile, kSpmvBlk, kSpmmTile, kSpmmBlk };
struct TileKernel {
    TileKind kind;       // kTileNone: no kernel (the pipelined CG's mode exists for L == 1 only)
    int L, mode;
    bool nt;
    int tb = kBlock;     // k_spmv_tile TB: threads sharing a tile
    bool blk = true;     // k_spmv_tile BLK: node-block staging compiled in
    bool fix = true;     // k_spmv_tile / k_spmm_tile FIX: close_split_rows compiled in
    bool dict = false;   // k_spmm_tile DICT
    bool fb = false;     // k_spmv_blk FB: the register fallback for tiles that are no register run tiles
    int kr = kBlkRows;   // k_spmv_blk / k_spmm_blk KR: rows of values a lane holds per run
};

static TileKernel pick_tile_kernel(const TileArgs &a, int L, int mode, bool nt)
{
    TileKernel k{kTileNone, L, mode, nt};
    if (mode == kModeCg && L != 1)
        return k;
    if (L == 1) {
        if (mode == kModeSpmv && a.blk_spmv) {
            // a node-block plan (every tile, or most: the rest run the kernel's register fallback):
            // the LDS-free kernel, column pairs, runs of <= 6 rows
            k.kind = kSpmvBlk;
            k.kr = 6;
            k.fb = !a.all_reg;  // every tile a register run tile: no register fallback compiled in
        } else if (mode == kModeDot && a.all_reg) {
            k.kind = kSpmvBlk;  // every tile a register node-block tile, dot mode (the row-sharded CG): column owners
        } else {
            k.kind = kSpmvTile;
            if (mode == kModeSpmv && a.tb == 64)  // one-wave tiles (skewed rows, spmv_plan)
                k.tb = 64;
            else if (mode == kModeCg && !a.blk)  // the pipelined CG without node blocks: fewer VGPRs
                k.blk = false;
            else if (mode == kModeSpmv && !a.fix)  // no split rows: the form without close_split_rows
                k.fix = false;
        }
    } else if (a.all_reg) {  // a node-block plan (single-RHS tiles): every tile a register run tile
        k.kind = kSpmmBlk;
        k.kr = a.blk_rows_max <= 6 ? 6 : kBlkRows;
    } else {
        k.kind = kSpmmTile;
        k.dict = spmm_dict_max(L) > 0 && a.dict;  // plans with column dictionaries (L = 16; L = 8 when enabled)
        k.fix = k.dict || mode != kModeSpmv || a.fix;  // no split rows: the form without close_split_rows
    }
    return k;
}

// The kernel as rocprofv3 lists it.  (k_spmv_tile's trailing STAMP is left to its default, as the recorded
// profiles and bench.py's attribution spell it.)
static std::string tile_kernel_name(const TileKernel &k)
{
    auto b = [](bool v) { return v ? ",true" : ",false"; };
    auto i = [](int v) { return "," + std::to_string(v); };
    const std::string L = std::to_string(k.L), mode_nt = i(k.mode) + b(k.nt);
    switch (k.kind) {
    case kSpmvTile: return "k_spmv_tile<" + std::to_string(kSpmvIpt) + mode_nt + i(k.tb) + b(k.blk) + b(k.fix) + ">";
    case kSpmvBlk: return "k_spmv_blk<" + std::to_string(k.mode) + b(k.nt) + i(k.kr) + b(k.fb) + ">";
    case kSpmmTile: return "k_spmm_tile<" + L + i(spmm_iptg_for(k.L)) + mode_nt + b(k.dict) + b(k.fix) + ">";
    case kSpmmBlk: return "k_spmm_blk<" + L + mode_nt + i(k.kr) + ">";
    default: return "";
    }
}

// One instantiation each: launched when it is the one k names (false: it is not).
template <int MODE, bool NT, int TB, bool BLK, bool FIX>
static bool run_spmv_tile(const TileKernel &k, const TileArgs &a, hipStream_t s)
{
    if (k.kind != kSpmvTile || k.tb != TB || k.blk != BLK || k.fix != FIX)
        return false;
    ggl(k_spmv_tile<kSpmvIpt, MODE, NT, TB, BLK, FIX>, dim3(a.num_tiles), dim3(TB), s, a);
    return true;
}
template <int MODE, bool NT, int KR, bool FB>
static bool run_spmv_blk(const TileKernel &k, const TileArgs &a, hipStream_t s)
{
    if (k.kind != kSpmvBlk || k.kr != KR || k.fb != FB)
        return false;
    ggl(k_spmv_blk<MODE, NT, KR, FB>, dim3(a.num_tiles), dim3(kBlock), s, a);
    return true;
}
template <int LL, int MODE, bool NT, bool DICT, bool FIX>
static bool run_spmm_tile(const TileKernel &k, const TileArgs &a, hipStream_t s)
{
    if (k.kind != kSpmmTile || k.dict != DICT || k.fix != FIX)
        return false;
    ggl(k_spmm_tile<LL, spmm_iptg_for(LL), MODE, NT, DICT, FIX>, dim3(a.num_tiles), dim3(kBlock), s, a);
    return true;
}
template <int LL, int MODE, bool NT, int KR>
static bool run_spmm_blk(const TileKernel &k, const TileArgs &a, hipStream_t s)
{
    if (k.kind != kSpmmBlk || k.kr != KR)
        return false;
    ggl(k_spmm_blk<LL, MODE, NT, KR>, dim3(a.num_tiles), dim3(kBlock), s, a);
    return true;
}

// The instantiations that exist for (MODE, LL, NT), each tried against the pick: a pick outside them launches
// nothing and is an error, never another kernel.
template <int MODE, int LL, bool NT>
static bool launch_picked(const TileKernel &k, const TileArgs &a, hipStream_t s)
{
    bool ok = false;
    if constexpr (LL == 1) {  // k_spmv_tile<.., TB, BLK, FIX>, k_spmv_blk<.., KR, FB>
        ok = run_spmv_tile<MODE, NT, kBlock, true, true>(k, a, s);
        if constexpr (MODE == kModeSpmv)
            ok = ok || run_spmv_tile<MODE, NT, kBlock, true, false>(k, a, s) ||
                 run_spmv_tile<MODE, NT, 64, true, true>(k, a, s) || run_spmv_blk<MODE, NT, 6, false>(k, a, s) ||
                 run_spmv_blk<MODE, NT, 6, true>(k, a, s);
        if constexpr (MODE == kModeCg)
            ok = ok || run_spmv_tile<MODE, NT, kBlock, false, true>(k, a, s);
        if constexpr (MODE == kModeDot)
            ok = ok || run_spmv_blk<MODE, NT, kBlkRows, false>(k, a, s);
    } else if constexpr (MODE != kModeCg) {  // k_spmm_tile<.., DICT, FIX>, k_spmm_blk<.., KR>
        ok = run_spmm_tile<LL, MODE, NT, false, true>(k, a, s) || run_spmm_blk<LL, MODE, NT, 6>(k, a, s) ||
             run_spmm_blk<LL, MODE, NT, kBlkRows>(k, a, s);
        if constexpr (MODE == kModeSpmv)
            ok = ok || run_spmm_tile<LL, MODE, NT, false, false>(k, a, s);
        if constexpr (spmm_dict_max(LL) > 0)  // plans with column dictionaries (L = 16; L = 8 when enabled)
            ok = ok || run_spmm_tile<LL, MODE, NT, true, true>(k, a, s);
    }
    return ok;
}

template <int MODE>
static hipError_t launch_tile(const TileArgs &a, int L, hipStream_t s, bool nt)
{
    const TileKernel k = pick_tile_kernel(a, L, MODE, nt);
    return dispatch_L(L, [&](auto Lc) {
        const bool ok = dispatch_bool(nt, [&](auto ntc) {
            return launch_picked<MODE, decltype(Lc)::value, decltype(ntc)::value>(k, a, s);
        });
        return ok ? hipGetLastError() : hipErrorInvalidValue;
    });
}

// Diagnostic: the plain single-RHS SpMV of a plan that runs k_spmv_tile on 256-thread workgroups, in its
// stamped instantiation (mspmv_spmv_tile_stamps).  hipErrorNotSupported for plans that run another kernel.
hipError_t launch_spmv_tile_stamped(mspmv_handle_s *h, const TilePlan &plan, const double *d_x, double *d_y,
                                   unsigned long long *d_stamps)
{
    TileArgs a = make_args(h, plan, d_x, d_y, 1);
    if (a.blk_spmv || a.tb == 64 || plan.dia || plan.slab)
        return hipErrorNotSupported;
    a.stamps = d_stamps;
    const dim3 grid(a.num_tiles), block(kBlock);
    if (plan.num_tiles == 0)
        return hipSuccess;
    const bool nt = stream_nt(h);
    dispatch_bool(nt, [&](auto ntc) {
        constexpr bool NT = decltype(ntc)::value;
        if (!a.fix)
            ggl(k_spmv_tile<kSpmvIpt, kModeSpmv, NT, kBlock, true, false, true>, grid, block, h->stream, a);
        else
            ggl(k_spmv_tile<kSpmvIpt, kModeSpmv, NT, kBlock, true, true, true>, grid, block, h->stream, a);
    });
    return hipGetLastError();
}

hipError_t launch_spmm_tile_only(mspmv_handle_s *h, const TilePlan &plan, const double *d_X, double *d_Y, int L,
                                 int ld, CgControl *ctrl)
{
    if (plan.num_tiles == 0)
        return hipSuccess;
    if (plan.dia)  // offset windows: every width on one plan
        return launch_dia(h, plan, d_X, d_Y, L, ld, ctrl);
    if (plan.slab) {  // a column-slab plan: the plain SpMV's (spmv_plan) or an L-wide SpMM's (product_plan)
        if (plan.slab->L != L || (L == 1 && ctrl))  // (the slab SpMV takes no control word)
            return hipErrorInvalidValue;
        return L == 1 ? launch_slab(h, plan, d_X, d_Y) : launch_slab_mm(h, plan, d_X, d_Y, L, ld, ctrl);
    }
    TileArgs a = make_args(h, plan, d_X, d_Y, L);
    if (ld > 0)
        a.ld = ld;
    if (ctrl) {  // a CG's product: stopped by the control word, faults into the solve's word
        a.ctrl = ctrl;
        a.fault = &ctrl->fault;
    }
    return launch_tile<kModeSpmv>(a, L, h->stream, stream_nt(h));
}

// The kernel launch_spmm_tile_only launches for a product of native width L on `plan`, as rocprofv3 lists it:
// its three steps, each name formatted from the pick its launcher launches from.
std::string product_kernel_name(const mspmv_handle_s *h, const TilePlan &plan, int L)
{
    if (plan.dia)
        return dia_kernel_name(pick_dia(h, L, false));
    if (plan.slab)
        return L == 1 ? slab_kernel_name(pick_slab(h, plan)) : slab_mm_kernel_name(pick_slab_mm(h, plan));
    return tile_kernel_name(pick_tile_kernel(make_args(h, plan, nullptr, nullptr, L), L, kModeSpmv, stream_nt(h)));
}

// The pipelined single-RHS CG's SpMV (iteration `parity`) on the tiles of `plan` (k_spmv_tile MODE 1;
// launch_cg1_dia's twin): reads {r_k, p_{k-1}} from rp_old, writes p_k into rp_new, Ap into h->d_ap, the
// deferred x term into d_x and one p.Ap partial per tile into h->d_partials (*nslots of them); sums the
// nblk r.r partials of the update before it.
hipError_t launch_cg1_tile(mspmv_handle_s *h, const TilePlan &plan, const double *rp_old, double *rp_new, double *d_x,
                           int parity, int nblk, double tol, int *nslots)
{
    TileArgs ta = make_args(h, plan, rp_old, h->d_ap, 1);
    ta.p_new = rp_new;
    ta.xsol = d_x;
    ta.scal = h->d_scal;
    ta.ctrl = h->d_ctrl;
    ta.fault = &h->d_ctrl->fault;
    ta.partials = h->d_partials;
    ta.gtickets = h->d_gtickets;
    ta.part_in = h->d_partials_b;
    ta.n_part_in = nblk;
    ta.parity = parity;
    ta.tol = tol;
    ta.hist = h->d_hist;
    ta.hist_cap = h->hist_cap;
    *nslots = plan.num_tiles;
    return launch_tile<kModeCg>(ta, 1, h->stream, stream_nt(h));
}

// Column block copy between row-major panels: dst[i][j] = (j < cols ? src[i][j] : 0) for
// j < dcols (dcols > cols: the zero column of an odd-L panel padded to even width).  Gathers a
// column group out of a wider panel, scatters it back, pads and unpads.
__global__ void k_panel_copy(const double *__restrict__ src, int lds, double *__restrict__ dst, int ldd,
                             long long rows, int cols, int dcols)
{
    const long long total = rows * dcols;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        const long long i = e / dcols;
        const int j = (int)(e - i * dcols);
        dst[i * ldd + j] = j < cols ? src[i * lds + j] : 0.0;
    }
}

hipError_t launch_panel_copy(const double *src, int lds, double *dst, int ldd, long long rows, int cols, int dcols,
                             hipStream_t s)
{
    const long long total = rows * dcols;
    if (total <= 0)
        return hipSuccess;
    const long long b = std::min<long long>((total + kBlock - 1) / kBlock, 8192);
    hipLaunchKernelGGL(k_panel_copy, dim3((unsigned)b), dim3(kBlock), 0, s, src, lds, dst, ldd, rows, cols, dcols);
    return hipGetLastError();
}

hipError_t launch_spmm(mspmv_handle_s *h, const TilePlan &plan, const double *d_X, double *d_Y, int L,
                       int *kernels_launched, int ld)
{
    const hipError_t e = launch_spmm_tile_only(h, plan, d_X, d_Y, L, ld);
    if (kernels_launched)
        *kernels_launched = plan.num_tiles ? 1 : 0;
    return e;
}

// The dot-mode SpMM's tile kernel on stream s: Y = A X and one x.(AX) partial per tile
// at partials[t * L ..] (plain stores, summed by launch_fold_dot in a later launch).
hipError_t launch_spmm_dot_tiles(mspmv_handle_s *h, const TilePlan &plan, const double *d_X, double *d_Y, int L,
                                 CgControl *ctrl, double *partials, hipStream_t s, long long row_off)
{
    if (plan.num_tiles == 0)
        return hipSuccess;
    TileArgs ta = make_args(h, plan, d_X, d_Y, L);
    ta.xr = d_X + row_off * L;  // the handle's rows start at row row_off of X
    ta.ctrl = ctrl;
    ta.fault = ctrl ? &ctrl->fault : h->d_fault;
    ta.partials = partials;
    return launch_tile<kModeDot>(ta, L, s, stream_nt(h));
}

// Cold-cache flush between timed launches: a read sweep (caches left holding clean unrelated lines;
// a write sweep left them dirty and the timed kernel paid the write-back: cant 35.1 vs 19.2 us, r02n).
hipError_t launch_flush(void *p, size_t bytes, hipStream_t s, bool fresh)
{
    const long long n = (long long)(bytes / sizeof(double));
    if (fresh)
        hipLaunchKernelGGL(k_flush, dim3(2048), dim3(256), 0, s, (double *)p, n, 1.0);
    else
        hipLaunchKernelGGL(k_flush_read, dim3(2048), dim3(256), 0, s, (const double *)p, n, (double *)p);
    return hipGetLastError();
}

}  // namespace mspmv

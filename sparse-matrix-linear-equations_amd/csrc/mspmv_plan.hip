// mspmv_plan.hip -- building tile plans and choosing the plan a product or a solver runs on: the merge-path
// tile plan and its single-RHS extras (build_plan), the optional plans the plain product may take instead
// (offset windows, column slabs / sliced ELL, one-wave tiles, run-balanced node blocks, slab-MM) and the order
// they are tried in.  Two questions are asked of it: product_plan (the plain y = A x / Y = A X) and solver_plan
// (CG, BiCGSTAB, dot-mode and sharded callers).  Host C++17 over the HIP runtime; no kernels.
#include "mspmv_internal.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

using namespace mspmv;

void mspmv::free_plan(TilePlan &p)
{
    dev_free(p.d_bounds);
    dev_free(p.d_split);
    for (auto &m : p.d_modes)
        dev_free(m);
    dev_free(p.d_fix);
    dev_free(p.d_fix_cnt);
    dev_free(p.d_carry_val);
    dev_free(p.d_colbase);
    dev_free(p.d_cols16);
    dev_free(p.d_dict);
    dev_free(p.d_ndict);
    dev_free(p.d_idx16);
    dev_free(p.d_blk);
    dev_free(p.d_pcols);
    dev_free(p.d_recs);
    free_slab(p.slab);
    p.slab = nullptr;
    free_dia(p.dia);
    p.dia = nullptr;
}

// Build (once) the tile plan for L right-hand sides, validating on the host every bound the
// kernels rely on (monotone boundaries, <= 1.25 * tile_items merge items per tile) before any
// tile kernel can run on it.
static mspmv_status build_plan(mspmv_handle_s *h, int L, const TilePlan **out, int lanes = 0,
                               const std::vector<int2> *fixed = nullptr);
// product_plan before it books the handle's cache lease
static mspmv_status product_plan_unbooked(mspmv_handle_s *h, int L, const TilePlan **out);

// The in-tile reduction modes of a plan for L right-hand sides, built on first use.
static mspmv_status ensure_modes(mspmv_handle_s *h, TilePlan &p, int L)
{
    unsigned char *&m = p.d_modes[l_index(L)];
    if (m)
        return MSPMV_OK;
    mspmv_status st = dev_alloc(&m, (size_t)std::max(p.num_tiles, 1));
    if (st != MSPMV_OK)
        return st;
    hipError_t e = launch_tile_modes(h->d_row_offsets, p.d_bounds, p.d_split, p.num_tiles, L, m, h->stream, p.lanes);
    if (e == hipSuccess)
        e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        set_error(std::string("tile modes: ") + hipGetErrorString(e));
        dev_free(m);
        m = nullptr;
        return MSPMV_ERR_HIP;
    }
    return MSPMV_OK;
}

// An on / off switch of the environment: -1 unset or empty, else 0 or 1.  Read at each handle's decision, never
// cached (the tests set the switches per matrix inside one process).
static int env_tristate(const char *name)
{
    const char *e = getenv(name);
    return e && *e ? (atoi(e) != 0 ? 1 : 0) : -1;
}

// The optional-plan rule: a plan the product could do without never fails it.  A builder's failure st is
// swallowed -- the error text and HIP's sticky error cleared, the tiles stay -- unless the plan's switch forced it
// and the failure is a real one (anything but "the matrix does not fit the form"), which goes through.
static mspmv_status optional_failed(mspmv_status st, bool forced)
{
    if (forced && st != MSPMV_ERR_UNSUPPORTED)
        return st;
    set_error("");
    (void)hipGetLastError();
    return MSPMV_OK;
}

// ... for a candidate p its builder returned st for: adopted under key (*decision = 1) when it was built, else
// freed and the failure handled as above.
static mspmv_status keep_optional(mspmv_handle_s *h, int key, TilePlan &p, mspmv_status st, bool forced, int *decision)
{
    if (st != MSPMV_OK) {
        free_plan(p);
        return optional_failed(st, forced);
    }
    h->plans.emplace(key, p);
    *decision = 1;
    return MSPMV_OK;
}

// Offset-window plan (mspmv_dia.hip) for the plain SpMV / SpMM of every width and the split CG's SpMM:
// taken when every 64-row window of the matrix lists its columns at <= kDiaMaxK common offsets col - row
// and the nonzeros fill >= kDiaAutoFill of the windows' rows x offsets overall (>= kDiaWindowFill in each
// window): structured-grid stencils, whose boundary planes miss a third of the offsets.  MSPMV_DIA=0
// never, =1 whenever every window fits at any fill; read at each handle's decision.
constexpr double kDiaAutoFill = 0.85;
constexpr double kDiaWindowFill = 0.3;

static mspmv_status dia_decide(mspmv_handle_s *h)
{
    h->dia = 0;
    const int sw = env_tristate("MSPMV_DIA");
    if (sw == 0)
        return MSPMV_OK;
    TilePlan p;
    const mspmv_status st = build_dia_plan(h, p, sw == 1 ? 0.0 : kDiaAutoFill, sw == 1 ? 0.0 : kDiaWindowFill);
    return keep_optional(h, kDiaPlanKey, p, st, sw == 1, &h->dia);
}

// The L-wide products take the windows too unless MSPMV_DIA_SPMM=0: with the offsets taken run by run
// through LDS they beat the merge tiles at every width on the stencil shapes (nlpkkt120 size L = 2 / 4 / 8
// / 16: 268 / 295 / 372 / 677 us against 336 / 375 / 441 / 753; parabolic_fem shape 10.5 / 13.5 / 19.2 /
// 37 against 15.4 / 16 / 21.8 / 37.5 us; configs[4]'s CG 0.786 -> 0.704 ms per iteration, r05x).
bool mspmv::dia_spmm_enabled()
{
    const char *e = getenv("MSPMV_DIA_SPMM");
    return !(e && *e && atoi(e) == 0);
}

// The offset-window plan for a product of width L when the handle takes one (deciding on first use),
// else null.
mspmv_status mspmv::window_plan(mspmv_handle_s *h, int L, const TilePlan **out)
{
    *out = nullptr;
    if (L > 1 && !dia_spmm_enabled())
        return MSPMV_OK;
    if (h->dia < 0)
        ST_TRY(dia_decide(h));
    if (h->dia == 1)
        *out = &h->plans.find(kDiaPlanKey)->second;
    return MSPMV_OK;
}

bool mspmv::host_pattern_resident(const mspmv_handle_s *h) { return h->pat_ro_ext || !h->pat_ro.empty(); }

mspmv_status mspmv::host_pattern(mspmv_handle_s *h, const int **ro, const int **ci)
{
    if (h->pat_ro_ext) {
        *ro = h->pat_ro_ext;
        *ci = h->pat_ci_ext;
        return MSPMV_OK;
    }
    if (h->pat_ro.empty()) {
        std::vector<int> r((size_t)h->m + 1), c((size_t)std::max(h->nnz, 1));
        HIP_TRY(hipMemcpy(r.data(), h->d_row_offsets, sizeof(int) * r.size(), hipMemcpyDeviceToHost));
        if (h->nnz)
            HIP_TRY(hipMemcpy(c.data(), h->d_cols, sizeof(int) * (size_t)h->nnz, hipMemcpyDeviceToHost));
        h->pat_ro.swap(r);
        h->pat_ci.swap(c);
    }
    *ro = h->pat_ro.data();
    *ci = h->pat_ci.data();
    return MSPMV_OK;
}

namespace mspmv {
// Split rows of a plan (boundaries hb, split flags hs; p.num_tiles set): the tiles t0 .. t1 - 1 that
// end inside one row carry into the tile t1 that completes it (the first tile after them with no
// carry into the same row; the last tile always ends on m) -- TilePlan::d_fix / d_fix_cnt, closed by
// close_split_rows.  No arrays when nothing is split.
mspmv_status plan_split_rows(TilePlan &p, const std::vector<int2> &hb, const std::vector<unsigned char> &hs)
{
    const int T = p.num_tiles;
    std::vector<int4> fix((size_t)T, make_int4(-1, 0, 0, 0));
    int carries = 0;
    for (int t = 0; t < T;) {
        if (!hs[(size_t)t + 1]) {
            ++t;
            continue;
        }
        const int t0 = t;
        while (t < T && hs[(size_t)t + 1] && hb[(size_t)t + 1].x == hb[(size_t)t0 + 1].x)
            ++t;
        if (t >= T) {
            set_error("tile plan: split row past the last tile");
            return MSPMV_ERR_INVALID;
        }
        for (int u = t0; u < t; ++u) {
            fix[(size_t)u].x = t;
            fix[(size_t)u].y = t - t0;
        }
        fix[(size_t)t].z = t - t0;
        carries += t - t0;
    }
    p.num_carries = carries;
    if (carries == 0)
        return MSPMV_OK;
    mspmv_status st;
    if ((st = dev_alloc(&p.d_fix, (size_t)T)) != MSPMV_OK || (st = dev_alloc(&p.d_fix_cnt, (size_t)T)) != MSPMV_OK)
        return st;
    hipError_t e = hipMemcpy(p.d_fix, fix.data(), sizeof(int4) * fix.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = memset_sync(p.d_fix_cnt, 0, sizeof(unsigned) * T);
    if (e != hipSuccess) {
        set_error(std::string("tile plan upload: ") + hipGetErrorString(e));
        return MSPMV_ERR_HIP;
    }
    return MSPMV_OK;
}
}  // namespace mspmv

static mspmv_status build_plan(mspmv_handle_s *h, int L, const TilePlan **out, int lanes,
                               const std::vector<int2> *fixed)
{
    // lanes: 64 builds the one-wave single-RHS plan (tile = 64 x items per thread, keyed by minus
    // that size); 0 the default plan for L.  fixed: the run-balanced single-RHS plan's boundaries
    // (whole rows, no split; spmv_run_plan), keyed kRunPlanKey -- run by the node-block SpMV only,
    // whose tiles have no LDS item bound
    const bool onewave = L == 1 && lanes == 64;
    const int tile = onewave ? 64 * spmv_items_per_thread() : tile_items_for(L);
    TilePlan p;
    p.lanes = onewave ? 64 : kBlock;
    const long long total = (long long)h->m + h->nnz;
    int step = tile, snap = tile / kSnapDiv;
    if (L == 1 && !onewave) {
        // A grid a few tiles over a whole number of resident generations of workgroups takes one
        // tile lifetime more (the parabolic_fem shape: 2,052 tiles on 2,048 slots).  Stretch the
        // tiles into the snap slack so they fit one generation fewer: MAXI (step + snap) is
        // unchanged, rows entered by more than the smaller snap distance stay split (carries,
        // close_split_rows).  (Measured against nominal tiles in round 3: kept.)
        const long long slots = (long long)h->num_cus * spmv_tile_blocks_per_cu();
        const long long t0 = (total + tile - 1) / tile;
        // Below one generation (cant: 1,988 tiles on 2,048 slots; rma10: 1,183) the nominal tiles stay: cut
        // into exactly one tile per slot they measured the same (r06e).
        if (slots > 0 && t0 > slots) {
            const long long fewer = (t0 + slots - 1) / slots - 1;  // generations after stretching
            const long long fit = (total + fewer * slots - 1) / (fewer * slots);
            if (fit + 16 <= tile + tile / kSnapDiv) {
                step = (int)fit;
                snap = tile + tile / kSnapDiv - step;  // >= 16
            }
        }
    }
    if (fixed) {
        int most = 0;
        for (size_t t = 0; t + 1 < fixed->size(); ++t)
            most = std::max(most, ((*fixed)[t + 1].x - (*fixed)[t].x) + ((*fixed)[t + 1].y - (*fixed)[t].y));
        step = most;
        snap = 0;
    }
    p.tile_items = step;
    p.snap = snap;
    p.num_tiles = fixed ? (int)fixed->size() - 1 : (int)((total + step - 1) / step);
    const int T = p.num_tiles;
    mspmv_status st;
    if ((st = dev_alloc(&p.d_bounds, (size_t)T + 1)) != MSPMV_OK ||
        (st = dev_alloc(&p.d_split, (size_t)T + 1)) != MSPMV_OK ||
        (st = dev_alloc(&p.d_carry_val, (size_t)std::max(T, 1) * 16 * 3)) != MSPMV_OK) {  // carries, heads x 2
        free_plan(p);
        return st;
    }
    p.carry_L = 16;
    auto fail = [&](mspmv_status s) {
        free_plan(p);
        return s;
    };
    hipError_t e = hipSuccess;
    if (fixed) {
        e = hipMemcpyAsync(p.d_bounds, fixed->data(), sizeof(int2) * (T + 1), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess)
            e = hipMemsetAsync(p.d_split, 0, (size_t)T + 1, h->stream);
    } else {
        e = launch_merge_coords(h->d_row_offsets, h->m, h->nnz, step, T, p.d_bounds, h->stream);
        if (e == hipSuccess)
            e = launch_snap(h->d_row_offsets, h->m, p.d_bounds, p.d_split, T, p.snap, h->stream);
    }
    std::vector<int2> hb((size_t)T + 1);
    std::vector<unsigned char> hs((size_t)T + 1);
    if (e == hipSuccess)
        e = hipMemcpyAsync(hb.data(), p.d_bounds, sizeof(int2) * (T + 1), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(hs.data(), p.d_split, T + 1, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        set_error(std::string("tile plan: ") + hipGetErrorString(e));
        return fail(MSPMV_ERR_HIP);
    }
    const int maxi = fixed ? step : tile + tile / kSnapDiv;
    if (hb[0].x != 0 || hb[0].y != 0 || hb[T].x != h->m || hb[T].y != h->nnz) {
        set_error("tile plan: bad end boundaries");
        return fail(MSPMV_ERR_INVALID);
    }
    for (int t = 0; t < T; ++t) {
        const int nr = hb[t + 1].x - hb[t].x, nz = hb[t + 1].y - hb[t].y;
        if (nr < 0 || nz < 0 || nr + nz > maxi) {
            set_error("tile plan: tile " + std::to_string(t) + " violates the merge bound");
            return fail(MSPMV_ERR_INVALID);
        }
    }
    if ((st = plan_split_rows(p, hb, hs)) != MSPMV_OK)
        return fail(st);
    // the single-RHS kernels' 16-bit column stream; keyed on the tile size, not L, because the
    // L = 2 SpMM shares the single-RHS plan.  (The SpMM itself keeps int32 columns: it is gather
    // bound, and the 16-bit stream measured 0% at L = 4/8 and 7% slower at L = 16.)
    const bool single = L == 1;  // a single-RHS plan
    if (single && T > 0 && h->nnz > 0) {
        if ((st = dev_alloc(&p.d_colbase, (size_t)T)) != MSPMV_OK ||
            (st = dev_alloc(&p.d_cols16, (size_t)h->nnz + kNnzPad)) != MSPMV_OK)
            return fail(st);
        e = hipMemsetAsync(p.d_cols16, 0, sizeof(unsigned short) * ((size_t)h->nnz + kNnzPad), h->stream);
        if (e == hipSuccess)
            e = launch_pack_cols16(h->d_cols, p.d_bounds, T, p.d_colbase, p.d_cols16, h->stream);
        std::vector<int> hbase((size_t)T);
        if (e == hipSuccess)
            e = hipMemcpyAsync(hbase.data(), p.d_colbase, sizeof(int) * T, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            set_error(std::string("16-bit columns: ") + hipGetErrorString(e));
            return fail(MSPMV_ERR_HIP);
        }
        for (int b : hbase)
            p.num_tiles16 += b >= 0;
        if (p.num_tiles16 == 0) {  // nothing fits: keep the plan on int32 columns only
            dev_free(p.d_colbase);
            dev_free(p.d_cols16);
            p.d_colbase = nullptr;
            p.d_cols16 = nullptr;
        }
    }
    // node blocks: single-RHS plan on the 16-bit stream only (the runs' pattern columns are read there)
    if (single && !onewave && p.d_cols16 && spmv_blocks_enabled()) {
        if ((st = dev_alloc(&p.d_blk, (size_t)T * kBlkPerTile)) != MSPMV_OK)
            return fail(st);
        e = launch_build_blocks(h->d_row_offsets, h->d_cols, p.d_bounds, p.d_split, p.d_colbase, T, p.d_blk,
                                h->stream, kBlkPlanChunks);
        std::vector<uint4> hd((size_t)T * kBlkPerTile);
        if (e == hipSuccess)
            e = hipMemcpyAsync(hd.data(), p.d_blk, sizeof(uint4) * hd.size(), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            set_error(std::string("node blocks: ") + hipGetErrorString(e));
            return fail(MSPMV_ERR_HIP);
        }
        p.h_blk_reg.assign((size_t)T, 0);
        int maxnd = 0, maxh = 0;
        std::vector<unsigned char> reg((size_t)T, 0);
        for (int t = 0; t < T; ++t) {
            const uint4 *d = &hd[(size_t)t * kBlkPerTile];
            const int nd = (int)((d[0].y >> 8) & 255u);
            if (nd == 0)
                continue;
            ++p.num_tiles_blk;
            maxnd = std::max(maxnd, nd);
            for (int i = 0; i < nd; ++i)
                maxh = std::max(maxh, (int)(d[i].y & 15u));
            bool one = true;  // the kernels' own test: every chunk starts at pattern column 0
            for (int i = 0; i < nd; ++i)
                one = one && ((d[i].x >> 16) & 255u) == 0;
            reg[(size_t)t] = one;
            p.num_tiles_reg += one;
        }
        // the plain SpMV runs the column-pair node-block kernel (its register fallback taking the
        // other tiles) when most tiles are register run tiles; otherwise k_spmv_tile, whose register
        // path takes the run tiles of one round (<= kBlkTileChunks chunks)
        p.blk_spmv = p.num_tiles_reg > 0 && 2LL * p.num_tiles_reg >= T;
        for (int t = 0; t < T; ++t) {
            const int nd = (int)((hd[(size_t)t * kBlkPerTile].y >> 8) & 255u);
            p.h_blk_reg[(size_t)t] = p.blk_spmv || (reg[(size_t)t] && nd <= kBlkTileChunks);
            p.blk_two_rounds += nd > kBlkTileChunks;
        }
        dev_free(p.d_blk);
        p.d_blk = nullptr;
        p.blk_rows_max = maxh > 0 ? maxh : 8;
        if (p.num_tiles_blk > 0) {  // repack at the smallest stride that holds every tile's set
            p.blk_stride = maxnd <= 8 ? 8 : maxnd <= 16 ? 16 : maxnd <= 32 ? 32 : 64;
            std::vector<uint4> packed((size_t)T * p.blk_stride, make_uint4(0u, 0u, 0u, 0u));
            for (int t = 0; t < T; ++t)
                for (int i = 0, nd = (int)((hd[(size_t)t * kBlkPerTile].y >> 8) & 255u); i < nd; ++i)
                    packed[(size_t)t * p.blk_stride + i] = hd[(size_t)t * kBlkPerTile + i];
            if ((st = dev_alloc(&p.d_blk, packed.size())) != MSPMV_OK)
                return fail(st);
            if (hipMemcpy(p.d_blk, packed.data(), sizeof(uint4) * packed.size(), hipMemcpyHostToDevice) != hipSuccess) {
                set_error("node blocks: upload failed");
                return fail(MSPMV_ERR_HIP);
            }
            // the chunks' pattern columns once more, one 128-B slot per descriptor slot (hipMalloc aligns
            // the array to more than a line): the kernels read a run's columns there, not in cols16
            const size_t np = packed.size() * 64;
            if ((st = dev_alloc(&p.d_pcols, np)) != MSPMV_OK)
                return fail(st);
            e = hipMemsetAsync(p.d_pcols, 0, sizeof(unsigned short) * np, h->stream);
            if (e == hipSuccess)
                e = launch_fill_pcols(p.d_blk, p.blk_stride, p.d_bounds, p.d_cols16, T, p.d_pcols, h->stream);
            if (e == hipSuccess)
                e = hipStreamSynchronize(h->stream);
            if (e != hipSuccess) {
                set_error(std::string("node blocks: pattern-column slots: ") + hipGetErrorString(e));
                return fail(MSPMV_ERR_HIP);
            }
            // descriptor and pattern once more as one 64-B record per descriptor slot, which is all the
            // column-pair SpMV reads of a run (blk_rec_encode)
            int *d_counts = nullptr;
            int counts[2] = {0, 0};
            if ((st = dev_alloc(&p.d_recs, packed.size() * kRecDwords)) != MSPMV_OK)
                return fail(st);
            if ((st = dev_alloc(&d_counts, (size_t)2)) != MSPMV_OK)
                return fail(st);
            e = hipMemsetAsync(p.d_recs, 0, sizeof(unsigned) * packed.size() * kRecDwords, h->stream);
            if (e == hipSuccess)
                e = hipMemsetAsync(d_counts, 0, sizeof(counts), h->stream);
            if (e == hipSuccess)
                e = launch_fill_recs(p.d_blk, p.blk_stride, p.d_pcols, T, p.d_recs, d_counts, h->stream);
            if (e == hipSuccess)
                e = hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess)
                e = hipStreamSynchronize(h->stream);
            dev_free(d_counts);
            if (e != hipSuccess) {
                set_error(std::string("node blocks: records: ") + hipGetErrorString(e));
                return fail(MSPMV_ERR_HIP);
            }
            p.blk_rec_compact = counts[0];
            p.blk_rec_escaped = counts[1];
        }
    }
    // multi-RHS: only the L = 16 plan (k_spmm_tile's DICT path runs at L = 16 only); not the run-
    // balanced plan (its kernel gathers x directly)
    const bool multi = !single;
    const bool want = fixed ? false : multi ? spmm_dict_max(L) > 0 : true;
    long long dict_entries = 0;  // distinct columns over the tiles that gather through a dictionary
    if (T > 0 && h->nnz > 0 && want) {
        if ((st = dev_alloc(&p.d_dict, (size_t)h->nnz + kNnzPad)) != MSPMV_OK ||
            (st = dev_alloc(&p.d_ndict, (size_t)T)) != MSPMV_OK ||
            (st = dev_alloc(&p.d_idx16, (size_t)h->nnz + kNnzPad)) != MSPMV_OK)
            return fail(st);
        e = hipMemsetAsync(p.d_dict, 0, sizeof(int) * ((size_t)h->nnz + kNnzPad), h->stream);
        if (e == hipSuccess)
            e = hipMemsetAsync(p.d_idx16, 0, sizeof(unsigned short) * ((size_t)h->nnz + kNnzPad), h->stream);
        if (e == hipSuccess)
            e = launch_build_dict(h->d_cols, p.d_bounds, T, maxi, p.d_dict, p.d_ndict, p.d_idx16, h->stream, multi, L);
        std::vector<int> hnd((size_t)T);
        if (e == hipSuccess)
            e = hipMemcpyAsync(hnd.data(), p.d_ndict, sizeof(int) * T, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            set_error(std::string("column dictionaries: ") + hipGetErrorString(e));
            return fail(MSPMV_ERR_HIP);
        }
        for (int v : hnd) {
            p.num_tiles_dict += v > 0;
            dict_entries += v;
        }
        if (p.num_tiles_dict == 0) {  // no tile takes one: drop the arrays, the kernel skips the test
            dev_free(p.d_dict);
            dev_free(p.d_ndict);
            dev_free(p.d_idx16);
            p.d_dict = nullptr;
            p.d_ndict = nullptr;
            p.d_idx16 = nullptr;
        }
    }
    p.stream_bytes = tile_stream_bytes(h, p, dict_entries);
    auto res = h->plans.emplace(fixed ? kRunPlanKey : p.lanes == 64 ? -tile : plan_key(L), p);  // one-wave: negative keys
    *out = &res.first->second;
    return MSPMV_OK;
}

// The plan the plain single-RHS SpMV runs on.  Decided once per handle on first use: a matrix
// whose workgroup plan is mostly merge-walk tiles (row lengths uneven inside most tiles: skewed,
// power-law rows) runs one-wave tiles instead (k_spmv_tile<.., 64>: 512 merge items, wave
// barriers only), so a tile's hub-row closing and its walkers' latencies stall one wave, not four.
// Measured on the skewed pwtk-sized variant 100.1 -> 78.3 us; on row-group plans (banded, FEM,
// stencils) one-wave tiles lost 1-15 % (r03r), so those keep the workgroup plan.
// Column-slab plan (mspmv_slab.hip) for the plain SpMV: MSPMV_SPMV_SLAB=1 takes it for every matrix
// it can hold, =0 never; by default a matrix takes it when its workgroup plan gathers through column
// dictionaries on most tiles (x gathers line-bound: scattered columns) and the slab plan stages at
// most kSlabAutoBytes of x per nonzero (the columns of a block lie in a few slabs: a band, not the
// whole width).  Scattered band at pwtk size: 58.9 -> 40 us per launch (r04w).
constexpr double kSlabAutoBytes = 16.0;
// ... and its blocks hold >= kSlabAutoNnzPerBlock nonzeros: a block's fixed costs (its descriptors,
// yacc, the first slab, the write-out) then spread over >= 6 chunks.  cant (7,800 per block) took the
// slab plan without it and lost: 0.396 against 0.43 on tiles (r04x).
constexpr double kSlabAutoNnzPerBlock = 12288.0;
constexpr bool kSlabAuto = true;
static int slab_switch()  // read at each handle's decision (tests set it per matrix); 2: column groups
{
    const char *e = getenv("MSPMV_SPMV_SLAB");
    return e && *e ? (atoi(e) >= 2 && atoi(e) <= 4 ? atoi(e) : atoi(e) != 0 ? 1 : 0) : -1;
}

// Most of the workgroup plan's tiles are merge walks (row lengths uneven inside most tiles: skewed,
// power-law rows): the one-wave plan's and the sliced-ELL plan's test.
static mspmv_status mostly_walks(const TilePlan *wg, bool *out)
{
    *out = false;
    if (wg->lanes != kBlock || wg->num_tiles < 64 || wg->d_blk)
        return MSPMV_OK;
    std::vector<unsigned char> hm((size_t)wg->num_tiles);
    HIP_TRY(hipMemcpy(hm.data(), wg->d_modes[0], hm.size(), hipMemcpyDeviceToHost));
    long long walk = 0;
    for (unsigned char v : hm)
        walk += v == 0;
    *out = 2 * walk >= (long long)wg->num_tiles;
    return MSPMV_OK;
}

// Skewed rows (mostly merge walks) with at least kSellAutoNnzPerBlock nonzeros per column-group block
// take the sliced-ELL plan (k_spmv_sell) when it stages at most kSlabAutoBytes of x per nonzero: the
// power-law variant at pwtk size 80 -> 55 us per launch (r05ao-r05as); smaller skewed matrices keep
// the one-wave tiles (their blocks would be a few chunks of work each).
constexpr double kSellAutoNnzPerBlock = 12288.0;

static mspmv_status spmv_slab_decide(mspmv_handle_s *h, const TilePlan *wg)
{
    const int sw = slab_switch();
    bool cand = sw >= 1;
    if (sw < 0 && kSlabAuto)
        cand = wg->lanes == kBlock && wg->num_tiles >= 64 && !wg->blk_spmv && 2 * wg->num_tiles_dict >= wg->num_tiles;
    h->spmv_slab = 0;
    // An automatic sliced-ELL attempt with `groups` column groups (0: the default count).  Optional whatever
    // fails, and a plan that stages more than kSlabAutoBytes of x per nonzero counts as one that does not fit.
    auto try_sell = [&](int groups) {
        TilePlan p;
        mspmv_status st = build_slab_plan(h, p, kSellAutoNnzPerBlock, 2, true, groups);
        if (st == MSPMV_OK && p.slab->x_bytes_per_nnz > kSlabAutoBytes)
            st = MSPMV_ERR_UNSUPPORTED;
        return keep_optional(h, kSlabPlanKey, p, st, false, &h->spmv_slab);
    };
    if (!cand && sw < 0 && kSlabAuto) {  // skewed rows: the sliced-ELL plan, when it pays
        bool skew = false;
        ST_TRY(mostly_walks(wg, &skew));
        if (skew && (double)h->nnz >= kSellAutoNnzPerBlock * h->num_cus)
            return try_sell(0);  // any failure keeps the tiles
        return MSPMV_OK;
    }
    if (!cand)
        return MSPMV_OK;
    if (sw < 0 && (double)h->nnz >= kSlabAutoNnzPerBlock * kSlabBlocksPerCu * h->num_cus) {
        // line-bound gathers over a band (rows whose columns scatter within a window of a few slabs): the
        // sliced-ELL kernel with ONE column group -- whole-row blocks, each staging only its band's slabs --
        // before the merge-path slab blocks: bench's scattered band 41.5-42.0 -> 36.3 us (r06r / r06t, with slabs
        // cut from each block's first column; with the power-law variant's 4 groups three of every four blocks of
        // a band would be empty: 118 us, r05).  At the slab blocks' own size bar (cant, 4 M nonzeros, stays on the
        // tiles: 14.2 us on these against 13.9)
        ST_TRY(try_sell(1));  // any failure keeps trying the slab blocks, then the tiles
        if (h->spmv_slab == 1)
            return MSPMV_OK;
    }
    TilePlan p;
    // automatic: the blocks-per-nonzero test runs inside the builder before anything past the bounds is
    // copied or allocated, and any failure (an allocation near capacity included) means "no slab plan":
    // the workgroup plan is ready, so the product must not fail for an optional plan
    const mspmv_status st = build_slab_plan(h, p, sw < 0 ? kSlabAutoNnzPerBlock : 0.0, sw == 2 ? 1 : sw == 4 ? 2 : 0, sw >= 2);
    if (st == MSPMV_OK && sw < 0 && p.slab->x_bytes_per_nnz > kSlabAutoBytes) {
        free_plan(p);
        return MSPMV_OK;
    }
    return keep_optional(h, kSlabPlanKey, p, st, sw >= 1, &h->spmv_slab);
}

// Column-slab plan for the plain SpMM of width L = 8 or 16 (mspmv_slab.hip k_spmm_slab): MSPMV_SPMM_SLAB=1
// takes it for every matrix it can hold, =0 never; by default a matrix whose L-wide product runs the
// merge tiles (not the node-block SpMM) takes it when the plan stages at most kSlabMmAutoFrac of the
// panel bytes the tiles gather (L x 8 B per nonzero): a band or a stencil, whose blocks reuse each staged
// panel row several times, not scattered columns.
constexpr double kSlabMmAutoFrac = 0.5;
constexpr long long kSlabMmAutoMinNnz = 1 << 20;
// Off by default until it beats the L-wide tiles on the BASELINE shapes: cant-shaped L = 16 48 vs 27 us,
// nlpkkt120-size L = 8 715 vs 460 us (r05f).
constexpr bool kSlabMmAuto = false;

static mspmv_status spmm_slab_decide(mspmv_handle_s *h, int L)
{
    int &dec = h->spmm_slab[l_index(L)];
    const int sw = env_tristate("MSPMV_SPMM_SLAB");
    dec = 0;
    if (!(sw == 1 || (sw < 0 && kSlabMmAuto && h->nnz >= kSlabMmAutoMinNnz)))
        return MSPMV_OK;
    TilePlan p;
    const mspmv_status st = build_slab_mm_plan(h, L, p);
    if (st == MSPMV_OK && sw < 0 && p.slab->x_bytes_per_nnz > kSlabMmAutoFrac * 8.0 * L) {
        free_plan(p);
        return MSPMV_OK;
    }
    return keep_optional(h, slab_mm_key(L), p, st, sw == 1, &dec);  // optional: never fail the product
}

// Run-balanced plan for the node-block SpMV / SpMM (round 5).  The merge-path tiles of a node-block plan hold
// ~2,048 items: 6-7 runs on the pwtk shape, one round of k_spmv_blk's eight half-wave run slots.  On
// imperfect FEM (odd-size nodes, off-pattern rows: more, shorter runs) a quarter of the tiles need 9-14
// slots, i.e. a second round after the first has returned (24.2 vs 21.1 us per launch, r04).  This plan
// cuts the tiles at run starts instead, each holding whole runs of <= kBlkTileChunks chunks (the
// runs k_build_blocks forms, restated here on the host: <= kBlkRunRows rows whose column lists are
// prefixes of the run's longest, <= 64 pattern columns per chunk), so every tile is one round.  Only
// the plain SpMV on an all-register node-block plan runs it (k_spmv_blk has no LDS item bound); CG,
// dot-mode callers keep the merge-path plan; the plain L-wide node-block SpMM (k_spmm_blk: the same
// per-round run slots) takes it too.  MSPMV_SPMV_RUNS=0/1 forces it off / on.
static mspmv_status spmv_runs_decide(mspmv_handle_s *h, const TilePlan *wg)
{
    h->spmv_runs = 0;
    const int sw = env_tristate("MSPMV_SPMV_RUNS");
    if (sw == 0 || !wg->blk_spmv || wg->num_tiles_reg != wg->num_tiles || h->m <= 0)
        return MSPMV_OK;
    // optional plan, whatever fails and also when forced: the merge-path plan stays, without the entry
    // build_plan may have inserted
    auto keep_merge_path = [&](mspmv_status st) {
        auto it = h->plans.find(kRunPlanKey);
        if (it != h->plans.end()) {
            free_plan(it->second);
            h->plans.erase(it);
        }
        return optional_failed(st, false);
    };
    const int *ro = nullptr, *ci = nullptr;
    mspmv_status st = host_pattern(h, &ro, &ci);
    if (st != MSPMV_OK)
        return keep_merge_path(st);
    // tiles of whole runs: <= kBlkTileChunks chunks and about the merge-path plan's items, and always
    // at least one run
    // (caps measured, r05l: 112 / 125 / 150 / 200 % of the merge-path tile's items within 1 % on pwtk,
    // 7 chunks per tile slower on the imperfect shape)
    const long long items_cap = (long long)wg->tile_items + wg->tile_items / 4;
    std::vector<int2> hb;
    hb.push_back(make_int2(0, 0));
    int chunks = 0;
    long long items = 0;
    for (int r = 0; r < h->m;) {
        const int g = r;
        int p = g, plen = ro[(size_t)g + 1] - ro[(size_t)g], hgt = 0;
        for (; r < h->m && hgt < kBlkRunRows; ++r, ++hgt) {
            const int s0 = ro[(size_t)r], len = ro[(size_t)r + 1] - s0;
            if (hgt > 0) {
                const int ps = ro[(size_t)p], mm = std::min(len, plen);
                bool same = true;
                for (int q = 0; q < mm && same; ++q)
                    same = ci[(size_t)s0 + q] == ci[(size_t)ps + q];
                if (!same || (len > 64 && plen <= 64))  // (k_build_blocks' rules, incl. its 64-column stop)
                    break;
                if (len > plen) {
                    p = r;
                    plen = len;
                }
            }
        }
        const int c = std::max(1, (plen + 63) / 64);
        const long long it = (long long)(r - g) + (ro[(size_t)r] - ro[(size_t)g]);
        if (chunks > 0 && (chunks + c > kBlkTileChunks || items + it > items_cap)) {
            hb.push_back(make_int2(g, ro[(size_t)g]));
            chunks = 0;
            items = 0;
        }
        chunks += c;
        items += it;
    }
    hb.push_back(make_int2(h->m, h->nnz));
    if (hb.size() > 2 && hb[hb.size() - 2].x == h->m)
        hb.erase(hb.end() - 2);
    const TilePlan *np = nullptr;
    if ((st = build_plan(h, 1, &np, 0, &hb)) != MSPMV_OK)
        return keep_merge_path(st);
    TilePlan &rp = h->plans.find(kRunPlanKey)->second;
    st = ensure_modes(h, rp, 1);
    if (st != MSPMV_OK || !rp.blk_spmv || rp.num_tiles_reg != rp.num_tiles)  // the runs must all be register tiles
        return keep_merge_path(st);
    h->spmv_runs = 1;
    return MSPMV_OK;
}

// ... after the windows (product_plan): slab / sliced-ELL, one-wave tiles, the run-balanced node-block plan, the
// workgroup plan.
static mspmv_status spmv_plan(mspmv_handle_s *h, const TilePlan **out)
{
    const TilePlan *wg = nullptr;
    ST_TRY(solver_plan(h, 1, &wg));
    if (h->spmv_slab < 0)
        ST_TRY(spmv_slab_decide(h, wg));
    if (h->spmv_slab == 1) {
        *out = &h->plans.find(kSlabPlanKey)->second;
        return MSPMV_OK;
    }
    if (h->spmv_onewave < 0) {
        bool want = false;
        ST_TRY(mostly_walks(wg, &want));
        if (want) {
            const TilePlan *np = nullptr;
            const int key = -64 * spmv_items_per_thread();  // build_plan's key for one-wave plans
            if (h->plans.find(key) == h->plans.end())
                ST_TRY(build_plan(h, 1, &np, 64));
            ST_TRY(ensure_modes(h, h->plans.find(key)->second, 1));
        }
        h->spmv_onewave = want ? 1 : 0;
    }
    if (h->spmv_onewave == 1) {
        *out = &h->plans.find(-64 * spmv_items_per_thread())->second;
        return MSPMV_OK;
    }
    if (h->spmv_runs < 0)
        ST_TRY(spmv_runs_decide(h, wg));
    *out = h->spmv_runs == 1 ? &h->plans.find(kRunPlanKey)->second : wg;
    return MSPMV_OK;
}

// The single-RHS plan when it is built and holds node blocks only (every tile a register run tile: FEM node
// rows) and k_spmm_blk is enabled, else null: L > 1 columns multiply on that plan with k_spmm_blk -- one
// panel-row gather per (run, column) -- instead of their own L-wide merge tiles.
static TilePlan *all_node_blocks(mspmv_handle_s *h)
{
    if (!spmm_blk_enabled())
        return nullptr;
    auto one = h->plans.find(plan_key(1));
    const bool all = one != h->plans.end() && one->second.d_blk && one->second.num_tiles_reg == one->second.num_tiles;
    return all ? &one->second : nullptr;
}

mspmv_status mspmv::solver_plan(mspmv_handle_s *h, int L, const TilePlan **out)
{
    TilePlan *tp = L > 1 ? all_node_blocks(h) : nullptr;
    if (!tp) {
        const int key = plan_key(L);
        if (h->plans.find(key) == h->plans.end()) {
            const TilePlan *np = nullptr;
            ST_TRY(build_plan(h, L, &np));
        }
        tp = &h->plans.find(key)->second;
    }
    ST_TRY(ensure_modes(h, *tp, L));
    *out = tp;
    return cache_book(h);
}

long long mspmv::tile_stream_bytes(const mspmv_handle_s *h, const TilePlan &p, long long dict_entries)
{
    const long long nnz = h->nnz, T = p.num_tiles;
    if (p.blk_spmv && p.d_recs)  // values, one 64-B record per descriptor slot, bounds (8 B) and column base per tile
        return 8 * nnz + 4LL * kRecDwords * T * p.blk_stride + 12 * T;
    const long long cols = p.d_cols16 && p.num_tiles16 == p.num_tiles ? 2 : 4;
    // a dictionary tile reads its distinct columns and a 16-bit index per nonzero besides
    const long long dict = p.d_dict ? 4 * dict_entries + 2 * nnz * p.num_tiles_dict / std::max(T, 1LL) : 0;
    return (8 + cols) * nnz + 4 * ((long long)h->m + 1) + dict;
}

constexpr double kShardedNtBytes = 128.0 * 1024 * 1024;  // (cache_book: handles outside the ledger)

mspmv_status mspmv::cache_book(mspmv_handle_s *h, bool force)
{
    if (!force && h->plans.size() == h->cache_plans)
        return MSPMV_OK;
    h->cache_plans = h->plans.size();
    long long want = 0;
    for (const auto &kv : h->plans)
        want = std::max(want, kv.second.stream_bytes);
    if (!force && want == h->cache_bytes)
        return MSPMV_OK;
    long long granted = 0;
    int resident = 1;
    if (!h->cache_ledger && h->cache_policy == MSPMV_CACHE_AUTO) {
        // a sharded object's handle: any lease an override took goes back, and the matrix streams nontemporal when
        // its CSR (12 B per nonzero + row offsets) is larger than half the 256 MiB cache, as before the ledger
        ST_TRY(mspmv_cache_lease(h->device, h->cache_lease, 0, MSPMV_CACHE_STREAM, &granted, &resident));
        resident = 12.0 * (double)h->nnz + 4.0 * (double)h->m > kShardedNtBytes ? 0 : 1;
    } else {
        ST_TRY(mspmv_cache_lease(h->device, h->cache_lease, want, h->cache_policy, &granted, &resident));
    }
    h->cache_bytes = want;
    h->cache_lease = granted;
    if ((resident != 0) != h->cache_resident) {
        if (h->stream)
            HIP_TRY(hipStreamSynchronize(h->stream));
        h->cg_graph.reset();
        h->bicg_graph.reset();
        h->pbicg_graph.reset();
        h->bcg_graph.reset();
        h->cache_resident = resident != 0;
    }
    return MSPMV_OK;
}

void mspmv::cache_release(mspmv_handle_s *h)
{
    long long granted = 0;
    int resident = 0;
    if (h->cache_lease > 0)
        (void)mspmv_cache_lease(h->device, h->cache_lease, 0, MSPMV_CACHE_STREAM, &granted, &resident);
    h->cache_lease = 0;
}

mspmv_status mspmv::product_plan(mspmv_handle_s *h, int L, const TilePlan **out)
{
    ST_TRY(product_plan_unbooked(h, L, out));
    return cache_book(h);
}

static mspmv_status product_plan_unbooked(mspmv_handle_s *h, int L, const TilePlan **out)
{
    PatternScope scope(h);  // the decisions share one host copy of the pattern
    ST_TRY(window_plan(h, L, out));
    if (*out)
        return MSPMV_OK;
    if (L == 1)
        return spmv_plan(h, out);
    if (TilePlan *one = all_node_blocks(h)) {  // on the run-balanced plan, as the plain SpMV (spmv_runs_decide)
        if (h->spmv_runs < 0)
            ST_TRY(spmv_runs_decide(h, one));
        auto rp = h->spmv_runs == 1 ? h->plans.find(kRunPlanKey) : h->plans.end();
        TilePlan *tp = rp != h->plans.end() ? &rp->second : one;
        ST_TRY(ensure_modes(h, *tp, L));
        *out = tp;
        return MSPMV_OK;
    }
    const TilePlan *tp = nullptr;
    ST_TRY(solver_plan(h, L, &tp));
    if (L == 8 || L == 16) {
        // on a column-slab plan when one was chosen (spmm_slab_decide, after the node-block check: FEM matrices
        // keep k_spmm_blk)
        if (h->spmm_slab[l_index(L)] < 0)
            ST_TRY(spmm_slab_decide(h, L));
        auto it = h->spmm_slab[l_index(L)] == 1 ? h->plans.find(slab_mm_key(L)) : h->plans.end();
        if (it != h->plans.end())
            tp = &it->second;
    }
    *out = tp;
    return MSPMV_OK;
}

void mspmv::drop_plans(mspmv_handle_s *h)
{
    for (auto &kv : h->plans)
        free_plan(kv.second);
    h->plans.clear();
    h->dia = h->spmv_slab = h->spmv_onewave = h->spmv_runs = -1;
    for (int &v : h->spmm_slab)
        v = -1;
}

// mspmv_api.hip -- the C-ABI (include/mspmv.h): matrix handles, the SpMV / SpMM entry points, measurement,
// batch entries, plan introspection and memory helpers.  (Building and choosing plans: mspmv_plan.hip; the solver
// entries and their drivers: mspmv_solve.hip; the IC(0) / ILU(0) factor objects: mspmv_tri.hip.)  Host C++17
// over the HIP runtime.
#include "mspmv_internal.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

namespace mspmv {

static thread_local std::string g_err;

void set_error(const std::string &msg) { g_err = msg; }

hipError_t launch_flush(void *p, size_t bytes, hipStream_t s, bool fresh);

}  // namespace mspmv

unsigned long long mspmv_next_generation()
{
    static std::atomic<unsigned long long> next{1};
    return next.fetch_add(1, std::memory_order_relaxed);
}

using namespace mspmv;

__global__ void k_check_cols(const int *__restrict__ cols, long long nnz, int n, int *bad)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += (long long)gridDim.x * blockDim.x) {
        const int c = cols[i];
        if (c < 0 || c >= n)
            atomicOr(bad, 1);
    }
}


static mspmv_status check_offsets_host(const int *ro, int m, int nnz)
{
    if (ro[0] != 0)
        return invalid("row_offsets[0] != 0");
    for (int i = 0; i < m; ++i)
        if (ro[i + 1] < ro[i])
            return invalid("row_offsets not monotone at row " + std::to_string(i));
    if (ro[m] != nnz)
        return invalid("row_offsets[num_rows] != num_nonzeros");
    return MSPMV_OK;
}

// ---- the stream pool: one stream per slot of the device's ledger (mspmv_streams.cpp) ----------
// The four are created back to back on the first lease and never destroyed, not at unload either: created
// together they sit on the process's four hardware queues, one each, and a handle that leases slot i always
// runs on queue i.  Streams created one per handle, between uploads and plan builds, landed two on one queue
// (DESIGN 4.2e).
static std::mutex g_pool_mu;
static std::map<int, std::array<hipStream_t, kStreamPool>> g_pool_streams;

// MSPMV_STREAM_POOL, read per create: 0 = every handle creates a stream of its own, as before the pool.
static bool stream_pool_env()
{
    const char *v = getenv("MSPMV_STREAM_POOL");
    return !(v && v[0] == '0');
}

// The lowest free slot of `device` (the current device) and its stream; *slot stays -1, and *s untouched, with
// the pool switched off or every slot taken.
static mspmv_status pool_lease(int device, int *slot, hipStream_t *s)
{
    *slot = -1;
    if (!stream_pool_env())
        return MSPMV_OK;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto it = g_pool_streams.find(device);
    if (it == g_pool_streams.end()) {
        std::array<hipStream_t, kStreamPool> a{};
        for (int i = 0; i < kStreamPool; ++i)
            if (hipStreamCreateWithFlags(&a[(size_t)i], hipStreamNonBlocking) != hipSuccess) {
                while (i-- > 0)
                    (void)hipStreamDestroy(a[(size_t)i]);
                set_error("hipStreamCreate failed (stream pool)");
                return MSPMV_ERR_HIP;
            }
        it = g_pool_streams.emplace(device, a).first;
    }
    ST_TRY(mspmv_stream_slot_take(device, slot));
    if (*slot >= 0)
        *s = it->second[(size_t)*slot];
    return MSPMV_OK;
}

// The handle's stream goes: a private one is destroyed, a pool slot given back (a caller's or a CU-masked one
// stays).  After the stream has been synchronised.
static void release_stream(mspmv_handle_s *h)
{
    if (h->stream && h->own_stream)
        (void)hipStreamDestroy(h->stream);
    if (h->stream_slot >= 0)
        (void)mspmv_stream_slot_give(h->device, h->stream_slot);
    h->stream = nullptr;
    h->stream_slot = -1;
}

// view_of: a row range of another handle on the same device -- a->row_offsets (host, rebased to 0)
// are uploaded, the columns and values are the parent's from nonzero view_off on (not copied, not
// owned; the parent validated them), a->column_indices / values are ignored.
static mspmv_status create_common(const mspmv_csr_d *a, int device, bool from_device, mspmv_handle *out,
                                  hipStream_t on_stream = nullptr, mspmv_handle_s *view_of = nullptr,
                                  long long view_off = 0)
{
    if (view_of) {
        if (!a || a->num_rows < 0 || a->num_nonzeros < 0 || !a->row_offsets || view_off < 0 ||
            view_off + a->num_nonzeros > view_of->nnz || a->num_cols != view_of->n)
            return invalid("row-range view outside its parent");
    } else {
        ST_TRY(validate_host_csr(a));
    }
    if (!out)
        return invalid("null out handle");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible");
        return MSPMV_ERR_HIP;
    }
    if (device < 0 || device >= ndev)
        return invalid("device index out of range");
    HIP_TRY(hipSetDevice(device));
    const auto t0 = std::chrono::steady_clock::now();
    auto *h = new mspmv_handle_s();
    h->device = device;
    h->m = a->num_rows;
    h->n = a->num_cols;
    h->nnz = a->num_nonzeros;
    h->cache_ledger = !on_stream && !view_of;  // a sharded object's handles keep out of the ledger (cache_book)
    auto fail = [&](mspmv_status s) {
        mspmv_destroy(h);
        return s;
    };
    if (hipDeviceGetAttribute(&h->num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
        h->num_cus < 1)
        h->num_cus = 256;
    mspmv_status st;
    if (on_stream) {  // a stream owned by the caller (mspmv_comm: one stream per rank)
        h->stream = on_stream;
        h->own_stream = false;
    } else {
        // a slot of the device's pool, while there is one (a row-range view keeps a stream of its own making);
        // before anything below submits work, so the pool's first use finds every hardware queue still free
        if (!view_of && (st = pool_lease(device, &h->stream_slot, &h->stream)) != MSPMV_OK)
            return fail(st);
        if (h->stream_slot >= 0) {
            h->own_stream = false;
        } else if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
            set_error("hipStreamCreate failed");
            return fail(MSPMV_ERR_HIP);
        }
    }
    // Column / value arrays are padded (zero column index, zero value) so the kernels' aligned
    // 16-byte group reads past the last nonzero stay inside the allocation.
    const size_t padded = (size_t)h->nnz + kNnzPad;
    if ((st = dev_alloc(&h->d_row_offsets, (size_t)h->m + 1)) != MSPMV_OK)
        return fail(st);
    if (view_of) {  // the parent's arrays (padded past its last nonzero, so past this range's too)
        h->own_arrays = false;
        h->d_cols = view_of->d_cols + view_off;
        h->d_vals = view_of->d_vals + view_off;
    } else {
        if ((st = dev_alloc(&h->d_cols, padded)) != MSPMV_OK || (st = dev_alloc(&h->d_vals, padded)) != MSPMV_OK)
            return fail(st);
        if (memset_sync(h->d_cols, 0, sizeof(int) * padded) != hipSuccess ||
            memset_sync(h->d_vals, 0, sizeof(double) * padded) != hipSuccess) {
            set_error("hipMemset of padded CSR arrays failed");
            return fail(MSPMV_ERR_HIP);
        }
    }
    if ((st = dev_alloc(&h->d_fault, 1)) != MSPMV_OK)
        return fail(st);
    if (memset_sync(h->d_fault, 0, sizeof(unsigned)) != hipSuccess) {
        set_error("hipMemset of the fault word failed");
        return fail(MSPMV_ERR_HIP);
    }
    const hipMemcpyKind kind = from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    std::vector<int> host_ro;
    const int *ro = a->row_offsets;
    if (from_device) {
        host_ro.resize((size_t)h->m + 1);
        if (hipMemcpy(host_ro.data(), a->row_offsets, sizeof(int) * (h->m + 1), hipMemcpyDeviceToHost) != hipSuccess) {
            set_error("copy of device row_offsets failed");
            return fail(MSPMV_ERR_HIP);
        }
        ro = host_ro.data();
    }
    if ((st = check_offsets_host(ro, h->m, h->nnz)) != MSPMV_OK)
        return fail(st);
    if (hipMemcpy(h->d_row_offsets, a->row_offsets, sizeof(int) * (h->m + 1), kind) != hipSuccess ||
        (!view_of && h->nnz &&
         hipMemcpy(h->d_cols, a->column_indices, sizeof(int) * (size_t)h->nnz, kind) != hipSuccess) ||
        (!view_of && h->nnz && hipMemcpy(h->d_vals, a->values, sizeof(double) * (size_t)h->nnz, kind) != hipSuccess)) {
        set_error("CSR upload failed");
        return fail(MSPMV_ERR_HIP);
    }
    if (h->nnz && !view_of) {  // column range check on the device (a bad index would fault a gather)
        int *d_bad = nullptr;
        if ((st = dev_alloc(&d_bad, 1)) != MSPMV_OK)
            return fail(st);
        int bad = 0;
        hipError_t e = memset_sync(d_bad, 0, sizeof(int));
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_check_cols, dim3(1024), dim3(256), 0, h->stream, h->d_cols, (long long)h->nnz, h->n,
                               d_bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess)
            e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess)
            e = hipMemcpy(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost);
        dev_free(d_bad);
        if (e != hipSuccess) {
            set_error(std::string("column check: ") + hipGetErrorString(e));
            return fail(MSPMV_ERR_HIP);
        }
        if (bad)
            return fail(invalid("column index out of [0, num_cols)"));
    }
    // The plain product's plan is decided here, from the caller's host arrays when there are any (no
    // download): a matrix that takes the offset windows never builds the merge tile plan (VERDICT r05:
    // 0.66 ms of unused k_build_dict / k_pack_cols16 / k_build_blocks on the nlpkkt120 size); any other
    // path that needs tiles builds them on first use.
    {
        PatternScope scope(h);
        if (!from_device && !view_of) {
            h->pat_ro_ext = a->row_offsets;
            h->pat_ci_ext = a->column_indices;
        }
        const TilePlan *plan = nullptr;
        st = product_plan(h, 1, &plan);
        h->pat_ro_ext = h->pat_ci_ext = nullptr;
        if (st != MSPMV_OK)
            return fail(st);
    }
    if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) {
        set_error("hipEventCreate failed");
        return fail(MSPMV_ERR_HIP);
    }
    if (hipStreamSynchronize(h->stream) != hipSuccess) {
        set_error("setup sync failed");
        return fail(MSPMV_ERR_HIP);
    }
    h->setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (view_of)
        ++view_of->num_views;
    *out = h;
    return MSPMV_OK;
}

// mspmv_csr_update_values{,_dev}: d_vals again from `values`, then every derived copy of the values the handle
// holds -- the window panels and remainder (DiaData), the slab value streams (SlabData), the resident CG's ELL.
// The merge tiles, node blocks (descriptors, records, run-balanced plan), one-wave tiles, 16-bit column streams
// and dictionaries read d_vals in CSR order and hold no value copy.  All on h's stream, nothing waited for.
static mspmv_status update_values_common(mspmv_handle_s *h, const double *values, bool from_device)
{
    ST_TRY(check_handle(h));
    if (h->nnz > 0 && !values)
        return invalid("update_values: null values");
    if (!h->own_arrays) {
        set_error("update_values: the handle is a row-range view; its values belong to the handle it was cut from");
        return MSPMV_ERR_UNSUPPORTED;
    }
    if (h->num_views > 0) {
        set_error("update_values: row-range views were cut from this handle and read its values");
        return MSPMV_ERR_UNSUPPORTED;
    }
    if (h->nnz == 0)
        return MSPMV_OK;
    for (auto &kv : h->plans) {  // what can fail for want of memory comes first: a failed update enqueues nothing
        ST_TRY(prepare_dia_update(kv.second));
        ST_TRY(prepare_slab_update(kv.second));
    }
    HIP_TRY(hipMemcpyAsync(h->d_vals, values, sizeof(double) * (size_t)h->nnz,
                           from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    for (auto &kv : h->plans) {
        ST_TRY(refresh_dia_values(h, kv.second));
        ST_TRY(refresh_slab_values(h, kv.second));
    }
    HIP_TRY(resident_refresh_values(h));
    return MSPMV_OK;
}

extern "C" {

const char *mspmv_last_error(void) { return g_err.c_str(); }

const char *mspmv_cg_kernel_name(mspmv_handle h) { return h ? h->last_cg_kernel.c_str() : ""; }

const char *mspmv_solver_product_kernel_name(mspmv_handle h) { return h ? h->last_solver_product.c_str() : ""; }

const char *mspmv_spmv_kernel_name(mspmv_handle h)
{
    thread_local std::string name;
    if (!h)
        return "";
    const TilePlan no_tiles;  // a handle without rows builds no plan: it reports what an empty one would run
    const TilePlan *plan = nullptr;
    if (h->m > 0 && product_plan(h, 1, &plan) != MSPMV_OK)
        return "";
    name = product_kernel_name(h, plan ? *plan : no_tiles, 1);
    return name.c_str();
}

const char *mspmv_spmm_kernel_name(mspmv_handle h, int L)
{
    thread_local std::string name;
    if (!h || L < 1)
        return "";
    // widths outside 1, 2, 4, 8, 16 run as column chunks (odd L on a zero-padded panel): the
    // widest chunk's kernel
    int w = 16;
    const int lp = (L > 1 && (L & 1)) ? L + 1 : L;
    while (w > lp)
        w >>= 1;
    const TilePlan *plan = nullptr;
    if (product_plan(h, w, &plan) != MSPMV_OK)
        return "";
    name = product_kernel_name(h, *plan, w);
    return name.c_str();
}

const char *mspmv_version(void) { return "mspmv 0.1.0 (gfx950, merge-path fp64)"; }

int mspmv_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

mspmv_status mspmv_csr_create(const mspmv_csr_d *host, int device, mspmv_handle *out)
{
    return create_common(host, device, false, out);
}

mspmv_status mspmv_csr_create_dev(const mspmv_csr_d *dev, int device, mspmv_handle *out)
{
    return create_common(dev, device, true, out);
}

}  // extern "C"

mspmv_status mspmv::csr_create_on_stream(const mspmv_csr_d *host, int device, hipStream_t stream, mspmv_handle *out)
{
    return create_common(host, device, false, out, stream);
}

mspmv_status mspmv::csr_create_view(mspmv_handle parent, int row_lo, int row_hi, const int *host_row_offsets,
                                    mspmv_handle *out)
{
    if (!parent || row_lo < 0 || row_hi < row_lo || row_hi > parent->m || !host_row_offsets)
        return invalid("csr_create_view: bad row range");
    const long long off = host_row_offsets[row_lo];
    std::vector<int> ro((size_t)(row_hi - row_lo) + 1);
    for (int r = row_lo; r <= row_hi; ++r)
        ro[(size_t)(r - row_lo)] = (int)(host_row_offsets[r] - off);
    const mspmv_csr_d v{row_hi - row_lo, parent->n, ro.back(), ro.data(), nullptr, nullptr};
    return create_common(&v, parent->device, false, out, nullptr, parent, off);
}

extern "C" {

mspmv_status mspmv_destroy(mspmv_handle h)
{
    if (!h)
        return MSPMV_OK;
    (void)hipSetDevice(h->device);
    if (h->stream)
        (void)hipStreamSynchronize(h->stream);
    drop_plans(h);
    cache_release(h);
    dev_free(h->d_row_offsets);
    if (h->own_arrays) {
        dev_free(h->d_cols);
        dev_free(h->d_vals);
    }
    dev_free(h->d_r);
    dev_free(h->d_p0);
    dev_free(h->d_p1);
    dev_free(h->d_ap);
    dev_free(h->d_rhat);
    dev_free(h->d_partials);
    dev_free(h->d_partials_b);
    dev_free(h->d_gtickets);
    dev_free(h->d_scal);
    dev_free(h->d_bcg);
    dev_free(h->d_red);
    dev_free(h->d_warm);
    dev_free(h->d_resw);
    dev_free(h->d_conv);
    dev_free(h->d_ctrl);
    dev_free(h->d_hist);
    dev_free(h->d_fault);
    h->cg_graph.reset();
    h->bicg_graph.reset();
    h->pbicg_graph.reset();
    h->bcg_graph.reset();
    if (h->d_flush)
        (void)hipFree(h->d_flush);
    if (h->h_ctrl)
        (void)hipHostFree(h->h_ctrl);
    if (h->ev0)
        (void)hipEventDestroy(h->ev0);
    if (h->ev1)
        (void)hipEventDestroy(h->ev1);
    resident_free(h->rcg);
    release_stream(h);
    delete h;
    return MSPMV_OK;
}

mspmv_status mspmv_shape(mspmv_handle h, int *num_rows, int *num_cols, int *num_nonzeros)
{
    if (!h)
        return invalid("null handle");
    if (num_rows)
        *num_rows = h->m;
    if (num_cols)
        *num_cols = h->n;
    if (num_nonzeros)
        *num_nonzeros = h->nnz;
    return MSPMV_OK;
}

double mspmv_setup_ms(mspmv_handle h) { return h ? h->setup_ms : 0.0; }

mspmv_status mspmv_csr_update_values(mspmv_handle h, const double *values)
{
    const auto t0 = std::chrono::steady_clock::now();
    ST_TRY(update_values_common(h, values, false));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->update_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return MSPMV_OK;
}

mspmv_status mspmv_csr_update_values_dev(mspmv_handle h, const double *d_values)
{
    return update_values_common(h, d_values, true);
}

double mspmv_update_ms(mspmv_handle h) { return h ? h->update_ms : 0.0; }

mspmv_status mspmv_sync(mspmv_handle h)
{
    ST_TRY(check_handle(h));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MSPMV_OK;
}

// One CU-masked stream per (device, CU count) for the whole process, shared by every handle
// limited to that count and never destroyed: a masked stream holds a hardware queue of its own,
// and creating one per handle / per call ran a process out of its few queues (a launch on a
// third masked stream never started).
static std::mutex g_cu_mu;
static std::map<std::pair<int, int>, hipStream_t> g_cu_streams;

mspmv_status mspmv_set_cu_limit(mspmv_handle h, int num_cus)
{
    ST_TRY(check_handle(h));
    HIP_TRY(hipSetDevice(h->device));
    int total = 0;
    HIP_TRY(hipDeviceGetAttribute(&total, hipDeviceAttributeMultiprocessorCount, h->device));
    const int n = (num_cus <= 0 || num_cus >= total) ? total : num_cus;
    hipStream_t s = nullptr;
    bool own = true;
    int slot = -1;
    if (n == total) {
        if (h->stream_slot >= 0)  // a pool stream runs on every CU already
            return MSPMV_OK;
        ST_TRY(pool_lease(h->device, &slot, &s));  // a free slot before a stream of its own
        if (slot >= 0)
            own = false;
        else
            HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    } else {
        std::lock_guard<std::mutex> lk(g_cu_mu);
        auto it = g_cu_streams.find({h->device, n});
        if (it != g_cu_streams.end()) {
            s = it->second;
        } else {
            // CU i joins when floor((i+1) n / total) steps: n of the total, evenly spaced
            std::vector<uint32_t> mask((size_t)(total + 31) / 32, 0u);
            for (int i = 0; i < total; ++i)
                if ((long long)(i + 1) * n / total > (long long)i * n / total)
                    mask[(size_t)i / 32] |= 1u << (i % 32);
            HIP_TRY(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()));
            g_cu_streams[{h->device, n}] = s;
        }
        own = false;
    }
    if (s == h->stream)
        return MSPMV_OK;
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        if (own)
            (void)hipStreamDestroy(s);
        if (slot >= 0)
            (void)mspmv_stream_slot_give(h->device, slot);
        set_error(std::string("set_cu_limit: ") + hipGetErrorString(e));
        return MSPMV_ERR_HIP;
    }
    // the solvers' graphs were captured on the old stream with the old launch sizing
    h->cg_graph.reset();
    h->bicg_graph.reset();
    h->pbicg_graph.reset();
    h->bcg_graph.reset();
    release_stream(h);
    h->stream = s;
    h->own_stream = own;
    h->stream_slot = slot;
    if (n != h->num_cus) {
        // the register-resident CG layout is one workgroup per CU of the whole device: a CU-limited
        // stream cannot hold it (and one built while limited is "does not fit") -- rebuilt on demand
        resident_free(h->rcg);
        h->rcg = nullptr;
        // the single-RHS plan's tile stretch is sized to num_cus x resident workgroups (build_plan):
        // drop every cached plan so the next call plans for the CUs it will actually run on
        drop_plans(h);
        h->num_cus = n;
        const TilePlan *plan = nullptr;
        ST_TRY(solver_plan(h, 1, &plan));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return MSPMV_OK;
}

mspmv_status mspmv_stream_slot(mspmv_handle h, int *slot)
{
    ST_TRY(check_handle(h));
    if (!slot)
        return invalid("stream_slot: null out pointer");
    *slot = h->stream_slot;
    return MSPMV_OK;
}

mspmv_status mspmv_set_cache_policy(mspmv_handle h, int policy)
{
    ST_TRY(check_handle(h));
    if (policy != MSPMV_CACHE_AUTO && policy != MSPMV_CACHE_STREAM && policy != MSPMV_CACHE_RESIDENT)
        return invalid("set_cache_policy: unknown policy");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->cache_policy = policy;
    // a captured graph holds one instantiation of every product kernel
    h->cg_graph.reset();
    h->bicg_graph.reset();
    h->pbicg_graph.reset();
    h->bcg_graph.reset();
    return cache_book(h, true);
}

mspmv_status mspmv_cache_info(mspmv_handle h, int *resident, long long *bytes)
{
    ST_TRY(check_handle(h));
    if (resident)
        *resident = h->cache_resident ? 1 : 0;
    if (bytes) {
        const TilePlan *plan = nullptr;
        if (h->m > 0)
            ST_TRY(product_plan(h, 1, &plan));
        *bytes = plan ? plan->stream_bytes : 0;
    }
    return MSPMV_OK;
}

mspmv_status mspmv_merge_coords(mspmv_handle h, int num_parts, mspmv_coord *coords)
{
    ST_TRY(check_handle(h));
    if (num_parts < 1 || !coords)
        return invalid("num_parts must be >= 1 and coords non-null");
    const long long total = (long long)h->m + h->nnz;
    const long long step = (total + num_parts - 1) / num_parts;  // cpu_spmv.cpp:379
    int2 *d = nullptr;
    ST_TRY(dev_alloc(&d, (size_t)num_parts + 1));
    hipError_t e = launch_merge_coords(h->d_row_offsets, h->m, h->nnz, step, num_parts, d, h->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(coords, d, sizeof(int2) * (num_parts + 1), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(h->stream);
    dev_free(d);
    if (e != hipSuccess) {
        set_error(std::string("merge coords: ") + hipGetErrorString(e));
        return MSPMV_ERR_HIP;
    }
    return MSPMV_OK;
}

// Even L outside the native set (6, 32, 1024, ... -- the reference's OmpMergeCsrmm takes any
// num_vectors, eval_vectors.sh sweeps 1..1024): column chunks of 16, 8, 4, 2 at even offsets of
// the same panels, the kernels reading and writing with panel stride L.  Each column's sum is
// the chunk kernel's, so the result equals the native-width one up to the tile plan's split
// rows (the SpMM tolerance of the tests).
static mspmv_status spmm_chunks(mspmv_handle_s *h, const double *d_X, double *d_Y, int L)
{
    const TilePlan *dp = nullptr;  // the offset-window plan serves every width it is enabled for
    ST_TRY(window_plan(h, 2, &dp));
    for (int c0 = 0; c0 < L;) {
        const int w = native_chunk(L - c0);
        const TilePlan *plan = dp;
        if (!plan)
            ST_TRY(solver_plan(h, w, &plan));
        HIP_TRY(launch_spmm(h, *plan, d_X + c0, d_Y + c0, w, nullptr, L));
        c0 += w;
    }
    return MSPMV_OK;
}

mspmv_status mspmv_dspmm_dev(mspmv_handle h, const double *d_X, double *d_Y, int L)
{
    ST_TRY(check_handle(h));
    if (L < 1)
        return invalid("L must be >= 1");
    if (h->m > 0 && (!d_X || !d_Y))
        return invalid("null vector");
    if (L > 1 && L % 2 == 0 && (!aligned16(d_X) || !aligned16(d_Y)))
        return invalid("multi-vector panels must be 16-byte aligned");
    if (h->m == 0)
        return MSPMV_OK;
    if (supported_L(L)) {
        const TilePlan *plan = nullptr;
        ST_TRY(product_plan(h, L, &plan));
        int nk = 0;
        HIP_TRY(launch_spmm(h, *plan, d_X, d_Y, L, &nk));
        return MSPMV_OK;
    }
    if (L % 2 == 0)
        return spmm_chunks(h, d_X, d_Y, L);
    // odd L > 1: through panels padded with a zero column to L + 1 (16-byte aligned rows)
    const int Lp = L + 1;
    double *xp = nullptr, *yp = nullptr;
    ST_TRY(dev_alloc(&xp, (size_t)h->n * Lp));
    mspmv_status st = dev_alloc(&yp, (size_t)h->m * Lp);
    hipError_t e = hipSuccess;
    if (st == MSPMV_OK)
        e = launch_panel_copy(d_X, L, xp, Lp, h->n, L, Lp, h->stream);
    if (st == MSPMV_OK && e == hipSuccess)
        st = spmm_chunks(h, xp, yp, Lp);
    if (st == MSPMV_OK && e == hipSuccess)
        e = launch_panel_copy(yp, Lp, d_Y, L, h->m, L, L, h->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(h->stream);  // before the padded panels are released
    dev_free(xp);
    dev_free(yp);
    if (st == MSPMV_OK && e != hipSuccess) {
        set_error(std::string("padded SpMM: ") + hipGetErrorString(e));
        st = MSPMV_ERR_HIP;
    }
    return st;
}

mspmv_status mspmv_dspmv_dev(mspmv_handle h, const double *d_x, double *d_y)
{
    return mspmv_dspmm_dev(h, d_x, d_y, 1);
}

mspmv_status mspmv_dspmm(mspmv_handle h, const double *X, double *Y, int L)
{
    ST_TRY(check_handle(h));
    if (L < 1)
        return invalid("L must be >= 1");
    if (h->m == 0)
        return MSPMV_OK;
    if (!X || !Y)
        return invalid("null vector");
    double *dX = nullptr, *dY = nullptr;
    ST_TRY(dev_alloc(&dX, (size_t)h->n * L));
    mspmv_status st = dev_alloc(&dY, (size_t)h->m * L);
    if (st == MSPMV_OK) {
        hipError_t e = hipMemcpyAsync(dX, X, sizeof(double) * h->n * L, hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) {
            set_error(hipGetErrorString(e));
            st = MSPMV_ERR_HIP;
        }
    }
    if (st == MSPMV_OK)
        st = mspmv_dspmm_dev(h, dX, dY, L);
    if (st == MSPMV_OK) {
        hipError_t e = hipMemcpyAsync(Y, dY, sizeof(double) * h->m * L, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            set_error(hipGetErrorString(e));
            st = MSPMV_ERR_HIP;
        }
    }
    if (st == MSPMV_OK)
        st = mspmv_check_faults(h);
    dev_free(dX);
    dev_free(dY);
    return st;
}

mspmv_status mspmv_dspmv(mspmv_handle h, const double *x, double *y) { return mspmv_dspmm(h, x, y, 1); }

mspmv_status mspmv_spmv_tile_stamps(mspmv_handle h, const double *d_x, double *d_y, size_t flush_bytes,
                                    unsigned long long *stamps, int *num_tiles)
{
    ST_TRY(check_handle(h));
    const TilePlan *p = nullptr;
    ST_TRY(product_plan(h, 1, &p));
    if (num_tiles)
        *num_tiles = p->num_tiles;
    if (!stamps)
        return MSPMV_OK;
    if (h->m > 0 && (!d_x || !d_y))
        return invalid("null vector");
    unsigned long long *d_st = nullptr;
    ST_TRY(dev_alloc(&d_st, (size_t)std::max(p->num_tiles, 1) * 6));
    hipError_t e = hipMemsetAsync(d_st, 0, sizeof(unsigned long long) * (size_t)std::max(p->num_tiles, 1) * 6, h->stream);
    if (e == hipSuccess && flush_bytes && flush_bytes > h->flush_cap) {  // the cold protocol's read sweep first
        if (h->d_flush)
            (void)hipFree(h->d_flush);
        h->d_flush = nullptr;
        h->flush_cap = 0;
        e = hipMalloc(&h->d_flush, flush_bytes);
        if (e == hipSuccess) {
            h->flush_cap = flush_bytes;
            e = launch_flush(h->d_flush, flush_bytes, h->stream, true);
        }
    }
    if (e == hipSuccess && flush_bytes)
        e = launch_flush(h->d_flush, flush_bytes, h->stream, false);
    if (e == hipSuccess)
        e = launch_spmv_tile_stamped(h, *p, d_x, d_y, d_st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess && p->num_tiles)
        e = hipMemcpy(stamps, d_st, sizeof(unsigned long long) * (size_t)p->num_tiles * 6, hipMemcpyDeviceToHost);
    dev_free(d_st);
    if (e == hipErrorNotSupported) {
        (void)hipGetLastError();
        set_error("spmv_tile_stamps: this matrix's plain SpMV does not run k_spmv_tile on 256-thread tiles");
        return MSPMV_ERR_UNSUPPORTED;
    }
    HIP_TRY(e);
    return MSPMV_OK;
}

mspmv_status mspmv_check_faults(mspmv_handle h)
{
    ST_TRY(check_handle(h));
    HIP_TRY(hipStreamSynchronize(h->stream));
    unsigned f = 0;
    HIP_TRY(hipMemcpy(&f, h->d_fault, sizeof f, hipMemcpyDeviceToHost));
    if (!f)
        return MSPMV_OK;
    HIP_TRY(memset_sync(h->d_fault, 0, sizeof f));
    set_error("a fold ticket drew past its group (its array was not zero when the launch began): the products "
              "since the last check are invalid");
    return MSPMV_ERR_FAULT;
}

mspmv_status mspmv_test_poison_tickets(mspmv_handle h, unsigned value, int flags)
{
    ST_TRY(check_handle(h));
    if (flags & ~(MSPMV_POISON_FILL | MSPMV_POISON_LATE_ZERO | MSPMV_POISON_NO_STOP))
        return invalid("test_poison_tickets: unknown flag");
    h->poison_value = value;
    h->poison_flags = flags;
    return MSPMV_OK;
}


// ---- measurement ---------------------------------------------------------------------------
mspmv_status mspmv_time_stream_read(int device, size_t bytes, int reps, double *gbps)
{
    if (!gbps || reps < 1 || bytes < (1u << 20))
        return invalid("time_stream_read: gbps non-null, reps >= 1, bytes >= 1 MiB");
    HIP_TRY(hipSetDevice(device));
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    bytes &= ~(size_t)15;
    double *buf = nullptr;
    HIP_TRY(hipMalloc(&buf, bytes));
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = memset_sync(buf, 0, bytes);
    if (e == hipSuccess)
        e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess)
        e = hipEventCreate(&e0);
    if (e == hipSuccess)
        e = hipEventCreate(&e1);
    if (e == hipSuccess)
        e = launch_stream_read(buf, bytes, cus, s);  // warm-up
    if (e == hipSuccess)
        e = hipEventRecord(e0, s);
    for (int r = 0; r < reps && e == hipSuccess; ++r)
        e = launch_stream_read(buf, bytes, cus, s);
    if (e == hipSuccess)
        e = hipEventRecord(e1, s);
    if (e == hipSuccess)
        e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess)
        e = hipEventElapsedTime(&ms, e0, e1);
    if (e1)
        (void)hipEventDestroy(e1);
    if (e0)
        (void)hipEventDestroy(e0);
    if (s)
        (void)hipStreamDestroy(s);
    (void)hipFree(buf);
    if (e != hipSuccess) {
        set_error(std::string("time_stream_read: ") + hipGetErrorString(e));
        return MSPMV_ERR_HIP;
    }
    *gbps = ms > 0.f ? (double)bytes * reps / (ms * 1e-3) / 1e9 : 0.0;
    return MSPMV_OK;
}

mspmv_status mspmv_time_spmm_dev(mspmv_handle h, const double *d_X, double *d_Y, int L, int reps,
                                 size_t flush_bytes, double *avg_ms)
{
    ST_TRY(check_handle(h));
    if (reps < 1 || !avg_ms)
        return invalid("reps >= 1 and avg_ms required");
    if (!supported_L(L))
        return (set_error("L must be one of 1, 2, 4, 8, 16"), MSPMV_ERR_UNSUPPORTED);
    if (L > 1 && (!aligned16(d_X) || !aligned16(d_Y)))
        return invalid("multi-vector panels must be 16-byte aligned");
    const TilePlan *plan = nullptr;
    ST_TRY(product_plan(h, L, &plan));
    if (flush_bytes && flush_bytes > h->flush_cap) {
        if (h->d_flush)
            (void)hipFree(h->d_flush);
        h->d_flush = nullptr;
        h->flush_cap = 0;
        HIP_TRY(hipMalloc(&h->d_flush, flush_bytes));
        h->flush_cap = flush_bytes;
        HIP_TRY(launch_flush(h->d_flush, flush_bytes, h->stream, true));  // defined contents (+1.0)
    }
    // Hot (flush_bytes == 0): reps launches back to back, events around the region only; per launch
    // = region / reps (the launch gap included, ~0.2 us: r04i's headline 21.06 us against 21.09 in the
    // trace).  Cold: blocks of n (flush, launch) pairs, each beside a control block of n flushes alone;
    // per launch = the median over blocks of (pairs - control) / n.  Per-launch events (stream events,
    // or hipExtLaunchKernel's kernel-boundary ones) measured 4.7 us over the traced kernel on cant and
    // rma10 (r04i_frac_check.md); one control region for all reps left rma10 at 7.4 us against 9.5 in
    // the trace (r04m).  avg_ms: the timed regions per launch (flushes included).
    const bool run = plan->num_tiles > 0;
    const int nblk = flush_bytes && run ? std::min(reps, 8) : 1;
    std::vector<hipEvent_t> ev((size_t)nblk * 4, nullptr);
    for (auto &x : ev)
        HIP_TRY(hipEventCreate(&x));
    hipError_t e = hipSuccess;
    std::vector<int> nper((size_t)nblk);
    for (int b = 0, done = 0; b < nblk && e == hipSuccess; ++b) {
        const int n = (reps - done) / (nblk - b);
        nper[(size_t)b] = n;
        done += n;
        hipEvent_t *q = &ev[(size_t)b * 4];
        if (flush_bytes && run) {  // the control: n flushes alone
            e = hipEventRecord(q[2], h->stream);
            for (int i = 0; i < n && e == hipSuccess; ++i)
                e = launch_flush(h->d_flush, flush_bytes, h->stream, false);
            if (e == hipSuccess)
                e = hipEventRecord(q[3], h->stream);
        }
        if (e == hipSuccess)
            e = hipEventRecord(q[0], h->stream);
        for (int i = 0; i < n && e == hipSuccess && run; ++i) {
            if (flush_bytes)
                e = launch_flush(h->d_flush, flush_bytes, h->stream, false);
            if (e == hipSuccess)
                e = launch_spmm_tile_only(h, *plan, d_X, d_Y, L);
        }
        if (e == hipSuccess)
            e = hipEventRecord(q[1], h->stream);
    }
    if (e == hipSuccess)
        e = hipEventSynchronize(ev[(size_t)nblk * 4 - 3]);
    double total = 0.0;
    std::vector<double> per;
    for (int b = 0; b < nblk && e == hipSuccess; ++b) {
        float t = 0.f, c = 0.f;
        e = hipEventElapsedTime(&t, ev[(size_t)b * 4], ev[(size_t)b * 4 + 1]);
        if (e == hipSuccess && flush_bytes && run)
            e = hipEventElapsedTime(&c, ev[(size_t)b * 4 + 2], ev[(size_t)b * 4 + 3]);
        total += t;
        per.push_back(nper[(size_t)b] > 0 ? (double)(t - c) / nper[(size_t)b] : 0.0);
    }
    for (auto &x : ev)
        (void)hipEventDestroy(x);
    if (e != hipSuccess) {
        set_error(std::string("timing: ") + hipGetErrorString(e));
        return MSPMV_ERR_HIP;
    }
    std::sort(per.begin(), per.end());
    const double med = per.empty() ? 0.0 : per.size() % 2 ? per[per.size() / 2]
                                                         : 0.5 * (per[per.size() / 2 - 1] + per[per.size() / 2]);
    h->last_tile_kernel_ms = std::max(0.0, med);
    h->last_kernels_per_call = run ? 1 : 0;
    *avg_ms = total / reps;
    return MSPMV_OK;
}

}  // extern "C"

// ---- batched products: one product per handle, each on its handle's own stream ----------------
// Independent products on distinct streams may run at the same time, so a y that another product of the
// batch reads or writes would be a race: every y range [d_Y[i], +8 m_i L) must be disjoint from every other
// y range and from every x range [d_X[j], +8 n_j L), j = i included (x of a 0-row matrix is never read).
// A shared x is fine.
static mspmv_status batch_check_ranges(const char *who, int count, const mspmv_handle *hs, const double *const *d_X,
                                       double *const *d_Y, int L)
{
    auto hit = [](uintptr_t a, size_t na, uintptr_t b, size_t nb) { return na && nb && a < b + nb && b < a + na; };
    for (int i = 0; i < count; ++i) {
        const uintptr_t y = (uintptr_t)d_Y[i];
        const size_t ny = sizeof(double) * (size_t)hs[i]->m * L;
        for (int j = 0; j < count; ++j) {
            if (j > i && hit(y, ny, (uintptr_t)d_Y[j], sizeof(double) * (size_t)hs[j]->m * L))
                return invalid(std::string(who) + ": products " + std::to_string(i) + " and " + std::to_string(j) +
                               " write overlapping y ranges");
            if (hs[j]->m > 0 && hit(y, ny, (uintptr_t)d_X[j], sizeof(double) * (size_t)hs[j]->n * L))
                return invalid(std::string(who) + ": y of product " + std::to_string(i) + " overlaps x of product " +
                               std::to_string(j));
        }
    }
    return MSPMV_OK;
}

// The checks the batch entries share (same device, non-null vectors of non-empty products, 16-byte panels
// for L > 1) and each handle's plain plan for width L; *kps = products that launch a kernel.
static mspmv_status batch_plans(const char *who, int count, const mspmv_handle *hs, const double *const *d_X,
                                double *const *d_Y, int L, std::vector<const TilePlan *> &plans, int *kps)
{
    for (int i = 0; i < count; ++i) {
        ST_TRY(check_handle(hs[i]));
        if (hs[i]->device != hs[0]->device)
            return invalid(std::string(who) + ": batch handles must share a device (products 0 and " +
                           std::to_string(i) + ")");
        if (hs[i]->m > 0 && (!d_X[i] || !d_Y[i]))
            return invalid(std::string(who) + ": null vector");
        if (L > 1 && (!aligned16(d_X[i]) || !aligned16(d_Y[i])))
            return invalid("multi-vector panels must be 16-byte aligned");
    }
    ST_TRY(check_handle(hs[0]));
    plans.assign((size_t)count, nullptr);
    *kps = 0;
    for (int i = 0; i < count; ++i) {
        if (hs[i]->m == 0)  // no rows: no plan, no launch (as mspmv_dspmm_dev)
            continue;
        ST_TRY(product_plan(hs[i], L, &plans[(size_t)i]));
        *kps += plans[(size_t)i]->num_tiles ? 1 : 0;
    }
    return MSPMV_OK;
}

// MSPMV_BATCH_OVERLAP, read per call (one process can alternate the two forms of the timing entry):
// 0 = every launch of a step on hs[0]'s stream, back to back; otherwise product i on hs[i]'s own stream.
static bool batch_overlap_env()
{
    const char *v = getenv("MSPMV_BATCH_OVERLAP");
    return !(v && v[0] == '0');
}

mspmv_status mspmv::time_spmm_batch(int count, const mspmv_handle *hs, const double *const *d_X, double *const *d_Y,
                                    int L, int reps, double *step_ms, double *tile_kernel_ms, int *kernels_per_step,
                                    bool overlap)
{
    if (count < 1 || !hs || !d_X || !d_Y || reps < 1 || !step_ms)
        return invalid("bad batch timing arguments");
    if (!supported_L(L))
        return (set_error("L must be one of 1, 2, 4, 8, 16"), MSPMV_ERR_UNSUPPORTED);
    std::vector<const TilePlan *> plans;
    int kps = 0;
    ST_TRY(batch_plans("time_spmm_batch", count, hs, d_X, d_Y, L, plans, &kps));
    hipStream_t s = hs[0]->stream;
    // the other streams of the overlapped form (handles may share one: a CU-masked stream, a handle listed twice)
    std::vector<hipStream_t> others;
    for (int i = 1; i < count && overlap; ++i)
        if (hs[i]->stream != s && std::find(others.begin(), others.end(), hs[i]->stream) == others.end())
            others.push_back(hs[i]->stream);
    if (!others.empty())  // launches of one step may run together
        ST_TRY(batch_check_ranges("time_spmm_batch", count, hs, d_X, d_Y, L));
    for (int i = 0; i < count; ++i)  // everything after this point is ordered by the region's events
        HIP_TRY(hipStreamSynchronize(hs[i]->stream));
    // The timed steps: events only around the whole region (one kernel per product: split rows are closed
    // inside the tile kernel).  Single-stream form: every launch back to back on hs[0]'s stream.  Overlapped
    // form: product i on hs[i]'s own stream; the start event, on hs[0]'s stream, is waited on by every other
    // stream once, and each of those records one done event at the end that hs[0]'s stream waits on before
    // the end event -- 2 + one event per extra stream per region, nothing per step (an event per launch
    // costs 5-10 us, more than the fill and drain the overlap hides).
    std::vector<hipEvent_t> ev(2 + others.size(), nullptr);
    hipError_t e = hipSuccess;
    for (size_t k = 0; k < ev.size() && e == hipSuccess; ++k)
        e = k < 2 ? hipEventCreate(&ev[k]) : hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
    if (e == hipSuccess)
        e = hipEventRecord(ev[0], s);
    for (size_t k = 0; k < others.size() && e == hipSuccess; ++k)
        e = hipStreamWaitEvent(others[k], ev[0], 0);
    for (int r = 0; r < reps && e == hipSuccess; ++r)
        for (int i = 0; i < count && e == hipSuccess; ++i) {
            if (!plans[(size_t)i])
                continue;
            hipStream_t own = hs[i]->stream;
            if (!overlap)
                hs[i]->stream = s;
            e = launch_spmm_tile_only(hs[i], *plans[(size_t)i], d_X[i], d_Y[i], L);
            hs[i]->stream = own;
        }
    for (size_t k = 0; k < others.size() && e == hipSuccess; ++k) {
        e = hipEventRecord(ev[2 + k], others[k]);
        if (e == hipSuccess)
            e = hipStreamWaitEvent(s, ev[2 + k], 0);
    }
    if (e == hipSuccess)
        e = hipEventRecord(ev[1], s);
    if (e == hipSuccess)
        e = hipEventSynchronize(ev[1]);
    float total = 0.f;
    if (e == hipSuccess)
        e = hipEventElapsedTime(&total, ev[0], ev[1]);
    const double sum = (double)total;
    for (auto &x : ev)
        if (x)
            (void)hipEventDestroy(x);
    if (e != hipSuccess) {
        set_error(std::string("batch timing: ") + hipGetErrorString(e));
        return MSPMV_ERR_HIP;
    }
    *step_ms = (double)total / reps;
    if (tile_kernel_ms)
        *tile_kernel_ms = sum / ((double)reps * count);
    if (kernels_per_step)
        *kernels_per_step = kps;
    return MSPMV_OK;
}

extern "C" {

mspmv_status mspmv_time_spmm_batch_dev(int count, const mspmv_handle *hs, const double *const *d_X,
                                       double *const *d_Y, int L, int reps, double *step_ms, double *tile_kernel_ms,
                                       int *kernels_per_step)
{
    return mspmv::time_spmm_batch(count, hs, d_X, d_Y, L, reps, step_ms, tile_kernel_ms, kernels_per_step,
                                  batch_overlap_env());
}

mspmv_status mspmv_spmm_batch_dev(int count, const mspmv_handle *hs, const double *const *d_X, double *const *d_Y,
                                  int L)
{
    if (count < 1 || !hs || !d_X || !d_Y)
        return invalid("spmm_batch: count >= 1 and non-null arrays required");
    if (!supported_L(L))
        return invalid("spmm_batch: L must be one of 1, 2, 4, 8, 16");
    std::vector<const TilePlan *> plans;
    int kps = 0;
    ST_TRY(batch_plans("spmm_batch", count, hs, d_X, d_Y, L, plans, &kps));
    ST_TRY(batch_check_ranges("spmm_batch", count, hs, d_X, d_Y, L));
    // Product i on hs[i]'s own stream, by the launch path of a single product: no events, no waits between
    // streams, no host sync.  Stream order on each handle is all the ordering there is.
    for (int i = 0; i < count; ++i) {
        mspmv_handle_s *h = hs[i];
        if (!plans[(size_t)i])
            continue;
        const TilePlan &plan = *plans[(size_t)i];
        // test hook (mspmv_test_poison_tickets): this product meets dirty split-row tickets, as an unordered
        // zeroing leaves them; zeroed again behind it, so the handle's next product is clean
        const bool poison = (h->poison_flags & MSPMV_POISON_FILL) && plan.num_carries && plan.d_fix_cnt;
        if (poison) {
            h->poison_flags = 0;
            HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)plan.d_fix_cnt, (int)h->poison_value, (size_t)plan.num_tiles,
                                      h->stream));
        }
        HIP_TRY(launch_spmm_tile_only(h, plan, d_X[i], d_Y[i], L));
        if (poison)
            HIP_TRY(hipMemsetAsync(plan.d_fix_cnt, 0, sizeof(unsigned) * (size_t)plan.num_tiles, h->stream));
    }
    return MSPMV_OK;
}

mspmv_status mspmv_sync_batch(int count, const mspmv_handle *hs)
{
    if (count < 1 || !hs)
        return invalid("sync_batch: count >= 1 and handles required");
    // every stream drained and every fault word read (and cleared) even when an earlier handle reports
    mspmv_status st = MSPMV_OK;
    std::string msg;
    for (int i = 0; i < count; ++i) {
        const mspmv_status si = mspmv_check_faults(hs[i]);
        if (si != MSPMV_OK && st == MSPMV_OK) {
            st = si;
            msg = "product " + std::to_string(i) + ": " + mspmv_last_error();
        }
    }
    if (st != MSPMV_OK)
        set_error(msg);
    return st;
}

mspmv_status mspmv_last_kernel_ms(mspmv_handle h, double *tile_kernel_ms, int *kernels_per_call)
{
    if (!h)
        return invalid("null handle");
    if (tile_kernel_ms)
        *tile_kernel_ms = h->last_tile_kernel_ms;
    if (kernels_per_call)
        *kernels_per_call = h->last_kernels_per_call;
    return MSPMV_OK;
}

mspmv_status mspmv_tile_plan(mspmv_handle h, int L, int *num_tiles, int *tile_items, int *num_carries,
                             mspmv_coord *bounds)
{
    ST_TRY(check_handle(h));
    if (!supported_L(L))
        return (set_error("L must be one of 1, 2, 4, 8, 16"), MSPMV_ERR_UNSUPPORTED);
    const TilePlan *plan = nullptr;
    ST_TRY(product_plan(h, L, &plan));
    if (num_tiles)
        *num_tiles = plan->num_tiles;
    if (tile_items)
        *tile_items = plan->tile_items;
    if (num_carries)
        *num_carries = plan->num_carries;
    if (bounds)
        HIP_TRY(hipMemcpy(bounds, plan->d_bounds, sizeof(int2) * (plan->num_tiles + 1), hipMemcpyDeviceToHost));
    return MSPMV_OK;
}

mspmv_status mspmv_tile_modes(mspmv_handle h, int L, unsigned char *modes)
{
    ST_TRY(check_handle(h));
    if (!supported_L(L))
        return (set_error("L must be one of 1, 2, 4, 8, 16"), MSPMV_ERR_UNSUPPORTED);
    if (!modes)
        return invalid("null modes");
    const TilePlan *plan = nullptr;
    ST_TRY(product_plan(h, L, &plan));
    if (plan->num_tiles)
        HIP_TRY(hipMemcpy(modes, plan->d_modes[l_index(L)], plan->num_tiles, hipMemcpyDeviceToHost));
    // node-block tiles reduced in registers (lane tree, not the plan's mode): L = 1 on any plan
    // with node blocks, L > 1 when product_plan chose the node-block plan (k_spmm_blk)
    if (plan->d_blk && (L == 1 || plan->num_tiles_reg == plan->num_tiles))
        for (int t = 0; t < plan->num_tiles; ++t)
            if (plan->h_blk_reg[(size_t)t])
                modes[t] = 255;
    return MSPMV_OK;
}

mspmv_status mspmv_tile_lanes(mspmv_handle h, int L, int *lanes)
{
    ST_TRY(check_handle(h));
    if (!lanes)
        return invalid("null out pointer");
    if (!supported_L(L))
        return (set_error("L must be one of 1, 2, 4, 8, 16"), MSPMV_ERR_UNSUPPORTED);
    const TilePlan *plan = nullptr;
    ST_TRY(product_plan(h, L, &plan));
    *lanes = L == 1 ? plan->lanes : kBlock;
    return MSPMV_OK;
}

mspmv_status mspmv_tile_streams(mspmv_handle h, int *tiles_cols16, int *tiles_dict)
{
    ST_TRY(check_handle(h));
    const TilePlan *plan = nullptr;
    ST_TRY(product_plan(h, 1, &plan));
    if (tiles_cols16)
        *tiles_cols16 = plan->d_cols16 ? plan->num_tiles16 : 0;
    if (tiles_dict)
        *tiles_dict = plan->d_dict ? plan->num_tiles_dict : 0;
    return MSPMV_OK;
}

mspmv_status mspmv_plan_block_tiles(mspmv_handle h, int L, int *tiles_blk)
{
    ST_TRY(check_handle(h));
    if (!tiles_blk)
        return invalid("null out pointer");
    if (!supported_L(L))
        return (set_error("L must be one of 1, 2, 4, 8, 16"), MSPMV_ERR_UNSUPPORTED);
    const TilePlan *plan = nullptr;
    ST_TRY(product_plan(h, L, &plan));
    *tiles_blk = plan->d_blk ? plan->num_tiles_blk : 0;
    return MSPMV_OK;
}

mspmv_status mspmv_plan_block_rounds(mspmv_handle h, int L, int *tiles_two_rounds)
{
    ST_TRY(check_handle(h));
    if (!tiles_two_rounds)
        return invalid("null out pointer");
    if (!supported_L(L))
        return (set_error("L must be one of 1, 2, 4, 8, 16"), MSPMV_ERR_UNSUPPORTED);
    const TilePlan *plan = nullptr;
    ST_TRY(product_plan(h, L, &plan));
    *tiles_two_rounds = plan->d_blk ? plan->blk_two_rounds : 0;
    return MSPMV_OK;
}

mspmv_status mspmv_plan_block_records(mspmv_handle h, int L, int *chunks_compact, int *chunks_escaped)
{
    ST_TRY(check_handle(h));
    if (!chunks_compact || !chunks_escaped)
        return invalid("null out pointer");
    if (!supported_L(L))
        return (set_error("L must be one of 1, 2, 4, 8, 16"), MSPMV_ERR_UNSUPPORTED);
    const TilePlan *plan = nullptr;
    ST_TRY(product_plan(h, L, &plan));
    *chunks_compact = plan->d_recs ? plan->blk_rec_compact : 0;
    *chunks_escaped = plan->d_recs ? plan->blk_rec_escaped : 0;
    return MSPMV_OK;
}

mspmv_status mspmv_slab_plan_stats(mspmv_handle h, int L, long long *stats, int count, int *on_slab)
{
    ST_TRY(check_handle(h));
    if (!on_slab || (count > 0 && !stats))
        return invalid("null out pointer");
    if (!supported_L(L))
        return (set_error("L must be one of 1, 2, 4, 8, 16"), MSPMV_ERR_UNSUPPORTED);
    const TilePlan *plan = nullptr;
    ST_TRY(product_plan(h, L, &plan));
    *on_slab = plan->slab ? 1 : 0;
    if (!plan->slab)
        return MSPMV_OK;
    SlabStats s = plan->slab->stats;
    s.v[MSPMV_SLAB_STAT_BLOCKS] = plan->num_tiles;
    s.v[MSPMV_SLAB_STAT_GROUPS] = plan->slab->groups;
    s.v[MSPMV_SLAB_STAT_CARRIES] = plan->num_carries;
    for (int i = 0; i < count && i < MSPMV_SLAB_STAT_COUNT; ++i)
        stats[i] = s.v[i];
    return MSPMV_OK;
}

mspmv_status mspmv_block_record_encode(const unsigned short *offsets, int wc, unsigned *entries, int *escaped)
{
    if (!entries || !escaped || (wc > 0 && !offsets))
        return invalid("null pointer");
    if (wc < 0 || wc > 64)
        return invalid("a chunk holds 0..64 pattern columns");
    *escaped = blk_rec_encode(offsets, wc, entries) ? 0 : 1;
    return MSPMV_OK;
}

mspmv_status mspmv_block_record_decode(const unsigned *record, int q, unsigned *offset)
{
    if (!record || !offset)
        return invalid("null pointer");
    if (q < 0)
        return invalid("q >= 0");
    *offset = blk_rec_decode(record + 4, (int)(record[0] >> 24), q);
    return MSPMV_OK;
}

mspmv_status mspmv_plan_dict_tiles(mspmv_handle h, int L, int *tiles_dict)
{
    ST_TRY(check_handle(h));
    if (!tiles_dict)
        return invalid("null out pointer");
    if (!supported_L(L))
        return (set_error("L must be one of 1, 2, 4, 8, 16"), MSPMV_ERR_UNSUPPORTED);
    const TilePlan *plan = nullptr;
    ST_TRY(product_plan(h, L, &plan));
    *tiles_dict = plan->d_dict && (L == 1 || L == 16) ? plan->num_tiles_dict : 0;
    return MSPMV_OK;
}

// ---- device memory helpers -----------------------------------------------------------------
mspmv_status mspmv_device_malloc(int device, size_t bytes, void **d_ptr)
{
    if (!d_ptr)
        return invalid("null out pointer");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc(d_ptr, bytes ? bytes : 1));
    return MSPMV_OK;
}

mspmv_status mspmv_device_free(void *d_ptr)
{
    if (d_ptr)
        HIP_TRY(hipFree(d_ptr));
    return MSPMV_OK;
}

mspmv_status mspmv_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes)
{
    HIP_TRY(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return MSPMV_OK;
}

mspmv_status mspmv_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes)
{
    HIP_TRY(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return MSPMV_OK;
}

mspmv_status mspmv_memcpy_d2d(void *d_dst, const void *d_src, size_t bytes)
{
    HIP_TRY(hipMemcpy(d_dst, d_src, bytes, hipMemcpyDeviceToDevice));
    return MSPMV_OK;
}

mspmv_status mspmv_memset_dev(void *d_dst, int byte_value, size_t bytes)
{
    HIP_TRY(memset_sync(d_dst, byte_value, bytes));
    return MSPMV_OK;
}

}  // extern "C"

// mspmv_streams.cpp -- the per-device stream-slot ledger (include/mspmv.h, "Stream pool").  Host only, no HIP
// call: the streams themselves, one per slot, are created and kept by mspmv_api.hip (pool_stream).
//
// One ledger per device ordinal: kStreamPool slots, each free or held by one handle.  A take gets the lowest
// free slot, so the same sequence of creates and destroys always puts the same handle on the same stream; a
// lease is exclusive, and a give of a slot nobody holds is refused.
#include <map>
#include <mutex>

#include "mspmv_host.h"

namespace {

using mspmv::kStreamPool;

struct Slots {
    bool held[kStreamPool] = {};
};

std::mutex g_mu;
std::map<int, Slots> g_slots;

}  // namespace

extern "C" {

mspmv_status mspmv_stream_slot_take(int device, int *slot)
{
    if (device < 0 || !slot)
        return mspmv::invalid("stream_slot_take: bad arguments");
    std::lock_guard<std::mutex> lk(g_mu);
    Slots &s = g_slots[device];
    *slot = -1;
    for (int i = 0; i < kStreamPool && *slot < 0; ++i)
        if (!s.held[i]) {
            s.held[i] = true;
            *slot = i;
        }
    return MSPMV_OK;
}

mspmv_status mspmv_stream_slot_give(int device, int slot)
{
    if (device < 0 || slot < 0 || slot >= kStreamPool)
        return mspmv::invalid("stream_slot_give: no such slot");
    std::lock_guard<std::mutex> lk(g_mu);
    Slots &s = g_slots[device];
    if (!s.held[slot])
        return mspmv::invalid("stream_slot_give: the slot is not held");
    s.held[slot] = false;
    return MSPMV_OK;
}

mspmv_status mspmv_stream_pool_stats(int device, int *slots, int *leased)
{
    if (device < 0)
        return mspmv::invalid("stream_pool_stats: negative device");
    std::lock_guard<std::mutex> lk(g_mu);
    const Slots &s = g_slots[device];
    if (slots)
        *slots = kStreamPool;
    if (leased) {
        *leased = 0;
        for (int i = 0; i < kStreamPool; ++i)
            *leased += s.held[i] ? 1 : 0;
    }
    return MSPMV_OK;
}

}  // extern "C"

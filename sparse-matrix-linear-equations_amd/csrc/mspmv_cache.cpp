// mspmv_cache.cpp -- the per-device Infinity-Cache ledger (include/mspmv.h, "Infinity-Cache leases").  Host
// only: the handles' side (what a plan streams, when a handle asks) is mspmv_plan.hip's cache_book.
//
// One ledger per device ordinal: a budget, a floor and the sum of the live leases.  A lease is a number of
// bytes, held by its handle; the ledger keeps no list of holders, so a handle's decision is never revisited
// behind its back -- the same creation order always gives the same choices.
#include <cstdlib>
#include <map>
#include <mutex>

#include "mspmv_host.h"

namespace {

constexpr long long kMiB = 1024 * 1024;
// The built-in budget: the largest resident total that still ran the headline batch at its best (three of its
// four 95 MB matrices, 271.5 MiB; all four lost 2 us per step), rounded down to 16 MiB -- DESIGN 3,
// profiles/r09a_cache_policy_probe.json.  MSPMV_CACHE_MIB replaces it.
constexpr long long kDefaultBudget = 256 * kMiB;
// At most this much of a matrix stream keeps the default policy without a lease: the eight 4 MiB L2s together.
constexpr long long kDefaultFloor = 32 * kMiB;

struct Ledger {
    long long budget, floor, leased = 0;
};

std::mutex g_mu;
std::map<int, Ledger> g_ledgers;

long long default_budget()
{
    static const long long v = [] {
        const char *e = getenv("MSPMV_CACHE_MIB");
        if (e && *e) {
            char *end = nullptr;
            const long long mib = strtoll(e, &end, 10);
            if (end != e && mib >= 0)
                return mib * kMiB;
        }
        return kDefaultBudget;
    }();
    return v;
}

Ledger &ledger(int device)  // g_mu held
{
    auto it = g_ledgers.find(device);
    if (it == g_ledgers.end())
        it = g_ledgers.emplace(device, Ledger{default_budget(), kDefaultFloor}).first;
    return it->second;
}

mspmv_status exchange(int device, long long bytes, long long *old, long long Ledger::*field)
{
    if (device < 0)
        return mspmv::invalid("cache ledger: negative device");
    std::lock_guard<std::mutex> lk(g_mu);
    Ledger &l = ledger(device);
    if (old)
        *old = l.*field;
    if (bytes >= 0)
        l.*field = bytes;
    return MSPMV_OK;
}

}  // namespace

extern "C" {

mspmv_status mspmv_cache_budget(int device, long long bytes, long long *old)
{
    return exchange(device, bytes, old, &Ledger::budget);
}

mspmv_status mspmv_cache_floor(int device, long long bytes, long long *old)
{
    return exchange(device, bytes, old, &Ledger::floor);
}

mspmv_status mspmv_cache_lease(int device, long long held, long long want, int policy, long long *granted,
                               int *resident)
{
    if (device < 0 || held < 0 || want < 0 || !granted || !resident)
        return mspmv::invalid("cache_lease: bad arguments");
    if (policy != MSPMV_CACHE_AUTO && policy != MSPMV_CACHE_STREAM && policy != MSPMV_CACHE_RESIDENT)
        return mspmv::invalid("cache_lease: unknown policy");
    std::lock_guard<std::mutex> lk(g_mu);
    Ledger &l = ledger(device);
    if (held > l.leased)
        return mspmv::invalid("cache_lease: more bytes returned than are leased");
    const long long others = l.leased - held;
    long long g = 0;
    bool res;
    if (policy == MSPMV_CACHE_STREAM) {
        res = false;
    } else if (policy == MSPMV_CACHE_RESIDENT) {
        res = true;
        g = want;  // booked whatever the budget says: later requests see it
    } else if (want <= l.floor) {
        res = true;  // fits the L2s: as every small matrix always ran, and nothing to book
    } else {
        res = others + want <= l.budget;
        g = res ? want : 0;
    }
    l.leased = others + g;
    *granted = g;
    *resident = res ? 1 : 0;
    return MSPMV_OK;
}

mspmv_status mspmv_cache_leased(int device, long long *bytes)
{
    if (device < 0 || !bytes)
        return mspmv::invalid("cache_leased: bad arguments");
    std::lock_guard<std::mutex> lk(g_mu);
    *bytes = ledger(device).leased;
    return MSPMV_OK;
}

}  // extern "C"

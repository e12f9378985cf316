// link_host.h — the host-side arithmetic of the link table (capi_link.hip):
// capacity rounding and the bookkeeping that decides when the slots lost to
// removals are reclaimed.  Plain C++ with no HIP in it, so that
// tests/link_host/ can build it alone under the sanitizers.
#pragma once
#include <stdint.h>

namespace rnstok {

// A slot word keeps 30 bits for a batch index, and the slot number shares the
// status word with a flag while an insert is in flight: 2^30 slots at most.
constexpr uint32_t LINK_MAX_CAPACITY = 1u << 30;
// Items per call: batch indices stay below the all-ones index of a settled slot.
constexpr uint32_t LINK_MAX_BATCH = (1u << 30) - 2u;

// The smallest power of two that is at least 2 * max_links; 0 where max_links
// is 0 or needs more than LINK_MAX_CAPACITY slots.
inline uint32_t link_capacity(uint32_t max_links) {
    if (max_links == 0 || max_links > LINK_MAX_CAPACITY / 2) return 0;
    uint32_t c = 2;
    while (c < 2 * max_links) c <<= 1;
    return c;
}

// What the host knows about a table without asking the device.  A slot is
// used when it holds an entry or the mark a removal leaves (a removed slot is
// not handed out as empty, because probe chains run through it); `used_ub`
// never falls below the number of used slots.  An insert of n items enqueues a
// rebuild first when removals were enqueued since the last rebuild and
// used_ub + n would pass three quarters of the capacity: after a rebuild the
// used slots are the live entries alone, so an insert meets a full table only
// when live entries + new ids exceed the capacity itself.  The rebuild reports
// the live count back (link tickets, capi_link.hip); until that report is read
// the bound stays at its earlier, larger value.
struct LinkBook {
    uint32_t cap = 0;
    uint32_t used_ub = 0;          // upper bound on used slots
    uint32_t since_rebuild = 0;    // items of the inserts enqueued after the last rebuild (saturates at cap)
    uint32_t removes = 0;          // items of the removes enqueued after the last rebuild (saturates)
    bool awaiting = false;         // a rebuild is enqueued whose live count has not been read

    uint32_t threshold() const { return cap - cap / 4; }
    bool needs_rebuild(uint32_t n) const { return removes != 0 && (uint64_t)used_ub + n > threshold(); }
    void on_rebuild() {
        since_rebuild = 0;
        removes = 0;
        awaiting = true;
    }
    // The live count the latest enqueued rebuild found.
    void on_report(uint32_t live) {
        if (!awaiting) return;
        const uint64_t u = (uint64_t)live + since_rebuild;
        used_ub = u > cap ? cap : (uint32_t)u;
        awaiting = false;
    }
    void on_insert(uint32_t n) {
        const uint64_t u = (uint64_t)used_ub + n, r = (uint64_t)since_rebuild + n;
        used_ub = u > cap ? cap : (uint32_t)u;
        since_rebuild = r > cap ? cap : (uint32_t)r;
    }
    void on_remove(uint32_t n) {
        const uint64_t r = (uint64_t)removes + n;
        removes = r > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)r;
    }
};

}  // namespace rnstok

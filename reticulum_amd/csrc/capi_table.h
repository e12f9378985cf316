// capi_table.h — what the C-ABI's device tables share (capi_link.hip,
// capi_filter.hip, capi_proof.hip): the link table's record, which the packet
// filter reads as its transit table and the proofs as their receipts, the frame
// that puts the calls on one table in host order, and how a table's memory
// comes and goes.
#pragma once
#include "capi_internal.h"
#include "link_host.h"

struct rt_linktable {
    rt_ctx *ctx = nullptr;
    LinkTab t{};
    // Calls take effect in host order: `done` is recorded after each call's
    // launches on its stream `last`, and a call on another stream waits for it.
    std::mutex mu;
    hipStream_t last = nullptr;
    hipEvent_t done = nullptr;
    LinkBook book;
    uint32_t report = 0;           // this table's word of ctx->h_link_report
    uint32_t ticket = 0;           // of the latest rebuild enqueued
};

// The packet hash list (capi_filter.hip; the link request proofs enter hashes
// into it, capi_lrproof.hip), ordered as a table is.
struct rt_hashlist {
    rt_ctx *ctx = nullptr;
    HashList l{};
    std::mutex mu;
    hipStream_t last = nullptr;
    hipEvent_t done = nullptr;
};

// Before an insert of n items, with the table's lock held: enqueues the rebuild
// that reclaims removed slots when the table's book asks for one (capi_link.hip).
hipError_t link_reclaim(rt_linktable *tab, uint32_t n, hipStream_t s);

inline int check_batch(uint32_t n, const char *who) {
    if (n > LINK_MAX_BATCH) return fail(RT_E_INVAL, std::string(who) + ": at most 2^30 - 2 items per call");
    return RT_OK;
}

// One call on a table (a record with ctx, mu, last and done): holds the
// table's lock, orders the stream after the call before, runs `body` (its
// launches on s; an RT_* code), and records the call on the way out.
// `ordering` names the table where one of those steps fails.
template <class Table, class Body>
int table_call(Table *tab, hipStream_t s, const char *ordering, Body body) {
    std::lock_guard<std::mutex> g(tab->mu);
    RT_HIP(hipSetDevice(tab->ctx->device), ordering);
    if (s != tab->last) RT_HIP(hipStreamWaitEvent(s, tab->done, 0), ordering);
    RT_TRY(body());
    tab->last = s;
    RT_HIP(hipEventRecord(tab->done, s), ordering);
    return RT_OK;
}

// A new table's memory (tab->ctx set): one allocation of tail_at + tail_bytes
// on the reclaim stream, its first `zeroed` bytes (the slot words) and its tail
// (the counts) set to 0; what lies between is read only behind a FULL word.
// Null, with `tab` deleted and the error set, when a step fails.
template <class Table>
uint8_t *table_alloc(Table *tab, const char *what, uint64_t zeroed, uint64_t tail_at, uint64_t tail_bytes) {
    rt_ctx *c = tab->ctx;
    hipStream_t s = c->stream;
    uint8_t *base = nullptr;
    hipError_t e = hipEventCreateWithFlags(&tab->done, hipEventDisableTiming);
    if (e == hipSuccess) e = rec_alloc(c, tail_at + tail_bytes, (uint32_t **)&base, s);
    if (e != hipSuccess) {
        fail(RT_E_NOMEM, std::string(what) + " allocation failed: " + hipGetErrorString(e));
    } else if ((e = hipMemsetAsync(base, 0, zeroed, s)) != hipSuccess ||
               (e = hipMemsetAsync(base + tail_at, 0, tail_bytes, s)) != hipSuccess ||
               (e = hipEventRecord(tab->done, s)) != hipSuccess) {
        hip_fail(e, (std::string(what) + " setup").c_str());
        hipFreeAsync(base, s);
    } else {
        tab->last = s;
        return base;
    }
    if (tab->done) hipEventDestroy(tab->done);
    delete tab;
    return nullptr;
}

// No synchronisation: the memory goes back on the reclaim stream after the
// last call on the table.
template <class Table>
void table_free(Table *tab, void *base) {
    rt_ctx *c = tab->ctx;
    hipSetDevice(c->device);
    hipStreamWaitEvent(c->stream, tab->done, 0);
    hipFreeAsync(base, c->stream);
    hipEventDestroy(tab->done);
    delete tab;
}

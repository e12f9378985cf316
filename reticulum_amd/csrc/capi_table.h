// capi_table.h — what the C-ABI's device tables share (capi_link.hip,
// capi_filter.hip): the link table's record, which the packet filter reads as
// its transit table, and the frame that puts the calls on one table in host
// order.
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

// The frame of one call on a table (a record with ctx, mu, last and done):
// holds the table's lock, orders the stream after the call before, and records
// the call on the way out.
template <class Table>
class TableCall {
public:
    TableCall(Table *tab, hipStream_t s) : tab_(tab), s_(s), g_(tab->mu) {}
    hipError_t begin() {
        hipError_t e = hipSetDevice(tab_->ctx->device);
        if (e == hipSuccess && s_ != tab_->last) e = hipStreamWaitEvent(s_, tab_->done, 0);
        return e;
    }
    hipError_t end() {
        tab_->last = s_;
        return hipEventRecord(tab_->done, s_);
    }

private:
    Table *tab_;
    hipStream_t s_;
    std::lock_guard<std::mutex> g_;
};

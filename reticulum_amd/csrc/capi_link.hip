// capi_link.hip — the link table of the C-ABI: a device-resident map from
// link id to the caller's value, and the dispatch of unpacked packets through
// it.  Device pointers on the caller's stream; the *_host calls go through a
// staging lane (capi_internal.h).  The kernels are in link_kernels.hip, the
// host-side arithmetic in link_host.h.
#include "capi_table.h"

namespace {

int check_table(const rt_linktable *tab) {
    if (!tab || !tab->ctx || !tab->t.slots) return fail(RT_E_INVAL, "null link table");
    return RT_OK;
}

// The mapped words the rebuilds report into, made with the context's first table.
bool ensure_reports(rt_ctx *c) {
    std::lock_guard<std::mutex> g(c->link_mu);
    if (c->h_link_report) return true;
    void *h = nullptr, *d = nullptr;
    if (hipHostMalloc(&h, 8ull * rt_ctx::LINK_REPORTS, hipHostMallocMapped) != hipSuccess) return false;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        hipHostFree(h);
        return false;
    }
    memset(h, 0, 8ull * rt_ctx::LINK_REPORTS);
    c->h_link_report = (uint64_t *)h;
    c->d_link_report = (uint64_t *)d;
    return true;
}

}  // namespace

// Before an insert of n items (table lock held): read the latest rebuild's
// report if it has arrived, and enqueue a rebuild when the bound asks for one.
hipError_t link_reclaim(rt_linktable *tab, uint32_t n, hipStream_t s) {
    rt_ctx *c = tab->ctx;
    LinkBook &b = tab->book;
    if (b.awaiting) {
        const uint64_t r = __atomic_load_n(c->h_link_report + tab->report, __ATOMIC_ACQUIRE);
        if ((uint32_t)(r >> 32) == tab->ticket) b.on_report((uint32_t)r);
    }
    if (!b.needs_rebuild(n)) return hipSuccess;
    void *ws = nullptr;
    hipError_t e = rec_alloc(c, link_rebuild_workspace_bytes(tab->t.cap), (uint32_t **)&ws, s);
    if (e != hipSuccess) return e;
    tab->ticket = c->link_ticket.fetch_add(1u, std::memory_order_relaxed) + 1u;
    e = launch_link_rebuild(tab->t, ws, c->d_link_report + tab->report, tab->ticket, s);
    const hipError_t f = hipFreeAsync(ws, s);
    if (e == hipSuccess) b.on_rebuild();
    return e != hipSuccess ? e : f;
}

namespace {

int insert_on(rt_linktable *tab, const uint8_t *ids, const uint32_t *values, int32_t *status, uint32_t n,
              hipStream_t s) {
    return table_call(tab, s, "link table ordering", [&] {
        RT_HIP(link_reclaim(tab, n, s), "link table rebuild");
        RT_HIP(launch_link_insert(tab->t, ids, values, status, n, s), "link insert");
        tab->book.on_insert(n);
        return RT_OK;
    });
}
int remove_on(rt_linktable *tab, const uint8_t *ids, int32_t *status, uint32_t n, hipStream_t s) {
    return table_call(tab, s, "link table ordering", [&] {
        RT_HIP(launch_link_remove(tab->t, ids, status, n, s), "link remove");
        tab->book.on_remove(n);
        return RT_OK;
    });
}
int lookup_on(rt_linktable *tab, const uint8_t *ids, uint32_t *values_out, uint8_t *found_out, uint32_t n,
              hipStream_t s) {
    return table_call(tab, s, "link table ordering", [&] {
        RT_HIP(launch_link_lookup(tab->t, ids, values_out, found_out, n, s), "link lookup");
        return RT_OK;
    });
}

}  // namespace

extern "C" {

rt_linktable *rt_linktable_create(rt_ctx *c, uint32_t max_links) {
    if (!c) {
        fail(RT_E_INVAL, "null context");
        return nullptr;
    }
    const uint32_t cap = link_capacity(max_links);
    if (cap == 0) {
        fail(RT_E_INVAL, "rt_linktable_create: max_links must be 1 .. 2^29");
        return nullptr;
    }
    hipSetDevice(c->device);
    if (!ensure_reports(c)) {
        fail(RT_E_NOMEM, "rt_linktable_create: pinned allocation failed");
        return nullptr;
    }
    rt_linktable *tab = new rt_linktable();
    tab->ctx = c;
    tab->book.cap = cap;
    {
        std::lock_guard<std::mutex> g(c->link_mu);
        tab->report = c->link_next++ % rt_ctx::LINK_REPORTS;
    }
    // slot words, ids, values, live count
    uint8_t *base = table_alloc(tab, "link table", 8ull * cap, 28ull * cap, 16);
    if (!base) return nullptr;
    tab->t = LinkTab{(uint64_t *)base, base + 8ull * cap, (uint32_t *)(base + 24ull * cap),
                     (uint32_t *)(base + 28ull * cap), cap};
    return tab;
}

void rt_linktable_destroy(rt_linktable *tab) {
    if (tab) table_free(tab, tab->t.slots);
}

uint32_t rt_linktable_capacity(const rt_linktable *tab) { return tab ? tab->t.cap : 0; }

int rt_linktable_insert(rt_linktable *tab, const uint8_t *ids, const uint32_t *values, int32_t *status, uint32_t n,
                        void *stream) {
    RT_TRY(check_table(tab));
    RT_TRY(check_batch(n, "rt_linktable_insert"));
    if (n == 0) return RT_OK;
    if (!ids || !values || !status) return fail(RT_E_INVAL, "rt_linktable_insert: null buffer");
    return insert_on(tab, ids, values, status, n, as_stream(stream));
}

int rt_linktable_remove(rt_linktable *tab, const uint8_t *ids, int32_t *status, uint32_t n, void *stream) {
    RT_TRY(check_table(tab));
    RT_TRY(check_batch(n, "rt_linktable_remove"));
    if (n == 0) return RT_OK;
    if (!ids || !status) return fail(RT_E_INVAL, "rt_linktable_remove: null buffer");
    return remove_on(tab, ids, status, n, as_stream(stream));
}

int rt_linktable_lookup(rt_linktable *tab, const uint8_t *ids, uint32_t *values_out, uint8_t *found_out, uint32_t n,
                        void *stream) {
    RT_TRY(check_table(tab));
    RT_TRY(check_batch(n, "rt_linktable_lookup"));
    if (n == 0) return RT_OK;
    if (!ids || !values_out || !found_out) return fail(RT_E_INVAL, "rt_linktable_lookup: null buffer");
    return lookup_on(tab, ids, values_out, found_out, n, as_stream(stream));
}

int rt_linktable_count(rt_linktable *tab, uint32_t *count_out, void *stream) {
    RT_TRY(check_table(tab));
    if (!count_out) return fail(RT_E_INVAL, "rt_linktable_count: null count_out");
    hipStream_t s = as_stream(stream);
    return table_call(tab, s, "link table ordering", [&] {
        RT_HIP(hipMemcpyAsync(count_out, tab->t.live, 4, hipMemcpyDeviceToDevice, s), "link count");
        return RT_OK;
    });
}

int rt_linktable_insert_host(rt_linktable *tab, const uint8_t *ids, const uint32_t *values, int32_t *status,
                             uint32_t n) {
    RT_TRY(check_table(tab));
    RT_TRY(check_batch(n, "rt_linktable_insert_host"));
    if (n == 0) return RT_OK;
    if (!ids || !values || !status) return fail(RT_E_INVAL, "rt_linktable_insert_host: null buffer");
    HostCall hc(tab->ctx, HostCall::PER_ARRAY);
    const uint64_t o_ids = hc.add(16ull * n), o_val = hc.add(4ull * n), o_st = hc.add(4ull * n);
    RT_TRY(hc.open());
    hc.put(o_ids, ids, 16ull * n, "H2D ids");
    hc.put(o_val, values, 4ull * n, "H2D values");
    RT_TRY(hc.send());
    RT_TRY(insert_on(tab, hc.dev<uint8_t>(o_ids), hc.dev<uint32_t>(o_val), hc.dev<int32_t>(o_st), n, hc.stream()));
    hc.get(status, o_st, 4ull * n, "D2H status");
    return hc.finish();
}

int rt_linktable_remove_host(rt_linktable *tab, const uint8_t *ids, int32_t *status, uint32_t n) {
    RT_TRY(check_table(tab));
    RT_TRY(check_batch(n, "rt_linktable_remove_host"));
    if (n == 0) return RT_OK;
    if (!ids || !status) return fail(RT_E_INVAL, "rt_linktable_remove_host: null buffer");
    HostCall hc(tab->ctx, HostCall::PER_ARRAY);
    const uint64_t o_ids = hc.add(16ull * n), o_st = hc.add(4ull * n);
    RT_TRY(hc.open());
    hc.put(o_ids, ids, 16ull * n, "H2D ids");
    RT_TRY(hc.send());
    RT_TRY(remove_on(tab, hc.dev<uint8_t>(o_ids), hc.dev<int32_t>(o_st), n, hc.stream()));
    hc.get(status, o_st, 4ull * n, "D2H status");
    return hc.finish();
}

int rt_linktable_lookup_host(rt_linktable *tab, const uint8_t *ids, uint32_t *values_out, uint8_t *found_out,
                             uint32_t n) {
    RT_TRY(check_table(tab));
    RT_TRY(check_batch(n, "rt_linktable_lookup_host"));
    if (n == 0) return RT_OK;
    if (!ids || !values_out || !found_out) return fail(RT_E_INVAL, "rt_linktable_lookup_host: null buffer");
    HostCall hc(tab->ctx, HostCall::PER_ARRAY);
    const uint64_t o_ids = hc.add(16ull * n), o_val = hc.add(4ull * n), o_found = hc.add(n);
    RT_TRY(hc.open());
    hc.put(o_ids, ids, 16ull * n, "H2D ids");
    RT_TRY(hc.send());
    RT_TRY(lookup_on(tab, hc.dev<uint8_t>(o_ids), hc.dev<uint32_t>(o_val), hc.dev<uint8_t>(o_found), n, hc.stream()));
    hc.get(values_out, o_val, 4ull * n, "D2H values");
    hc.get(found_out, o_found, n, "D2H found");
    return hc.finish();
}

int rt_link_spans(rt_linktable *tab, const rt_packet_fields *fields, const uint64_t *pkt_off, uint32_t n,
                  uint32_t n_keys, uint64_t *tok_off, uint32_t *tok_len, uint32_t *key_idx, int32_t *link,
                  uint8_t *route, void *stream) {
    RT_TRY(check_table(tab));
    if (n == 0) return RT_OK;
    if (!fields || !pkt_off || !tok_off || !tok_len || !key_idx || !link || !route)
        return fail(RT_E_INVAL, "rt_link_spans: null buffer");
    hipStream_t s = as_stream(stream);
    const LinkSpanArgs a{(const uint8_t *)fields, pkt_off, tab->t, n_keys, tok_off, tok_len, key_idx, link, route, n};
    return table_call(tab, s, "link table ordering", [&] {
        RT_HIP(launch_link_spans(a, s), "link spans");
        return RT_OK;
    });
}

}  // extern "C"

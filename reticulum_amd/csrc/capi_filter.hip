// capi_filter.hip — the packet hash list of the C-ABI and Transport's packet
// filter over it.  Device pointers on the caller's stream; the *_host calls go
// through a staging lane (capi_internal.h).  The kernels are in
// filter_kernels.hip; capacity rounding and the batch limit are the link
// table's (link_host.h), and so is the ordering of the calls (capi_table.h).
#include "capi_table.h"

namespace {

int check_list(const rt_hashlist *list) {
    if (!list || !list->ctx || !list->l.st) return fail(RT_E_INVAL, "null hash list");
    return RT_OK;
}

int add_on(rt_hashlist *list, const uint8_t *hashes, uint32_t n, hipStream_t s) {
    return table_call(list, s, "hash list ordering", [&] {
        int32_t *scratch = nullptr;
        RT_HIP(rec_alloc(list->ctx, 4ull * n, (uint32_t **)&scratch, s), "hash list scratch");
        const hipError_t e = launch_hashlist_add(list->l, hashes, scratch, n, s);
        const hipError_t f = hipFreeAsync(scratch, s);
        RT_HIP(e, "hash list add");
        RT_HIP(f, "hash list scratch");
        return RT_OK;
    });
}
int remove_on(rt_hashlist *list, const uint8_t *hashes, int32_t *status, uint32_t n, hipStream_t s) {
    return table_call(list, s, "hash list ordering", [&] {
        RT_HIP(launch_hashlist_remove(list->l, hashes, status, n, s), "hash list remove");
        return RT_OK;
    });
}
int contains_on(rt_hashlist *list, const uint8_t *hashes, uint8_t *found_out, uint32_t n, hipStream_t s) {
    return table_call(list, s, "hash list ordering", [&] {
        RT_HIP(launch_hashlist_contains(list->l, hashes, found_out, n, s), "hash list contains");
        return RT_OK;
    });
}

}  // namespace

extern "C" {

rt_hashlist *rt_hashlist_create(rt_ctx *c, uint32_t max_hashes) {
    if (!c) {
        fail(RT_E_INVAL, "null context");
        return nullptr;
    }
    const uint32_t cap = link_capacity(max_hashes);
    if (cap == 0) {
        fail(RT_E_INVAL, "rt_hashlist_create: max_hashes must be 1 .. 2^29");
        return nullptr;
    }
    hipSetDevice(c->device);
    rt_hashlist *list = new rt_hashlist();
    list->ctx = c;
    // two generations of slot words, their hashes, the state
    uint8_t *base = table_alloc(list, "hash list", 16ull * cap, 80ull * cap, sizeof(HashListState));
    if (!base) return nullptr;
    list->l = HashList{{(uint64_t *)base, (uint64_t *)(base + 8ull * cap)},
                       {base + 16ull * cap, base + 48ull * cap},
                       (HashListState *)(base + 80ull * cap), cap, max_hashes};
    return list;
}

void rt_hashlist_destroy(rt_hashlist *list) {
    if (list) table_free(list, list->l.slots[0]);
}

uint32_t rt_hashlist_capacity(const rt_hashlist *list) { return list ? list->l.cap : 0; }

int rt_packet_filter(rt_hashlist *list, rt_linktable *transit, const uint8_t *transport_identity,
                     rt_packet_fields *fields, uint32_t n, int32_t *status, void *stream) {
    RT_TRY(check_list(list));
    RT_TRY(check_batch(n, "rt_packet_filter"));
    if (transit && (!transit->t.slots || transit->ctx != list->ctx))
        return fail(RT_E_INVAL, "rt_packet_filter: the transit table is not one of the list's context");
    if (n == 0) return RT_OK;
    if (!transport_identity || !fields || !status) return fail(RT_E_INVAL, "rt_packet_filter: null buffer");
    hipStream_t s = as_stream(stream);
    FilterArgs a{list->l, LinkTab{}, transport_identity, (uint8_t *)fields, status, n};
    const auto launch = [&] {
        RT_HIP(launch_packet_filter(a, s), "packet filter");
        return RT_OK;
    };
    return table_call(list, s, "hash list ordering", [&] {
        if (!transit) return launch();
        // the transit table is read like any lookup on it: in host order with its inserts and removes
        return table_call(transit, s, "link table ordering", [&] {
            a.transit = transit->t;
            return launch();
        });
    });
}

int rt_hashlist_cull(rt_hashlist *list, void *stream) {
    RT_TRY(check_list(list));
    hipStream_t s = as_stream(stream);
    return table_call(list, s, "hash list ordering", [&] {
        RT_HIP(launch_hashlist_cull(list->l, s), "hash list cull");
        return RT_OK;
    });
}

int rt_hashlist_add(rt_hashlist *list, const uint8_t *hashes, uint32_t n, void *stream) {
    RT_TRY(check_list(list));
    RT_TRY(check_batch(n, "rt_hashlist_add"));
    if (n == 0) return RT_OK;
    if (!hashes) return fail(RT_E_INVAL, "rt_hashlist_add: null buffer");
    return add_on(list, hashes, n, as_stream(stream));
}

int rt_hashlist_remove(rt_hashlist *list, const uint8_t *hashes, uint32_t n, int32_t *status, void *stream) {
    RT_TRY(check_list(list));
    RT_TRY(check_batch(n, "rt_hashlist_remove"));
    if (n == 0) return RT_OK;
    if (!hashes || !status) return fail(RT_E_INVAL, "rt_hashlist_remove: null buffer");
    return remove_on(list, hashes, status, n, as_stream(stream));
}

int rt_hashlist_contains(rt_hashlist *list, const uint8_t *hashes, uint32_t n, uint8_t *found_out, void *stream) {
    RT_TRY(check_list(list));
    RT_TRY(check_batch(n, "rt_hashlist_contains"));
    if (n == 0) return RT_OK;
    if (!hashes || !found_out) return fail(RT_E_INVAL, "rt_hashlist_contains: null buffer");
    return contains_on(list, hashes, found_out, n, as_stream(stream));
}

int rt_hashlist_counts(rt_hashlist *list, uint32_t *out, void *stream) {
    RT_TRY(check_list(list));
    if (!out) return fail(RT_E_INVAL, "rt_hashlist_counts: null out");
    hipStream_t s = as_stream(stream);
    return table_call(list, s, "hash list ordering", [&] {
        RT_HIP(launch_hashlist_counts(list->l, out, s), "hash list counts");
        return RT_OK;
    });
}

int rt_hashlist_add_host(rt_hashlist *list, const uint8_t *hashes, uint32_t n) {
    RT_TRY(check_list(list));
    RT_TRY(check_batch(n, "rt_hashlist_add_host"));
    if (n == 0) return RT_OK;
    if (!hashes) return fail(RT_E_INVAL, "rt_hashlist_add_host: null buffer");
    HostCall hc(list->ctx, HostCall::PER_ARRAY);
    const uint64_t o_h = hc.add(32ull * n);
    RT_TRY(hc.open());
    hc.put(o_h, hashes, 32ull * n, "H2D hashes");
    RT_TRY(hc.send());
    RT_TRY(add_on(list, hc.dev<uint8_t>(o_h), n, hc.stream()));
    return hc.finish();
}

int rt_hashlist_remove_host(rt_hashlist *list, const uint8_t *hashes, uint32_t n, int32_t *status) {
    RT_TRY(check_list(list));
    RT_TRY(check_batch(n, "rt_hashlist_remove_host"));
    if (n == 0) return RT_OK;
    if (!hashes || !status) return fail(RT_E_INVAL, "rt_hashlist_remove_host: null buffer");
    HostCall hc(list->ctx, HostCall::PER_ARRAY);
    const uint64_t o_h = hc.add(32ull * n), o_st = hc.add(4ull * n);
    RT_TRY(hc.open());
    hc.put(o_h, hashes, 32ull * n, "H2D hashes");
    RT_TRY(hc.send());
    RT_TRY(remove_on(list, hc.dev<uint8_t>(o_h), hc.dev<int32_t>(o_st), n, hc.stream()));
    hc.get(status, o_st, 4ull * n, "D2H status");
    return hc.finish();
}

int rt_hashlist_contains_host(rt_hashlist *list, const uint8_t *hashes, uint32_t n, uint8_t *found_out) {
    RT_TRY(check_list(list));
    RT_TRY(check_batch(n, "rt_hashlist_contains_host"));
    if (n == 0) return RT_OK;
    if (!hashes || !found_out) return fail(RT_E_INVAL, "rt_hashlist_contains_host: null buffer");
    HostCall hc(list->ctx, HostCall::PER_ARRAY);
    const uint64_t o_h = hc.add(32ull * n), o_found = hc.add(n);
    RT_TRY(hc.open());
    hc.put(o_h, hashes, 32ull * n, "H2D hashes");
    RT_TRY(hc.send());
    RT_TRY(contains_on(list, hc.dev<uint8_t>(o_h), hc.dev<uint8_t>(o_found), n, hc.stream()));
    hc.get(found_out, o_found, n, "D2H found");
    return hc.finish();
}

}  // extern "C"

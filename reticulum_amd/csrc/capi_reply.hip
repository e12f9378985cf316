// capi_reply.hip — the send side of a read in the C-ABI (reply_kernels.hip):
// the replies gathered, the framing that takes its packet count from the
// device, and the hashes of what was sent entered into the packet hash list.
// Device pointers on the caller's stream; nothing is read back.
#include "capi_table.h"
#include "reply_host.h"

extern "C" {

uint64_t rt_reply_gather_workspace_bytes(uint32_t n, uint32_t n_sources) {
    if (n > RG_MAX_FRAMES) return 0;
    return reply_gather_workspace_bytes(n, n_sources);
}

int rt_reply_gather(rt_ctx *c, uint32_t n_sources, const uint8_t *const *rows, const uint64_t *row_stride,
                    const uint32_t *row_width, const int32_t *const *len, uint32_t n, uint8_t *out, int32_t *reply_len,
                    int32_t *reply_frame, uint8_t *reply_source, int64_t *reply_counts, uint32_t cap, void *workspace,
                    void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (!reply_sources_ok(n_sources)) return fail(RT_E_INVAL, "rt_reply_gather: 1 to 4 sources");
    if (n > RG_MAX_FRAMES) return fail(RT_E_INVAL, "rt_reply_gather: at most 2^31 - 1 frames per call");
    if (!rows || !row_stride || !row_width || !len) return fail(RT_E_INVAL, "rt_reply_gather: null source arrays");
    if (!reply_counts || !workspace) return fail(RT_E_INVAL, "rt_reply_gather: null reply_counts/workspace");
    if (cap && (!out || !reply_len || !reply_frame || !reply_source))
        return fail(RT_E_INVAL, "rt_reply_gather: null output");
    if ((uintptr_t)out & (RG_ROW - 1)) return fail(RT_E_INVAL, "rt_reply_gather: out is 128-byte aligned");
    if ((uintptr_t)workspace & 7u) return fail(RT_E_INVAL, "rt_reply_gather: workspace is 8-byte aligned");
    ReplyGatherArgs a{};
    for (uint32_t s = 0; s < n_sources; ++s) {
        if (n && (!rows[s] || !len[s])) return fail(RT_E_INVAL, "rt_reply_gather: null source");
        if (row_width[s] == 0 || row_stride[s] < row_width[s])
            return fail(RT_E_INVAL, "rt_reply_gather: a row holds 1 .. row_stride bytes");
        a.rows[s] = rows[s]; a.stride[s] = row_stride[s]; a.width[s] = row_width[s]; a.len[s] = len[s];
    }
    a.n_sources = n_sources; a.n = n; a.out = out; a.reply_len = reply_len; a.reply_frame = reply_frame;
    a.reply_source = reply_source; a.reply_counts = reply_counts; a.cap = cap; a.part = (uint64_t *)workspace;
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    RT_HIP(launch_reply_gather(a, as_stream(stream)), "reply gather");
    return RT_OK;
}

int rt_hdlc_frame_counted(rt_ctx *c, const uint8_t *pkt, const uint64_t *pkt_off, const uint32_t *pkt_len, uint32_t n,
                          const int64_t *n_dev, uint8_t *out, uint64_t *frame_off, void *workspace, void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (!frame_off) return fail(RT_E_INVAL, "rt_hdlc_frame_counted: null frame_off");
    if (n && (!pkt || !pkt_off || !pkt_len || !n_dev || !out || !workspace))
        return fail(RT_E_INVAL, "rt_hdlc_frame_counted: null buffer");
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    RT_HIP(launch_hdlc_frame_counted(pkt, pkt_off, pkt_len, n, n_dev, out, frame_off, workspace, as_stream(stream)),
           "hdlc frame counted");
    return RT_OK;
}

int rt_reply_remember(rt_hashlist *list, const uint8_t *rows, uint64_t row_stride, const int32_t *reply_len,
                      const int64_t *reply_counts, uint32_t cap, void *stream) {
    if (!list || !list->ctx || !list->l.st) return fail(RT_E_INVAL, "null hash list");
    RT_TRY(check_batch(cap, "rt_reply_remember"));
    if (cap == 0) return RT_OK;
    if (!rows || !reply_len || !reply_counts) return fail(RT_E_INVAL, "rt_reply_remember: null buffer");
    if (row_stride < RG_ROW) return fail(RT_E_INVAL, "rt_reply_remember: rows of at least 128 bytes");
    hipStream_t s = as_stream(stream);
    return table_call(list, s, "hash list ordering", [&] {
        // the hashes (32 B each), the add's scratch (a word each) and which rows are replies (a byte each)
        uint8_t *hashes = nullptr;
        RT_HIP(rec_alloc(list->ctx, 37ull * cap + 3, (uint32_t **)&hashes, s), "reply hash scratch");
        uint8_t *mask = hashes + 36ull * cap;
        hipError_t e = launch_reply_hashes(rows, row_stride, reply_len, reply_counts, cap, hashes, mask, s);
        if (e == hipSuccess) e = launch_hashlist_add(list->l, hashes, (int32_t *)(hashes + 32ull * cap), cap, s, mask);
        const hipError_t f = hipFreeAsync(hashes, s);
        RT_HIP(e, "reply remember");
        RT_HIP(f, "reply hash scratch");
        return RT_OK;
    });
}

}  // extern "C"

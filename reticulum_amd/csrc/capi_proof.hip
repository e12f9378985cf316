// capi_proof.hip — packet proofs on a link in the C-ABI (proof_kernels.hip):
// proving what a link received and settling the proofs that come back against
// a receipt table.  Device pointers on the caller's stream; nothing is read
// back.  The receipts are an rt_linktable, so the calls that read or change it
// take their place in that table's host order (capi_table.h).
#include "capi_table.h"

namespace {

int check_receipts(const rt_linktable *tab) {
    if (!tab || !tab->ctx || !tab->t.slots) return fail(RT_E_INVAL, "null receipt table");
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_link_prove(rt_ctx *c, const rt_packet_fields *fields, const uint8_t *route, const int32_t *link,
                  const int32_t *token_status, const uint8_t *seeds, const uint8_t *publics, uint64_t key_stride,
                  const uint8_t *flags, uint32_t n_links, uint8_t *proofs, uint64_t proof_stride, uint32_t *proof_len,
                  uint32_t n, void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (n == 0) return RT_OK;
    if (!fields || !route || !link || !token_status || !proofs || !proof_len)
        return fail(RT_E_INVAL, "rt_link_prove: null fields, route, link, token_status, proofs or proof_len");
    if (n_links && (!seeds || !publics || !flags)) return fail(RT_E_INVAL, "rt_link_prove: null seeds, publics or flags");
    if (key_stride != 0 && key_stride < 32) return fail(RT_E_INVAL, "rt_link_prove: key_stride is 0 or at least 32");
    if (proof_stride < 115) return fail(RT_E_INVAL, "rt_link_prove: proof_stride is at least 115");
    hipStream_t s = as_stream(stream);
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    // the candidate count and list: a stream-ordered temporary of the context's pool
    uint32_t *work = nullptr;
    RT_HIP(rec_alloc(c, prove_workspace_bytes(n), &work, s), "proof workspace");
    const ProveArgs a{(const uint8_t *)fields, route, link, token_status, seeds, publics, key_stride, flags, n_links,
                      proofs, proof_stride, proof_len, work, n};
    const hipError_t e = launch_link_prove(a, s);
    const hipError_t f = hipFreeAsync(work, s);
    RT_HIP(e, "link prove");
    RT_HIP(f, "proof workspace");
    return RT_OK;
}

int rt_receipt_store(rt_linktable *receipts, uint8_t *receipt_hashes, uint32_t max_receipts, const uint8_t *hashes,
                     const uint32_t *ids, const int32_t *status, uint32_t n, void *stream) {
    RT_TRY(check_receipts(receipts));
    if (n == 0) return RT_OK;
    if (!receipt_hashes || !hashes || !ids || !status) return fail(RT_E_INVAL, "rt_receipt_store: null buffer");
    hipStream_t s = as_stream(stream);
    return table_call(receipts, s, "receipt table ordering", [&] {
        RT_HIP(launch_receipt_store(receipt_hashes, max_receipts, hashes, ids, status, n, s), "receipt store");
        return RT_OK;
    });
}

int rt_proof_settle(rt_linktable *receipts, const uint8_t *receipt_hashes, uint32_t max_receipts, const uint8_t *pkt,
                    const uint64_t *pkt_off, const rt_packet_fields *fields, const int32_t *link,
                    const uint8_t *peer_publics, uint32_t n_links, int32_t *proof_status, int32_t *receipt, uint32_t n,
                    void *stream) {
    RT_TRY(check_receipts(receipts));
    if (n == 0) return RT_OK;
    if (n > LINK_MAX_BATCH) return fail(RT_E_INVAL, "rt_proof_settle: at most 2^30 - 2 items per call");
    if (!receipt_hashes || !pkt || !pkt_off || !fields || !link || !proof_status || !receipt)
        return fail(RT_E_INVAL, "rt_proof_settle: null buffer");
    if (n_links && !peer_publics) return fail(RT_E_INVAL, "rt_proof_settle: null peer_publics");
    rt_ctx *c = receipts->ctx;
    hipStream_t s = as_stream(stream);
    return table_call(receipts, s, "receipt table ordering", [&] {
        uint32_t *work = nullptr;
        RT_HIP(rec_alloc(c, settle_workspace_bytes(n), &work, s), "proof workspace");
        const SettleArgs a{receipts->t, receipt_hashes, max_receipts, pkt, pkt_off, (const uint8_t *)fields, link,
                           peer_publics, n_links, proof_status, receipt, work, n};
        const hipError_t e = launch_proof_settle(a, s);
        const hipError_t f = hipFreeAsync(work, s);
        RT_HIP(e, "proof settle");
        RT_HIP(f, "proof workspace");
        // every delivered receipt leaves the mark of a removal behind
        receipts->book.on_remove(n);
        return RT_OK;
    });
}

}  // extern "C"

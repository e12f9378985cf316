// capi_dproof.hip — proofs for packets sent to SINGLE destinations in the C-ABI
// (dproof_kernels.hip): the keyed receipts' store and the stage that settles
// the proofs of a read against them.  Device pointers on the caller's stream;
// nothing is read back.  The receipts are an rt_linktable, so the calls take
// their place in that table's host order (capi_table.h).
#include "capi_table.h"
#include "dproof_host.h"

namespace {

int check_keyed_receipts(const rt_linktable *tab) {
    if (!tab || !tab->ctx || !tab->t.slots) return fail(RT_E_INVAL, "null receipt table");
    return RT_OK;
}

}  // namespace

extern "C" {

uint64_t rt_destination_proof_workspace_bytes(uint32_t n, uint32_t max_receipts) {
    const uint32_t cap = link_capacity(max_receipts);
    if (n > DP_MAX_RECORDS || cap == 0) return 0;
    return dproof_workspace_bytes(n, cap, max_receipts);
}

int rt_receipt_store_keyed(rt_linktable *receipts, uint8_t *receipt_hashes, uint8_t *receipt_keys,
                           uint8_t *receipt_keyed, uint32_t max_receipts, const uint8_t *hashes, const uint8_t *keys,
                           const uint32_t *ids, const int32_t *status, uint32_t n, void *stream) {
    RT_TRY(check_keyed_receipts(receipts));
    if (n == 0) return RT_OK;
    if (!receipt_hashes || !receipt_keys || !receipt_keyed || !hashes || !ids || !status)
        return fail(RT_E_INVAL, "rt_receipt_store_keyed: null buffer");
    hipStream_t s = as_stream(stream);
    return table_call(receipts, s, "receipt table ordering", [&] {
        RT_HIP(launch_receipt_store_keyed(receipt_hashes, receipt_keys, receipt_keyed, max_receipts, hashes, keys, ids,
                                          status, n, s),
               "keyed receipt store");
        return RT_OK;
    });
}

int rt_destination_proof_settle(rt_linktable *receipts, const uint8_t *receipt_hashes, const uint8_t *receipt_keys,
                                const uint8_t *receipt_keyed, uint32_t max_receipts, uint32_t scan_trials, void *work,
                                uint64_t work_bytes, const uint8_t *pkt, const uint64_t *pkt_off,
                                const rt_packet_fields *fields, const int32_t *link, uint32_t n_links,
                                int32_t *dproof_status, int32_t *receipt, uint32_t n, void *stream) {
    RT_TRY(check_keyed_receipts(receipts));
    if (n == 0) return RT_OK;
    if (n > DP_MAX_RECORDS) return fail(RT_E_INVAL, "rt_destination_proof_settle: at most 2^30 - 2 records per call");
    if (scan_trials > DP_MAX_TRIALS) return fail(RT_E_INVAL, "rt_destination_proof_settle: scan_trials is at most 2^30 - 2");
    if (!receipt_hashes || !receipt_keys || !receipt_keyed || !pkt || !pkt_off || !fields || !dproof_status || !receipt)
        return fail(RT_E_INVAL, "rt_destination_proof_settle: null buffer");
    if (max_receipts == 0 || max_receipts > receipts->t.cap)
        return fail(RT_E_INVAL, "rt_destination_proof_settle: max_receipts is 1 .. the table's capacity");
    if (!work || ((uintptr_t)work & 15u) || work_bytes < dproof_workspace_bytes(n, receipts->t.cap, max_receipts))
        return fail(RT_E_INVAL, "rt_destination_proof_settle: work is 16-byte aligned memory of "
                                "rt_destination_proof_workspace_bytes(n, max_receipts)");
    hipStream_t s = as_stream(stream);
    return table_call(receipts, s, "receipt table ordering", [&] {
        const DproofArgs a{receipts->t, receipt_hashes, receipt_keys, receipt_keyed, max_receipts, pkt, pkt_off,
                           (const uint8_t *)fields, link, link ? n_links : 0u, scan_trials, dproof_status, receipt,
                           (uint32_t *)work, n};
        RT_HIP(launch_dproof_settle(a, s), "destination proof settle");
        // every delivered receipt leaves the mark of a removal behind
        receipts->book.on_remove(n);
        return RT_OK;
    });
}

}  // extern "C"

// capi_destination.hip — destination delivery in the C-ABI
// (destination_kernels.hip): the stage that opens and proves the DATA packets
// of a read that are addressed to the node's own SINGLE destinations.  Device
// pointers on the caller's stream; nothing is read back.  The stage reads the
// destinations' table, so it takes its place in that table's host order
// (capi_table.h), and it writes records of the scratch key set in stream order.
#include "capi_table.h"
#include "destination_host.h"

extern "C" {

uint64_t rt_destination_deliver_workspace_bytes(uint32_t max_frames, uint32_t retry_trials) {
    return deliver_workspace_bytes(max_frames, retry_trials);
}

int rt_destination_deliver(rt_linktable *dests, uint32_t n_dests, const uint8_t *privates,
                           const uint8_t *identity_hashes, const uint8_t *seeds, const uint8_t *publics,
                           const uint8_t *flags, const uint32_t *ratchet_off, const uint8_t *ratchets,
                           uint32_t n_ratchets, rt_keyset *scratch, uint32_t max_frames, uint32_t retry_trials,
                           void *work, uint64_t work_bytes, const uint8_t *pkt, const uint64_t *pkt_off,
                           const rt_packet_fields *fields, uint32_t n, int implicit_proof, uint32_t pt_shift,
                           uint8_t *pt, uint64_t *pt_off, uint32_t *pt_len, int32_t *status, int32_t *deliver_status,
                           int32_t *destination, int32_t *ratchet, uint8_t *proofs, uint64_t proof_stride,
                           uint32_t *proof_len, void *stream) {
    if (!dests || !dests->ctx || !dests->t.slots) return fail(RT_E_INVAL, "null destination table");
    RT_TRY(check_keyset(scratch));
    if (dests->ctx != scratch->ctx)
        return fail(RT_E_INVAL, "rt_destination_deliver: table and key set of one context");
    if (scratch->key_len != 64)
        return fail(RT_E_INVAL, "rt_destination_deliver: a destination's token key is 64 bytes (AES-256-CBC)");
    if (max_frames > DD_MAX_FRAMES || retry_trials > DD_MAX_FRAMES ||
        (uint64_t)max_frames + retry_trials > scratch->n_keys)
        return fail(RT_E_INVAL, "rt_destination_deliver: the scratch key set holds max_frames + retry_trials records");
    if (n > max_frames) return fail(RT_E_INVAL, "rt_destination_deliver: at most max_frames frames per call");
    if (n == 0) return RT_OK;
    if (!work || ((uintptr_t)work & 15) || work_bytes < deliver_workspace_bytes(max_frames, retry_trials))
        return fail(RT_E_INVAL, "rt_destination_deliver: a 16-byte aligned workspace of "
                                "rt_destination_deliver_workspace_bytes(max_frames, retry_trials)");
    if (!pkt || !pkt_off || !fields || !pt || !pt_off || !pt_len || !status || !deliver_status || !destination ||
        !ratchet || !proofs || !proof_len)
        return fail(RT_E_INVAL, "rt_destination_deliver: null buffer");
    if (n_dests && (!privates || !identity_hashes || !seeds || !publics || !flags || !ratchet_off))
        return fail(RT_E_INVAL, "rt_destination_deliver: null destination rows");
    if (n_ratchets && !ratchets) return fail(RT_E_INVAL, "rt_destination_deliver: null ratchets");
    if (((uintptr_t)identity_hashes & 3)) return fail(RT_E_INVAL, "rt_destination_deliver: identity_hashes on words");
    if (proof_stride < DD_PROOF_EXPLICIT) return fail(RT_E_INVAL, "rt_destination_deliver: proof_stride is at least 115");
    if (pt_shift > 16) return fail(RT_E_INVAL, "rt_destination_deliver: pt_shift is at most 16, the token's IV");
    rt_ctx *c = scratch->ctx;
    hipStream_t s = as_stream(stream);
    DeliverArgs a{};
    a.pkt = pkt; a.pkt_off = pkt_off; a.fields = (const uint8_t *)fields;
    a.dests = dests->t; a.n_dests = n_dests; a.privates = privates; a.id_hashes = identity_hashes;
    a.seeds = seeds; a.publics = publics; a.flags = flags; a.ratchet_off = ratchet_off; a.ratchets = ratchets;
    a.n_ratchets = n_ratchets;
    a.rec = scratch->d_rec; a.sbox = c->d_sbox; a.max_frames = max_frames; a.retry = retry_trials;
    a.implicit_proof = implicit_proof != 0; a.pt_shift = pt_shift;
    a.pt = pt; a.pt_off = pt_off; a.pt_len = pt_len; a.status = status;
    a.deliver_status = deliver_status; a.destination = destination; a.ratchet = ratchet;
    a.proofs = proofs; a.proof_stride = proof_stride; a.proof_len = proof_len;
    a.work = (uint32_t *)work; a.n = n;
    if (unsigned long long *w = c->clk.load(std::memory_order_acquire)) a.clk = w + 4 * RT_CLOCK_DECRYPT;
    return table_call(dests, s, "destination table ordering", [&] {
        a.dests = dests->t;
        // the candidates' keys are written into the scratch records on s: after
        // the key set's build, and recorded so that rt_keyset_destroy frees the
        // records after the stage
        RT_HIP(after_setup(scratch, s), "wait for key setup");
        const hipError_t e = launch_destination_deliver(a, c->n_cu, &c->queues, s);
        const hipError_t u = note_use(scratch, s);
        RT_HIP(e, "destination deliver");
        RT_HIP(u, "record key set use");
        return RT_OK;
    });
}

}  // extern "C"

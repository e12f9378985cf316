// capi_announce.hip — announce validation in the C-ABI (announce_kernels.hip).
// Device pointers on the caller's stream; nothing is read back.
#include "capi_internal.h"

extern "C" {

int rt_announce_validate(rt_ctx *c, const uint8_t *pkt, const uint64_t *pkt_off, const rt_packet_fields *fields,
                         uint32_t n, int32_t *status, uint8_t *identity_hash, void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (n == 0) return RT_OK;
    if (!pkt || !pkt_off || !fields || !status)
        return fail(RT_E_INVAL, "rt_announce_validate: null packets, offsets, fields or status");
    hipStream_t s = as_stream(stream);
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    // the candidate count and list: a stream-ordered temporary of the context's pool
    uint32_t *work = nullptr;
    RT_HIP(rec_alloc(c, announce_workspace_bytes(n), &work, s), "announce workspace");
    const AnnounceArgs a{pkt, pkt_off, (const uint8_t *)fields, status, identity_hash, work, n};
    const hipError_t e = launch_announce_validate(a, s);
    const hipError_t f = hipFreeAsync(work, s);
    RT_HIP(e, "announce validation");
    RT_HIP(f, "announce workspace");
    return RT_OK;
}

}  // extern "C"

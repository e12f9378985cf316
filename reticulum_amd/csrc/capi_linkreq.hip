// capi_linkreq.hip — link requests in the C-ABI (linkreq_kernels.hip): the
// stage that answers the LINKREQUEST packets of a read, and the call that
// rewrites chosen records of a key set from an exchange.  Device pointers on
// the caller's stream; nothing is read back.  The stage changes the link table
// and reads the destinations' table, so it takes its place in both tables' host
// order (capi_table.h), and it writes records of the key set in stream order.
#include "capi_table.h"

namespace {

int check_tab(const rt_linktable *tab, const char *what) {
    if (!tab || !tab->ctx || !tab->t.slots) return fail(RT_E_INVAL, std::string("null ") + what);
    return RT_OK;
}

// Records of k are written on s by `launch`: after the key set's build, and
// recorded so that rt_keyset_destroy frees the records after it.
template <class Launch>
int write_keys(rt_keyset *k, hipStream_t s, const char *what, Launch launch) {
    RT_HIP(after_setup(k, s), "wait for key setup");
    const hipError_t e = launch();
    const hipError_t u = note_use(k, s);
    RT_HIP(e, what);
    RT_HIP(u, "record key set use");
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_link_accept(rt_linktable *links, rt_keyset *ks, rt_linktable *dests, const uint8_t *dest_seeds,
                   const uint8_t *dest_publics, const uint8_t *dest_flags, uint32_t n_dests,
                   const uint8_t *transport_identity, int64_t nh_mtu, const uint8_t *pkt, const uint64_t *pkt_off,
                   const rt_packet_fields *fields, uint32_t n, const int32_t *slots, const uint8_t *ephemeral,
                   uint32_t m, uint32_t n_links, uint8_t *sg_seeds, uint8_t *sg_publics, uint64_t sg_stride,
                   uint8_t *sg_peer_publics, uint8_t *sg_flags, int32_t *status, int32_t *accepted, uint8_t *link_id,
                   int32_t *mtu, uint8_t *proofs, uint64_t proof_stride, uint32_t *proof_len, void *stream) {
    RT_TRY(check_tab(links, "link table"));
    RT_TRY(check_tab(dests, "destination table"));
    RT_TRY(check_keyset(ks));
    if (links == dests) return fail(RT_E_INVAL, "rt_link_accept: links and dests are two tables");
    if (links->ctx != ks->ctx || dests->ctx != ks->ctx)
        return fail(RT_E_INVAL, "rt_link_accept: tables and key set of one context");
    if (ks->key_len != 64) return fail(RT_E_INVAL, "rt_link_accept: a link's key is 64 bytes (AES-256-CBC)");
    RT_TRY(check_batch(n, "rt_link_accept"));
    if (n == 0) return RT_OK;
    if (!pkt || !pkt_off || !fields || !transport_identity || !status || !accepted || !link_id || !mtu || !proofs ||
        !proof_len)
        return fail(RT_E_INVAL, "rt_link_accept: null buffer");
    if (n_dests && (!dest_seeds || !dest_publics || !dest_flags))
        return fail(RT_E_INVAL, "rt_link_accept: null dest_seeds, dest_publics or dest_flags");
    if (m && (!slots || !ephemeral)) return fail(RT_E_INVAL, "rt_link_accept: null slots or ephemeral");
    if (proof_stride < 118) return fail(RT_E_INVAL, "rt_link_accept: proof_stride is at least 118");
    if (sg_peer_publics && !sg_flags) return fail(RT_E_INVAL, "rt_link_accept: sg_peer_publics without sg_flags");
    if (sg_peer_publics && sg_stride && (sg_stride < 32 || !sg_seeds || !sg_publics))
        return fail(RT_E_INVAL, "rt_link_accept: sg_stride is 0 or at least 32, with sg_seeds and sg_publics");
    if (nh_mtu > 0xFFFFFFFFll) return fail(RT_E_INVAL, "rt_link_accept: nh_mtu is a uint32, or negative for none");
    rt_ctx *c = ks->ctx;
    hipStream_t s = as_stream(stream);
    const uint32_t cap = n < m ? n : m;
    LinkReqArgs a{};
    a.pkt = pkt; a.pkt_off = pkt_off; a.fields = (const uint8_t *)fields; a.transport_id = transport_identity;
    a.dests = dests->t; a.dest_seeds = dest_seeds; a.dest_publics = dest_publics; a.dest_flags = dest_flags;
    a.n_dests = n_dests;
    a.has_nh_mtu = nh_mtu >= 0; a.nh_mtu = nh_mtu >= 0 ? (uint32_t)nh_mtu : 0u;
    a.links = links->t; a.slots = slots; a.ephemeral = ephemeral; a.m = m;
    a.n_keys = ks->n_keys; a.n_links = n_links; a.rec = ks->d_rec; a.sbox = c->d_sbox;
    a.sg_seeds = sg_seeds; a.sg_publics = sg_publics; a.sg_stride = sg_peer_publics ? sg_stride : 0;
    a.sg_peer = sg_peer_publics; a.sg_flags = sg_flags;
    a.status = status; a.accepted = accepted; a.link_id = link_id; a.mtu = mtu;
    a.proofs = proofs; a.proof_stride = proof_stride; a.proof_len = proof_len; a.n = n;
    return table_call(dests, s, "destination table ordering", [&] {
        return table_call(links, s, "link table ordering", [&] {
            // the host does not learn how many requests the read holds: the table's book counts the most
            // the call can insert, min(n, m), so a long free list brings the next rebuild forward
            RT_HIP(link_reclaim(links, cap, s), "link table rebuild");
            a.links = links->t;
            RT_HIP(rec_alloc(c, linkreq_workspace_bytes(n, m), &a.work, s), "link request workspace");
            const int rc = write_keys(ks, s, "link accept", [&] { return launch_link_accept(a, s); });
            const hipError_t f = hipFreeAsync(a.work, s);
            RT_TRY(rc);
            RT_HIP(f, "link request workspace");
            links->book.on_insert(cap);
            return RT_OK;
        });
    });
}

int rt_keyset_set_rows_x25519(rt_keyset *ks, const uint8_t *scalars, uint64_t scalar_stride, const uint8_t *points,
                              uint64_t point_stride, const uint64_t *point_off, const uint8_t *salt,
                              uint64_t salt_stride, uint32_t salt_len, const uint32_t *rows, const uint8_t *mask,
                              uint32_t n, void *stream) {
    RT_TRY(check_keyset(ks));
    if (ks->key_len != 64) return fail(RT_E_INVAL, "rt_keyset_set_rows_x25519: a key set of 64-byte keys");
    if (!scalars) return fail(RT_E_INVAL, "rt_keyset_set_rows_x25519: null scalars");
    if (point_off && !points) return fail(RT_E_INVAL, "rt_keyset_set_rows_x25519: point_off without points");
    if ((scalar_stride && scalar_stride < 32) || (points && !point_off && point_stride && point_stride < 32))
        return fail(RT_E_INVAL, "rt_keyset_set_rows_x25519: a stride is 0 (one row for all) or at least 32");
    if (n == 0) return RT_OK;
    if (!rows) return fail(RT_E_INVAL, "rt_keyset_set_rows_x25519: null rows");
    if (!salt || salt_len == 0 || salt_len > 64 || (salt_len & 3) || (salt_stride & 3) || salt_stride < salt_len ||
        ((uintptr_t)salt & 3))
        return fail(RT_E_INVAL, "rt_keyset_set_rows_x25519: one salt row per item, whole aligned words, at most 64 bytes");
    rt_ctx *c = ks->ctx;
    hipStream_t s = as_stream(stream);
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    // the shared secrets and the rows to write live in a stream-ordered
    // temporary: written by the exchange, read by the key setup, freed after it
    uint32_t *tmp = nullptr;
    RT_HIP(rec_alloc(c, 36ull * n, &tmp, s), "key rows workspace");
    uint8_t *d_shared = (uint8_t *)tmp;
    uint32_t *d_rows = tmp + 8ull * n;
    const int rc = write_keys(ks, s, "key rows", [&] {
        const X25519Args x{scalars, scalar_stride, points, point_stride, point_off, d_shared, 32, n};
        hipError_t e = launch_x25519(x, s);
        if (e == hipSuccess) e = launch_rows_select(rows, mask, ks->n_keys, d_rows, n, s);
        if (e != hipSuccess) return e;
        HkdfArgs h{};
        h.ikm = d_shared; h.ikm_stride = 32; h.ikm_len = 32;
        h.salt = salt; h.salt_stride = salt_stride; h.salt_len = salt_len;
        h.length = 64; h.n = n;
        return launch_hkdf_key_setup_rows(h, c->d_sbox, ks->d_rec, d_rows, nullptr, s);
    });
    const hipError_t f = hipFreeAsync(tmp, s);
    RT_TRY(rc);
    RT_HIP(f, "key rows workspace");
    return RT_OK;
}

}  // extern "C"

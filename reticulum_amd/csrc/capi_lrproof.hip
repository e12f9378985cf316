// capi_lrproof.hip — link request proofs in the C-ABI (lrproof_kernels.hip):
// the stage that validates the LRPROOF packets of a read against the node's
// pending links.  Device pointers on the caller's stream; nothing is read back.
// The stage reads the pending table (and borrows its slot words while it runs),
// changes the link table and, where there is one, the packet hash list, so it
// takes its place in the host order of all three (capi_table.h), and it writes
// records of the key set in stream order.
#include "capi_table.h"

namespace {

int check_tab(const rt_linktable *tab, const char *what) {
    if (!tab || !tab->ctx || !tab->t.slots) return fail(RT_E_INVAL, std::string("null ") + what);
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_link_establish(rt_linktable *pending, uint32_t n_rows, const uint8_t *row_privates,
                      const uint8_t *row_dest_publics, const uint8_t *row_sig_seeds, const uint8_t *row_sig_publics,
                      const uint8_t *row_flags, const int32_t *row_slots, int32_t *row_hops, uint8_t *row_rebalanced,
                      uint8_t *row_state, int32_t *row_mtu, rt_linktable *links, rt_keyset *ks, uint32_t n_links,
                      const uint8_t *pkt, const uint64_t *pkt_off, const rt_packet_fields *fields, uint32_t n,
                      uint8_t *sg_seeds, uint8_t *sg_publics, uint64_t sg_stride, uint8_t *sg_peer_publics,
                      uint8_t *sg_flags, rt_hashlist *seen, int32_t *status, int32_t *established, int32_t *mtu,
                      void *stream) {
    RT_TRY(check_tab(pending, "pending table"));
    RT_TRY(check_tab(links, "link table"));
    RT_TRY(check_keyset(ks));
    if (links == pending) return fail(RT_E_INVAL, "rt_link_establish: pending and links are two tables");
    if (links->ctx != ks->ctx || pending->ctx != ks->ctx)
        return fail(RT_E_INVAL, "rt_link_establish: tables and key set of one context");
    if (seen && (!seen->l.st || seen->ctx != ks->ctx))
        return fail(RT_E_INVAL, "rt_link_establish: the hash list is not one of the key set's context");
    if (ks->key_len != 64) return fail(RT_E_INVAL, "rt_link_establish: a link's key is 64 bytes (AES-256-CBC)");
    RT_TRY(check_batch(n, "rt_link_establish"));
    if (n == 0) return RT_OK;
    if (!pkt || !pkt_off || !fields || !status || !established || !mtu)
        return fail(RT_E_INVAL, "rt_link_establish: null buffer");
    if (n_rows && (!row_privates || !row_dest_publics || !row_sig_seeds || !row_sig_publics || !row_flags ||
                   !row_slots || !row_hops || !row_rebalanced || !row_state || !row_mtu))
        return fail(RT_E_INVAL, "rt_link_establish: null row array");
    if (sg_peer_publics && !sg_flags) return fail(RT_E_INVAL, "rt_link_establish: sg_peer_publics without sg_flags");
    if (sg_peer_publics && sg_stride && (sg_stride < 32 || !sg_seeds || !sg_publics))
        return fail(RT_E_INVAL, "rt_link_establish: sg_stride is 0 or at least 32, with sg_seeds and sg_publics");
    rt_ctx *c = ks->ctx;
    hipStream_t s = as_stream(stream);
    const uint32_t cap = n < n_rows ? n : n_rows;
    LrProofArgs a{};
    a.pkt = pkt; a.pkt_off = pkt_off; a.fields = (const uint8_t *)fields;
    a.n_rows = n_rows;
    a.row_privates = row_privates; a.row_dest_publics = row_dest_publics; a.row_sig_seeds = row_sig_seeds;
    a.row_sig_publics = row_sig_publics; a.row_flags = row_flags; a.row_slots = row_slots; a.row_hops = row_hops;
    a.row_rebalanced = row_rebalanced; a.row_state = row_state; a.row_mtu = row_mtu;
    a.n_keys = ks->n_keys; a.n_links = n_links; a.rec = ks->d_rec; a.sbox = c->d_sbox;
    a.sg_seeds = sg_seeds; a.sg_publics = sg_publics; a.sg_stride = sg_peer_publics ? sg_stride : 0;
    a.sg_peer = sg_peer_publics; a.sg_flags = sg_flags;
    a.status = status; a.established = established; a.mtu = mtu; a.n = n;
    const auto run = [&] {
        return table_call(pending, s, "pending table ordering", [&] {
            return table_call(links, s, "link table ordering", [&] {
                // the host does not learn how many links come up: the table's book counts the most the call can
                // insert, as rt_link_accept's does
                RT_HIP(link_reclaim(links, cap, s), "link table rebuild");
                a.pending = pending->t;
                a.links = links->t;
                // behind the stage's own workspace: the hashes the list is to learn (32 B and a flag per record)
                // and the scratch of the add
                const uint64_t at = (lrproof_workspace_bytes(n, n_rows) + 15) & ~15ull;
                RT_HIP(rec_alloc(c, at + (seen ? 37ull * n + 3 : 0), &a.work, s), "link proof workspace");
                if (seen) {
                    a.hashes = (uint8_t *)a.work + at;
                    a.remember = a.hashes + 36ull * n;
                }
                RT_HIP(after_setup(ks, s), "wait for key setup");
                hipError_t e = launch_link_establish(a, s);
                const hipError_t u = note_use(ks, s);
                if (e == hipSuccess && seen)
                    e = launch_hashlist_add(seen->l, a.hashes, (int32_t *)(a.hashes + 32ull * n), n, s, a.remember);
                const hipError_t f = hipFreeAsync(a.work, s);
                RT_HIP(e, "link establish");
                RT_HIP(u, "record key set use");
                RT_HIP(f, "link proof workspace");
                links->book.on_insert(cap);
                return RT_OK;
            });
        });
    };
    if (!seen) return run();
    return table_call(seen, s, "hash list ordering", run);
}

}  // extern "C"

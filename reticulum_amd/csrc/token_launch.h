// token_launch.h — internal interface between the C-ABI layer and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rnstok {

struct EncArgs {
    const uint32_t *rec;        // key records (REC_WORDS each)
    const uint8_t *sbox;        // 256 B S-box || 256 B inverse S-box (device)
    const uint8_t *pt;
    const uint64_t *pt_off;     // null -> i * pt_stride
    uint64_t pt_stride;
    const uint32_t *pt_len;     // null -> uni_len
    uint32_t uni_len;
    const uint32_t *key_idx;    // null -> key 0
    const uint8_t *iv;
    uint8_t *tok;
    const uint64_t *tok_off;    // null -> i * tok_stride
    uint64_t tok_stride;
    const uint32_t *order;      // null -> lane i handles packet i; else packet order[i]
    uint32_t *queue;            // null -> static grid stride; else a zeroed chunk counter (sorted batches)
    uint32_t n;
    uint32_t ilv;               // 1: unit-interleaved layout (16-B unit u of packet p at 16*(u*n + p)), uniform
    unsigned long long *clk;    // null, or this kernel class's 4 launch-clock words (rt_clock_stamps)
};

struct DecArgs {
    const uint32_t *rec;
    const uint8_t *sbox;
    const uint8_t *tok;
    const uint64_t *tok_off;
    uint64_t tok_stride;
    const uint32_t *tok_len;
    uint32_t uni_len;
    const uint32_t *key_idx;
    uint8_t *pt;
    const uint64_t *pt_off;
    uint64_t pt_stride;
    uint32_t *out_len;
    int32_t *status;
    const uint32_t *order;      // null -> lane i handles token i; else token order[i]
    uint32_t *queue;            // as EncArgs::queue
    uint32_t n;
    uint32_t ilv;               // as EncArgs::ilv (tokens and plaintexts), well-formed uniform tokens only
    unsigned long long *clk;    // as EncArgs::clk
};

// Ratchet trials (Identity.py:865-878): pairs j in [pair_off[t],
// pair_off[t+1]) try key pair_key[j] on token t; first[t] = the rank of the
// first pair whose HMAC verifies over a well-formed token, or 0xFFFFFFFF.
struct TrialArgs {
    const uint32_t *rec;
    const uint8_t *tok;
    const uint64_t *tok_off;
    const uint32_t *tok_len;
    const uint32_t *pair_off;   // n_tok + 1 entries, pair_off[0] = 0, pair_off[n_tok] = n_pairs
    const uint32_t *pair_key;
    uint32_t *first;
    uint32_t n_tok, n_pairs;
};
hipError_t launch_verify_trials(const TrialArgs &a, hipStream_t s);

// HKDF-SHA256 over n items (hkdf_kernels.hip): item i reads ikm + i*ikm_stride
// and salt + i*salt_stride (salt null or salt_len 0: zero key), shares the
// context, writes `length` bytes at out + i*out_stride.
struct HkdfArgs {
    const uint8_t *ikm;
    uint64_t ikm_stride;
    uint32_t ikm_len;
    const uint8_t *salt;
    uint64_t salt_stride;
    uint32_t salt_len;
    const uint8_t *context;
    uint32_t context_len;
    uint8_t *out;
    uint64_t out_stride;
    uint32_t length;
    uint32_t n;
};

// X25519 over n items (x25519_kernels.hip): out_i = X25519(scalar_i, point_i),
// scalar_i at scalars + i*scalar_stride, point_i at points + point_off[i]
// (point_off null: points + i*point_stride; points null: the base point 9),
// 32 bytes at out + i*out_stride.  Strides of 0 share one row.
struct X25519Args {
    const uint8_t *scalars;
    uint64_t scalar_stride;
    const uint8_t *points;
    uint64_t point_stride;
    const uint64_t *point_off;
    uint8_t *out;
    uint64_t out_stride;
    uint32_t n;
};
hipError_t launch_x25519(const X25519Args &a, hipStream_t s);

// Ed25519 over n items (ed25519_kernels.hip).  Item i's key is at pubs +
// i*pub_stride (32 bytes), its signature at sigs + i*sig_stride (64 bytes), its
// message at msgs + msg_off[i] (msg_len[i] bytes, any alignment; never read
// where msg_len[i] is 0).  Strides of 0 share one row.
struct Ed25519VerifyArgs {
    const uint8_t *pubs;
    uint64_t pub_stride;
    const uint8_t *sigs;
    uint64_t sig_stride;
    const uint8_t *msgs;
    const uint64_t *msg_off;
    const uint32_t *msg_len;
    uint8_t *ok;                   // 1 accepted, 0 rejected
    uint32_t n;
};
struct Ed25519SignArgs {
    const uint8_t *seeds;
    uint64_t seed_stride;
    const uint8_t *pubs;           // null: each lane derives its public key
    uint64_t pub_stride;
    const uint8_t *msgs;
    const uint64_t *msg_off;
    const uint32_t *msg_len;
    uint8_t *out;                  // 64 bytes at out + i*out_stride
    uint64_t out_stride;
    uint32_t n;
};
struct Ed25519PublicArgs {
    const uint8_t *seeds;
    uint64_t seed_stride;
    uint8_t *out;                  // 32 bytes at out + i*out_stride
    uint64_t out_stride;
    uint32_t n;
};
hipError_t launch_ed25519_verify(const Ed25519VerifyArgs &a, hipStream_t s);
hipError_t launch_ed25519_sign(const Ed25519SignArgs &a, hipStream_t s);
hipError_t launch_ed25519_public(const Ed25519PublicArgs &a, hipStream_t s);

// The interface access code (k_ifac_sign): item i's packet is pkt + pkt_off[i]
// (pkt_len[i] bytes, any alignment; an item of length 0 is skipped and its
// offset never used), signed with the batch's one seed and public key; the
// code is the last ifac_size (1..64) bytes of the signature.  status null:
// make, the code goes to ifac_out + i*ifac_size (zeros for a skipped item).
// status given: check, the code is compared with ifac_in + i*ifac_size where
// status[i] is 0, and a mismatch sets status[i] = IFAC_MISMATCH and
// pkt_len_io[i] (the same array as pkt_len) = 0.
constexpr int32_t IFAC_MISMATCH = 2;       // RT_IFAC_MISMATCH (include/rnstok.h)
struct IfacSignArgs {
    const uint8_t *seed;           // 32 bytes
    const uint8_t *pub;            // 32 bytes
    uint64_t key_stride;           // 0: one seed and one key for the batch (see k_ifac_sign)
    const uint8_t *pkt;
    const uint64_t *pkt_off;
    const uint32_t *pkt_len;
    uint32_t ifac_size;
    uint8_t *ifac_out;             // make
    const uint8_t *ifac_in;        // check
    int32_t *status;               // check, else null
    uint32_t *pkt_len_io;          // check: pkt_len, writable
    uint32_t n;
};
hipError_t launch_ifac_sign(const IfacSignArgs &a, hipStream_t s);

// Announce validation over rt_packet_unpack's records (announce_kernels.hip):
// status[i] = RT_ANNOUNCE_*; identity (n x 16, may be null) receives the
// announced identity's hash, zeros for a record that is no candidate.
// `work` is announce_workspace_bytes(n) of device memory the launch may use
// until it has run: the candidate count and the candidates' indices.
struct AnnounceArgs {
    const uint8_t *pkt;
    const uint64_t *pkt_off;
    const uint8_t *fields;         // n rt_packet_fields records
    int32_t *status;
    uint8_t *identity;
    uint32_t *work;
    uint32_t n;
};
uint64_t announce_workspace_bytes(uint32_t n);
hipError_t launch_announce_validate(const AnnounceArgs &a, hipStream_t s);

// Resource map hashes (resource_kernels.hip): part j = data + part_off[j]
// (part_len[j] bytes), or with part_off null the uniform segmentation
// data[j*sdu, min((j+1)*sdu, size)); salt = salts + part_res[j]*salt_len.
struct MapArgs {
    const uint8_t *data;
    const uint64_t *part_off;
    const uint32_t *part_len;
    uint64_t size;
    uint32_t sdu;
    const uint8_t *salts;
    uint32_t salt_len;
    const uint32_t *part_res;
    uint32_t n_res;
    uint32_t guard;
    uint8_t *out;                  // 4 bytes per part
    uint32_t *first_collision;     // n_res entries or null
    uint32_t n_parts;
};

// Resource integrity hash and proof (resource_kernels.hip): segment i =
// data + seg_off[i] (seg_len[i] bytes, any alignment, 0 allowed);
// hash[i] = SHA-256(segment || random_hashes[i]), proof[i] = SHA-256(segment
// || hash[i]).  With expect_hash (receiver) status[i] = 0 / 1 (hash differs:
// Resource.CORRUPT), the proof is over expect_hash[i] and zero where status is 1.
struct ResHashArgs {
    const uint8_t *data;
    const uint64_t *seg_off;
    const uint32_t *seg_len;
    const uint8_t *random_hashes;  // n x rh_len
    uint32_t rh_len;               // <= 32
    const uint8_t *expect_hash;    // n x 32 or null
    uint8_t *hash;                 // n x 32
    uint8_t *proof;                // n x 32 or null
    int32_t *status;               // n or null
    uint32_t n;
};
// Batches of fewer segments than this take k_resource_hashes_split (one
// workgroup per segment); measured, DESIGN.md 4.4.  A variant build may
// override it to time one kernel alone (tools/bench_resource_hash.py).
#ifndef RNSTOK_RESOURCE_SPLIT_BELOW
#define RNSTOK_RESOURCE_SPLIT_BELOW 1025u
#endif
constexpr uint32_t RES_HASH_SPLIT_BELOW = RNSTOK_RESOURCE_SPLIT_BELOW;
constexpr uint32_t RES_HASH_THREADS = 64;
uint32_t resource_hash_split_below();
hipError_t launch_resource_hashes(const ResHashArgs &a, hipStream_t s);

// Wire-side neighbours (wire_kernels.hip).
struct IfacArgs {
    const uint8_t *pkt;
    const uint64_t *pkt_off;
    const uint32_t *pkt_len;
    uint8_t *ifac;                 // mask: input (n x ifac_size); unmask: output
    uint32_t ifac_size;
    const uint8_t *ifac_key;
    uint32_t key_len;
    uint8_t *out;
    const uint64_t *out_off;
    int32_t *status;               // unmask only
    uint32_t *out_len;             // unmask only, may be null: unmasked length (0 where status != 0)
    uint32_t n;
};
struct PackArgs {
    const uint8_t *flags, *hops, *context;
    const uint8_t *destination_hash;   // 16 B per packet
    const uint8_t *transport_id;       // 16 B per packet or null (HEADER_1)
    uint8_t *out;
    const uint64_t *out_off;
    uint32_t n;
};
uint64_t hdlc_frame_workspace_bytes(uint32_t n);
uint64_t hdlc_deframe_workspace_bytes(uint64_t len);
hipError_t launch_hdlc_frame(const uint8_t *pkt, const uint64_t *off, const uint32_t *len, uint32_t n, uint8_t *out,
                             uint64_t *frame_off, void *ws, hipStream_t s);
// the same with the packet count on the device: entries at or past min(*n_dev, n) contribute no bytes
hipError_t launch_hdlc_frame_counted(const uint8_t *pkt, const uint64_t *off, const uint32_t *len, uint32_t n,
                                     const int64_t *n_dev, uint8_t *out, uint64_t *frame_off, void *ws,
                                     hipStream_t s);
// k_scan_parts alone: part[0..nb) scanned in place (exclusive), the sum at part[nb]
hipError_t launch_scan_parts(uint64_t *part, uint64_t nb, hipStream_t s);
hipError_t launch_hdlc_deframe(const uint8_t *buf, uint64_t len, uint32_t hw_mtu, uint32_t ifac_size, uint8_t *out,
                               uint64_t *frame_off, uint32_t *frame_len, int32_t *status, uint64_t *counts,
                               uint64_t max_pairs, void *ws, hipStream_t s, uint32_t line_phase = 0xFFFFFFFFu);
hipError_t launch_ifac(const IfacArgs &a, bool mask, hipStream_t s);
uint64_t frames_compact_workspace_bytes(uint64_t max_pairs);
hipError_t launch_frames_compact(const uint64_t *d_off, const uint32_t *d_len, const int32_t *st,
                                 const uint64_t *counts, uint64_t max_pairs, uint64_t *f_off, uint32_t *f_len,
                                 int64_t *frame_pair, int64_t *n_frames, void *ws, hipStream_t s);
hipError_t launch_token_spans(const void *fields, const uint64_t *pkt_off, uint32_t n, uint64_t *tok_off,
                              uint32_t *tok_len, hipStream_t s);
hipError_t launch_unpack(const uint8_t *pkt, const uint64_t *off, const uint32_t *len, void *fields, uint32_t n,
                         hipStream_t s);
hipError_t launch_pack_headers(const PackArgs &a, hipStream_t s);

// The send side of a read (reply_kernels.hip; sizes and grids in reply_host.h).
struct ReplyGatherArgs {
    const uint8_t *rows[4];        // source s: row k at rows[s] + k * stride[s]
    uint64_t stride[4];
    uint32_t width[4];             // bytes a row of source s holds (<= stride[s])
    const int32_t *len[4];         // 0, or outside 1 .. min(128, width[s]): nothing for that frame
    uint32_t n_sources;            // 1..4
    uint32_t n;                    // frames
    uint8_t *out;                  // cap x 128
    int32_t *reply_len, *reply_frame;
    uint8_t *reply_source;
    int64_t *reply_counts;         // [written, found]
    uint32_t cap;
    uint64_t *part;                // the workspace: reply_blocks(n) + 1 words
};
hipError_t launch_reply_gather(const ReplyGatherArgs &a, hipStream_t s);
// hashes[j] (32 B) = the packet hash of row j and mask[j] = 1 for j < min(counts[0], cap) whose length makes a
// packet; mask[j] = 0 for the others, whose hash is not written
hipError_t launch_reply_hashes(const uint8_t *rows, uint64_t stride, const int32_t *len, const int64_t *counts,
                               uint32_t cap, uint8_t *hashes, uint8_t *mask, hipStream_t s);

// Link table and dispatch (link_kernels.hip; the layout is described there).
struct LinkTab {
    uint64_t *slots;               // cap slot words
    uint8_t *ids;                  // cap x 16 B, entry s belongs to slot s
    uint32_t *values;              // cap
    uint32_t *live;                // one word: entries present
    uint32_t cap;                  // a power of two
};
struct LinkSpanArgs {
    const uint8_t *fields;         // n rt_packet_fields records
    const uint64_t *pkt_off;
    LinkTab t;
    uint32_t n_keys;               // values not below it are never a key index
    uint64_t *tok_off;
    uint32_t *tok_len, *key_idx;
    int32_t *link;
    uint8_t *route;
    uint32_t n;
};
hipError_t launch_link_lookup(const LinkTab &t, const uint8_t *ids, uint32_t *values_out, uint8_t *found_out,
                              uint32_t n, hipStream_t s);
// status doubles as the scratch between each call's two kernels
hipError_t launch_link_insert(const LinkTab &t, const uint8_t *ids, const uint32_t *values, int32_t *status,
                              uint32_t n, hipStream_t s);
hipError_t launch_link_remove(const LinkTab &t, const uint8_t *ids, int32_t *status, uint32_t n, hipStream_t s);
// Rebuild in place through `workspace` (device, link_rebuild_workspace_bytes);
// `report` (device address of mapped host memory, or null) receives
// ticket << 32 | live entries.
uint64_t link_rebuild_workspace_bytes(uint32_t cap);
hipError_t launch_link_rebuild(const LinkTab &t, void *workspace, uint64_t *report, uint32_t ticket, hipStream_t s);
hipError_t launch_link_spans(const LinkSpanArgs &a, hipStream_t s);

// Packet proofs on a link (proof_kernels.hip).  The signers' rows are indexed
// by the link table's value: seeds and publics 32 bytes each at l*key_stride
// (0: one row for every link), flags one byte each (1: the link proves every
// packet it could decrypt, 2: it has a channel), peer_publics 32 bytes each.
// `work` is prove_workspace_bytes(n) / settle_workspace_bytes(n) of device
// memory the launch may use until it has run.
struct ProveArgs {
    const uint8_t *fields;         // n rt_packet_fields records
    const uint8_t *route;
    const int32_t *link;
    const int32_t *status;         // the token status of the decrypt
    const uint8_t *seeds, *publics;
    uint64_t key_stride;
    const uint8_t *flags;
    uint32_t n_links;
    uint8_t *proofs;               // 115 bytes at proofs + i*proof_stride where proof_len[i] is 115
    uint64_t proof_stride;
    uint32_t *proof_len;
    uint32_t *work;
    uint32_t n;
};
struct SettleArgs {
    LinkTab t;                     // the receipts: hash[:16] -> id
    const uint8_t *hashes;         // max_receipts x 32 B, by id
    uint32_t max_receipts;
    const uint8_t *pkt;
    const uint64_t *pkt_off;
    const uint8_t *fields;
    const int32_t *link;
    const uint8_t *peer_publics;
    uint32_t n_links;
    int32_t *status, *receipt;
    uint32_t *work;
    uint32_t n;
};
uint64_t prove_workspace_bytes(uint32_t n);
uint64_t settle_workspace_bytes(uint32_t n);
hipError_t launch_link_prove(const ProveArgs &a, hipStream_t s);
hipError_t launch_proof_settle(const SettleArgs &a, hipStream_t s);
// store[ids[i]] = hashes[i] (32 bytes) where status[i] is RT_LINK_OK and ids[i] < max_receipts
hipError_t launch_receipt_store(uint8_t *store, uint32_t max_receipts, const uint8_t *hashes, const uint32_t *ids,
                                const int32_t *status, uint32_t n, hipStream_t s);

// Proofs for packets sent to SINGLE destinations (dproof_kernels.hip): the
// receipts as above, beside them the key each is verified under (keys, 32 B by
// id) and whether it has one (keyed, one byte by id).  `link` may be null: no
// link is active.  `work` is dproof_workspace_bytes(n, t.cap, max_receipts)
// (dproof_host.h) of 16-byte aligned device memory.
struct DproofArgs {
    LinkTab t;                     // the receipts: hash[:16] -> id
    const uint8_t *hashes;         // max_receipts x 32 B, by id
    const uint8_t *keys;           // max_receipts x 32 B, by id
    const uint8_t *keyed;          // max_receipts
    uint32_t max_receipts;
    const uint8_t *pkt;
    const uint64_t *pkt_off;
    const uint8_t *fields;
    const int32_t *link;
    uint32_t n_links;
    uint32_t scan_trials;
    int32_t *status, *receipt;
    uint32_t *work;
    uint32_t n;
};
hipError_t launch_dproof_settle(const DproofArgs &a, hipStream_t s);
// as launch_receipt_store, and key_store[ids[i]] = keys[i], keyed[ids[i]] = 1 (keys null: keyed 0)
hipError_t launch_receipt_store_keyed(uint8_t *store, uint8_t *key_store, uint8_t *keyed, uint32_t max_receipts,
                                      const uint8_t *hashes, const uint8_t *keys, const uint32_t *ids,
                                      const int32_t *status, uint32_t n, hipStream_t s);

// Link requests (linkreq_kernels.hip): the records rt_packet_unpack wrote, the
// node's destinations (a link table from destination hash to row, beside the
// rows' seeds, publics and flags), the link table and key records the accepted
// links go into, and the free list.  `work` is linkreq_workspace_bytes(n, m) of
// device memory the launch may use until it has run.
struct LinkReqArgs {
    const uint8_t *pkt;
    const uint64_t *pkt_off;
    const uint8_t *fields;         // n rt_packet_fields records
    const uint8_t *transport_id;   // 16 B
    LinkTab dests;                 // destination hash -> row
    const uint8_t *dest_seeds, *dest_publics;   // n_dests x 32 B each
    const uint8_t *dest_flags;     // n_dests: RT_DEST_ACCEPTS | RT_LINK_PROVE_ALL | RT_LINK_HAS_CHANNEL
    uint32_t n_dests;
    uint32_t has_nh_mtu, nh_mtu;
    LinkTab links;                 // link id -> slot
    const int32_t *slots;          // m free slots, request r in stream order takes slots[r]
    const uint8_t *ephemeral;      // m x 32 B, row r for request r
    uint32_t m;
    uint32_t n_keys, n_links;      // a slot is below both
    uint32_t *rec;                 // the key set's records
    const uint8_t *sbox;
    uint8_t *sg_seeds, *sg_publics;    // the signers' rows, or null: sg_stride 0 leaves the one shared row alone
    uint64_t sg_stride;
    uint8_t *sg_peer, *sg_flags;
    int32_t *status, *accepted;
    uint8_t *link_id;              // n x 16 B
    int32_t *mtu;
    uint8_t *proofs;               // 118 bytes at proofs + i*proof_stride where proof_len[i] is 118
    uint64_t proof_stride;
    uint32_t *proof_len;
    uint32_t *work;
    uint32_t n;
};
uint64_t linkreq_workspace_bytes(uint32_t n, uint32_t m);
hipError_t launch_link_accept(const LinkReqArgs &a, hipStream_t s);
// out[i] = rows[i] where mask[i] (null: every item) and rows[i] < n_keys, else 0xFFFFFFFF
hipError_t launch_rows_select(const uint32_t *rows, const uint8_t *mask, uint32_t n_keys, uint32_t *out, uint32_t n,
                              hipStream_t s);

// Link request proofs (lrproof_kernels.hip): the records rt_packet_unpack
// wrote, the pending links (a link table from link id to row, beside the rows'
// keys and state), and the link table, key records and signers' rows the
// activated links go into.  `work` is lrproof_workspace_bytes(n, n_rows) of
// device memory the launch may use until it has run; `remember` (n bytes, or
// null) and `hashes` (n x 32 B) receive which records' packet hashes the hash
// list is to learn, and the hashes of those.
struct LrProofArgs {
    const uint8_t *pkt;
    const uint64_t *pkt_off;
    const uint8_t *fields;         // n rt_packet_fields records
    LinkTab pending;               // link id -> row
    uint32_t n_rows;
    const uint8_t *row_privates, *row_dest_publics, *row_sig_seeds, *row_sig_publics;   // n_rows x 32 B each
    const uint8_t *row_flags;
    const int32_t *row_slots;
    int32_t *row_hops;
    uint8_t *row_rebalanced, *row_state;
    int32_t *row_mtu;
    LinkTab links;                 // link id -> slot
    uint32_t n_keys, n_links;      // a slot is below both
    uint32_t *rec;                 // the key set's records
    const uint8_t *sbox;
    uint8_t *sg_seeds, *sg_publics;
    uint64_t sg_stride;
    uint8_t *sg_peer, *sg_flags;
    int32_t *status, *established, *mtu;
    uint8_t *remember, *hashes;
    uint32_t *work;
    uint32_t n;
};
uint64_t lrproof_workspace_bytes(uint32_t n, uint32_t n_rows);
hipError_t launch_link_establish(const LrProofArgs &a, hipStream_t s);

// Destination delivery (destination_kernels.hip): the records rt_packet_unpack
// wrote, the node's SINGLE destinations (a link table from destination hash to
// row, beside the rows' keys, flags and ratchets), and the scratch key records
// the candidates' keys go into: rows 0 .. max_frames-1 for the first pass,
// max_frames .. max_frames+retry-1 for the second.  `work` is
// deliver_workspace_bytes(max_frames, retry) of device memory (destination_host.h)
// the launch may use until it has run.
struct DeliverArgs {
    const uint8_t *pkt;
    const uint64_t *pkt_off;
    const uint8_t *fields;         // n rt_packet_fields records
    LinkTab dests;                 // destination hash -> row
    uint32_t n_dests;
    const uint8_t *privates;       // n_dests x 32 B: the identities' X25519 private keys
    const uint8_t *id_hashes;      // n_dests x 16 B: the identities' hashes, the HKDF salt
    const uint8_t *seeds, *publics;    // n_dests x 32 B each: Ed25519
    const uint8_t *flags;          // n_dests: RT_LINK_PROVE_ALL | RT_DEST_ENFORCE_RATCHETS
    const uint32_t *ratchet_off;   // n_dests + 1
    const uint8_t *ratchets;       // total x 32 B, each destination's newest first
    uint32_t n_ratchets;           // rows `ratchets` holds: an offset past them is never followed
    uint32_t *rec;                 // the scratch key set's records
    const uint8_t *sbox;
    uint32_t max_frames, retry;
    uint32_t implicit_proof, pt_shift;
    uint8_t *pt;
    uint64_t *pt_off;
    uint32_t *pt_len;
    int32_t *status;               // the token status
    int32_t *deliver_status, *destination, *ratchet;
    uint8_t *proofs;               // 83 or 115 bytes at proofs + i*proof_stride where proof_len[i] says so
    uint64_t proof_stride;
    uint32_t *proof_len;
    uint32_t *work;
    uint32_t n;
    unsigned long long *clk;       // the decrypt's launch-clock words, or null
};
struct SpareQueue;                 // below: the decrypt's chunk counters
hipError_t launch_destination_deliver(const DeliverArgs &a, int n_cu, SpareQueue *spare, hipStream_t s);

// Packet hash list and packet filter (filter_kernels.hip; the layout is
// described there).  Two generations of slot words and 32-byte hashes; which
// of them is the current one is a word in device memory that every kernel reads.
struct HashListState {
    uint32_t sel;                  // the current generation, 0 or 1
    uint32_t count[2];             // entries present, by generation
    uint32_t overflow;             // packets passed but not remembered: the current generation was full
    uint32_t rotate;               // the latest cull's decision, for its clearing kernel
    uint32_t pad[3];
};
struct HashList {
    uint64_t *slots[2];            // cap slot words each
    uint8_t *hashes[2];            // cap x 32 B each, entry s belongs to slot s
    HashListState *st;
    uint32_t cap;                  // a power of two
    uint32_t max;                  // entries a generation holds at most
};
struct FilterArgs {
    HashList l;
    LinkTab transit;               // slots null: none
    const uint8_t *identity;       // 16 B
    uint8_t *fields;               // n rt_packet_fields records
    int32_t *status;
    uint32_t n;
    const uint8_t *mask;           // launch_hashlist_add only: items with mask[i] == 0 are left out; null: none is
};
// status doubles as the scratch between each call's kernels
hipError_t launch_packet_filter(const FilterArgs &a, hipStream_t s);
hipError_t launch_hashlist_add(const HashList &l, const uint8_t *hashes, int32_t *scratch, uint32_t n, hipStream_t s,
                               const uint8_t *mask = nullptr);
hipError_t launch_hashlist_remove(const HashList &l, const uint8_t *hashes, int32_t *status, uint32_t n,
                                  hipStream_t s);
hipError_t launch_hashlist_contains(const HashList &l, const uint8_t *hashes, uint8_t *found_out, uint32_t n,
                                    hipStream_t s);
hipError_t launch_hashlist_cull(const HashList &l, hipStream_t s);
hipError_t launch_hashlist_counts(const HashList &l, uint32_t *out, hipStream_t s);

hipError_t configure_kernels();

// bytes from device memory `src` to pinned host memory, as GPU stores into the
// mapped host buffer (dst_dev: its device-side address) on stream s
// (copy_kernels.hip; faster than the copy engine's D2H, see there).
// dev_bytes (device pointer, optional): copy min(bytes, *dev_bytes) bytes.
hipError_t launch_store_host(uint8_t *dst_dev, const uint8_t *src, uint64_t bytes, hipStream_t s,
                             const uint64_t *dev_bytes = nullptr);

// Length bucketing: order[] = packet indices grouped by descending AES quad
// count, so that the lanes of a wave carry similar lengths.  `dec` selects
// token lengths (quads of the ciphertext body) instead of plaintext lengths.
// *queue receives a zeroed chunk counter: the token kernels' waves then take
// the ordered packets 64 at a time, longest first (dynamic balance).
constexpr uint32_t SORT_BUCKETS = 4096;
uint64_t sort_workspace_bytes(uint32_t n);    // order[n] + 2 x SORT_BUCKETS counters
hipError_t launch_length_order(const uint32_t *len, uint32_t n, int dec, void *workspace, const uint32_t **order,
                               uint32_t **queue, int n_cu, hipStream_t s);
// Chunk counters for ragged uniform batches (the static stride would leave a
// ragged last pass).  acquire() hands out a 4-byte device counter (and its
// slot number) that no other launch can still be reading once work queued on
// `s` after this call runs (the C-ABI orders slot reuse with an event per
// slot), or null; release(s, slot) is called once after the launch that used
// it has been enqueued on `s`.  Thread-safe, no lock held in between.
struct SpareQueue {
    virtual uint32_t *acquire(hipStream_t s, uint32_t *slot) = 0;
    virtual void release(hipStream_t s, uint32_t slot) = 0;
    virtual ~SpareQueue() {}
};
// Which kernel a batch runs on (RT_KERNEL_*, include/rnstok.h): the routing
// launch_encrypt / launch_decrypt apply, exposed as rt_plan_uniform.
int plan_encrypt(uint32_t n, bool packed, uint32_t uni_len, bool per_key, int n_cu);
int plan_decrypt(uint32_t n, bool packed, uint32_t uni_len, bool per_key, int n_cu);
hipError_t launch_encrypt(const EncArgs &a, int nr, int n_cu, SpareQueue *spare, hipStream_t s);
hipError_t launch_decrypt(const DecArgs &a, int nr, int n_cu, SpareQueue *spare, hipStream_t s);
// Token.verify_hmac (Token.py:77-84) over n tokens: status[i] = 0 (tag
// valid), 1 (len <= 32) or 2 (tag mismatch); no AES, no plaintext.
struct VerifyArgs {
    const uint32_t *rec;
    const uint8_t *tok;
    const uint64_t *tok_off;    // null -> i * tok_stride
    uint64_t tok_stride;
    const uint32_t *tok_len;    // null -> uni_len
    uint32_t uni_len;
    const uint32_t *key_idx;    // null -> key 0
    int32_t *status;
    uint32_t n;
};
hipError_t launch_verify(const VerifyArgs &a, hipStream_t s);
hipError_t launch_map_hashes(const MapArgs &m, hipStream_t s);
hipError_t launch_hkdf(const HkdfArgs &a, hipStream_t s);
hipError_t launch_key_setup(const uint8_t *keys, uint32_t key_len, uint32_t n_keys, const uint8_t *sbox,
                            uint32_t *rec, hipStream_t s);
// HKDF (a.length = key_len, a.out unused) and key setup in one launch: key i
// of the records is Token(hkdf(key_len, ikm_i, salt_i, context)) and the
// derived key never reaches HBM.  Returns hipErrorNotSupported for shapes
// outside the fused kernel's (the caller then runs launch_hkdf +
// launch_key_setup through a temporary).
hipError_t launch_hkdf_key_setup(const HkdfArgs &a, const uint8_t *sbox, uint32_t *rec, int n_cu, hipStream_t s);
// The same into chosen records of an existing table of 64-byte keys: item i
// writes record rows[i], or nothing where rows[i] is 0xFFFFFFFF; rows of one
// launch are distinct.  count (device, may be null): only the first
// min(*count, a.n) items exist.  One salt row per item, the fused kernel's
// shape only (hipErrorNotSupported otherwise).
hipError_t launch_hkdf_key_setup_rows(const HkdfArgs &a, const uint8_t *sbox, uint32_t *rec, const uint32_t *rows,
                                      const uint32_t *count, hipStream_t s);

}  // namespace rnstok

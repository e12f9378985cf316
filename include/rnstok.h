/*
 * rnstok.h — C-ABI of the MI355X encrypted-token engine (librnstok.so).
 *
 * Drop-in boundary for Reticulum's per-packet token path.  The reference is
 * pure Python; the maintainer-side binding is a ctypes stub
 * behind the unchanged class surface of RNS/Cryptography/Token.py.  Each
 * entry point names the reference interface it replaces (markqvist/Reticulum
 * 1.4.2, paths relative to the repository root):
 *
 *   rt_keyset_create   Token.__init__            RNS/Cryptography/Token.py:58-74
 *                      (+ the per-call key schedule AES.py:83,100 and the
 *                       per-call HMAC key pad HMAC.py:73-82, hoisted per key)
 *   rt_encrypt*        Token.encrypt             RNS/Cryptography/Token.py:87-97
 *   rt_decrypt*        Token.verify_hmac+decrypt RNS/Cryptography/Token.py:77-84,100-114
 *   rt_verify*         Token.verify_hmac         RNS/Cryptography/Token.py:77-84 (no AES)
 *   rt_token_len       token size arithmetic     Token.py:50 (TOKEN_OVERHEAD) + PKCS7.py:35-39
 *   rt_hkdf*           RNS.Cryptography.hkdf     RNS/Cryptography/HKDF.py:35-62
 *   rt_map_hashes /    Resource hashmap          RNS/Resource.py:426-468 (map hashes + the
 *   rt_resource_hashmap_host                      collision guard), get_map_hash :505-506,
 *                                                receive_part :865-866
 *   rt_resource_hashes /  Resource hash + proof  RNS/Resource.py:436-439 (hash, expected_proof),
 *   rt_resource_hashes_host                       :698-699 (receiver's check), :759-760 (prove)
 *   rt_hdlc_frame     HDLC.escape + framing     RNS/Interfaces/TCPInterface.py:44-53, :323
 *   rt_hdlc_deframe    HDLC read loop            RNS/Interfaces/TCPInterface.py:387-410, :336-339
 *   rt_hdlc_deframe_slots  the same, each frame in a 128-B-aligned slot
 *   rt_ifac_mask       IFAC on transmit          RNS/Transport.py:1069-1101
 *   rt_ifac_unmask     IFAC on inbound           RNS/Transport.py:1441-1475
 *   rt_ifac_sign/check the IFAC's signature      RNS/Transport.py:1073, 1470-1474
 *   rt_packet_unpack   Packet.unpack + get_hash  RNS/Packet.py:236-268, 342-353
 *   rt_packet_pack_headers  Packet.pack header   RNS/Packet.py:167-228
 *   rt_frames_compact  frames a read hands on    RNS/Interfaces/TCPInterface.py:391-401
 *                      (one process_incoming call per frame, in stream order)
 *   rt_token_spans     packet.data (the token)   RNS/Packet.py:262-275 (data after the header)
 *   rt_linktable_* /   the link of a DATA packet  RNS/Transport.py:2161-2176 (first link in
 *   rt_link_spans      and whether it is decrypted  active_links with the link_id), RNS/Link.py:941-1148
 *   rt_hashlist_* /    packets seen before        RNS/Transport.py:1377-1427, 1525-1545, 656-658
 *   rt_packet_filter
 *   rt_announce_validate  validate_announce       RNS/Identity.py:505-606 (Transport.py:1748-1750, 1772)
 *   rt_link_prove      Packet.prove on a link     RNS/Link.py:943-955, 1140-1145 (whether), :378-389 and
 *                                                RNS/Packet.py:199-200 (the proof packet)
 *   rt_receipt_store / Transport.receipts and     RNS/Transport.py:2326-2363 (the receipt of a link proof),
 *   rt_proof_settle    validate_link_proof        RNS/Packet.py:434-459
 *   rt_link_accept     link requests answered      RNS/Transport.py:2127-2158, RNS/Destination.py:414-435,
 *                      (responder side)            RNS/Link.py:186-227, 336-376, RNS/Packet.py:170-185
 *   rt_keyset_set_rows_x25519  Link.handshake's key into a record of an existing key set  RNS/Link.py:348-361
 *   rt_link_establish  link request proofs        RNS/Transport.py:2270-2318, RNS/Link.py:391-451, 326-333,
 *                      validated (initiator side)  348-361
 *   rt_destination_deliver  packets for the node's  RNS/Transport.py:2188-2202, RNS/Destination.py:414-429,
 *                      SINGLE destinations         622-654, RNS/Identity.py:848-898, 942-953,
 *                      opened and proved           RNS/Packet.py:327-336, 376-381
 *   rt_receipt_store_keyed /  proofs for packets    RNS/Transport.py:2326-2363 (packet.link unset),
 *   rt_destination_proof_settle  sent to SINGLE    RNS/Packet.py:480-524 (validate_proof), 376-381
 *                      destinations, settled
 *   rt_reply_gather /  the replies of a read, sent  RNS/Identity.py:942-953, RNS/Link.py:366-389 (proofs go out
 *   rt_hdlc_frame_counted /  on the interface the   on the receiving interface), RNS/Transport.py:1069-1104
 *   rt_reply_remember  frames came in on            (transmit), 1199-1356 (outbound's broadcast), 1343-1345
 *   rt_keyset_create_hkdf  per-packet keying     Identity.py:837-846 (hkdf -> Token(derived_key)),
 *                                                Link.py handshake key derivation
 *   rt_x25519*         X25519 exchange / public key  RNS/Cryptography/X25519.py:49-93, 136-145
 *   rt_ed25519_*       Ed25519 verify / sign / public key  RNS/Cryptography/pure25519/eddsa.py,
 *                                                Identity.validate, Identity.sign, validate_announce
 *   rt_keyset_create_x25519  the same keying from the exchange on: Identity.py:812-829, 861-871
 *   rt_verify_trials*  ratchet trial loop       Identity.py:865-878 (first ratchet whose key
 *                                                opens the token; Token.py:77-84,114)
 *
 * Conventions
 *  - No exceptions cross the boundary.  API misuse returns a negative RT_E_*
 *    code and sets a thread-local message (rt_last_error).  Per-packet
 *    outcomes of decrypt are reported in an int32 status array (RT_ST_*),
 *    mirroring the reference's exception classes (Token.py:78,102,114;
 *    PKCS7.py:45-46): the Python layer maps non-zero status to ValueError.
 *  - The caller owns every buffer; the library never frees caller memory.
 *    rt_encrypt / rt_decrypt take DEVICE pointers and a hipStream_t (as
 *    void*; NULL = HIP's null stream, which is also torch's default stream)
 *    and only enqueue work.
 *    rt_*_host take HOST pointers, stage through the context's workspace and
 *    return after the results are back in host memory.
 *  - Token layout (Token.py:96-97): iv(16) || AES-CBC(ek, iv, PKCS7(pt)) ||
 *    HMAC-SHA256(sk, iv||ct)(32), so len(token) = 16 + 16*(L/16 + 1) + 32.
 *  - Key layout (Token.py:61-70): 64-byte keys -> sk = key[0:32],
 *    ek = key[32:64], AES-256-CBC; 32-byte keys -> sk = key[0:16],
 *    ek = key[16:32], AES-128-CBC.  One keyset holds keys of one length.
 *  - IVs are supplied by the caller (16 bytes per packet), drawn from
 *    os.urandom as in Token.py:89; the library never generates IVs.
 *  - Thread safety: a context may be used from several host threads.  Host
 *    staging calls run on one of the context's staging lanes (each its own
 *    stream, workspace and pinned buffer), so up to 4 run concurrently.
 *    Device calls are re-entrant given distinct output buffers, from any
 *    thread and on any streams.
 *  - Stream ordering of key sets: a key set is built on the stream it was
 *    created on (rt_keyset_create: a staging lane's stream), and every later
 *    launch that reads it, on any stream, first waits for that build.
 *    rt_keyset_destroy never blocks: the records are released once the last
 *    launch on every stream that used them has completed.
 */
#ifndef RNSTOK_H
#define RNSTOK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RNSTOK_ABI_VERSION 3   /* 2: rt_hdlc_deframe_slots, rt_clock_stamps; 3: rt_resource_hashes* */

/* Return codes (< 0: API misuse or runtime failure). */
#define RT_OK        0
#define RT_E_INVAL  -1   /* bad argument (NULL pointer, bad key length, ...) */
#define RT_E_HIP    -2   /* HIP runtime error (message in rt_last_error)     */
#define RT_E_NOMEM  -3   /* device or pinned allocation failed               */
#define RT_E_NODEV  -4   /* no usable gfx950 device                          */

/* Per-packet decrypt status. */
#define RT_ST_OK          0  /* plaintext written, pt_len set                    */
#define RT_ST_TOO_SHORT   1  /* len(token) <= 32            (Token.py:78)        */
#define RT_ST_BAD_HMAC    2  /* tag mismatch                (Token.py:102)       */
#define RT_ST_BAD_CT_LEN  3  /* valid tag, ct empty or %16  (Token.py:114 wrap)  */
#define RT_ST_BAD_PAD     4  /* valid tag, last byte > 16   (PKCS7.py:45-46)     */

typedef struct rt_ctx rt_ctx;
typedef struct rt_keyset rt_keyset;

/* ---- library / context --------------------------------------------------- */
int         rt_abi_version(void);
const char *rt_last_error(void);
int         rt_device_count(void);
/* One context per device.  Builds the S-box tables on the device. */
rt_ctx     *rt_create(int device);
void        rt_destroy(rt_ctx *ctx);
/* Number of compute units the context launches over (persistent grid). */
int         rt_num_cus(const rt_ctx *ctx);

/* ---- keys (Token.__init__, Token.py:58-74) ------------------------------- */
/* keys: HOST pointer, n_keys x key_len bytes, key_len 64 (AES-256) or 32
 * (AES-128).  Runs the key-setup kernel: AES encryption and equivalent
 * decryption schedules plus HMAC-SHA256 ipad/opad midstates per key. */
rt_keyset  *rt_keyset_create(rt_ctx *ctx, const uint8_t *keys, uint32_t key_len, uint32_t n_keys);
/* Same, with the raw keys already in DEVICE memory (on-device key tables). */
rt_keyset  *rt_keyset_create_device(rt_ctx *ctx, const uint8_t *d_keys, uint32_t key_len, uint32_t n_keys,
                                    void *stream);
void        rt_keyset_destroy(rt_keyset *ks);
uint32_t    rt_keyset_size(const rt_keyset *ks);

/* ---- sizes --------------------------------------------------------------- */
uint64_t    rt_token_len(uint64_t pt_len);      /* 16 + 16*(pt_len/16+1) + 32 */

/* ---- unit-interleaved device batches (no reference counterpart) ---------- */
/* For batches that are produced and consumed on the device (e.g. the
 * deframer's output feeding decrypt), a layout in which every wave load and
 * store instruction covers 1 KiB of contiguous HBM: 16-B unit u of packet p
 * at buf + 16*(u*n + p).  Plaintexts hold ceil(pt_len/16) units (the last
 * one partial: only its first pt_len % 16 bytes are read), tokens
 * rt_token_len(pt_len)/16 units (IV, ciphertext blocks, 2 tag units), the
 * decrypted plaintext (tok_len - 48)/16 units (pad block included, as
 * rt_decrypt_uniform).  iv: n x 16 B.  Outputs, statuses and error order are
 * those of rt_encrypt_uniform / rt_decrypt_uniform on the same packets;
 * decrypt takes well-formed token lengths only (48 + 16*k, k >= 1), others
 * are RT_E_INVAL.  Always the one-packet-per-lane kernels. */
int rt_encrypt_interleaved(const rt_keyset *ks, const uint8_t *pt, uint32_t pt_len, const uint32_t *key_idx,
                           const uint8_t *iv, uint8_t *tok, uint32_t n, void *stream);
int rt_decrypt_interleaved(const rt_keyset *ks, const uint8_t *tok, uint32_t tok_len, const uint32_t *key_idx,
                           uint8_t *pt, uint32_t *pt_len, int32_t *status, uint32_t n, void *stream);

/* ---- kernel plan (diagnostic; no reference counterpart) ------------------ */
/* The kernel rt_encrypt_uniform (decrypt = 0, len = plaintext bytes) or
 * rt_decrypt_uniform (decrypt = 1, len = token bytes) runs for n packets on
 * ctx's device, with one key (per_packet_keys = 0) or a key_idx array.  Lets
 * tests and callers check which path a batch shape takes (e.g. that the
 * 8-GPU c4 per-rank shard runs the long-token kernels). */
enum {
    RT_KERNEL_GENERAL = 0,      /* one packet per lane (k_encrypt / k_decrypt) */
    RT_KERNEL_ENC_LONG4 = 1,    /* single key, a lane quad per CBC chain (k_encrypt_long4) */
    RT_KERNEL_ENC_LONG = 2,     /* per-packet keys, hashing on waves of their own (k_encrypt_long) */
    RT_KERNEL_DEC_LONG2 = 3,    /* single key, producer/consumer HMAC chains (k_decrypt_long2) */
    RT_KERNEL_ENC_SPLIT = 4     /* single key, AES and HMAC chains on waves of their own (k_encrypt_split) */
};
int         rt_plan_uniform(const rt_ctx *ctx, uint32_t n, uint32_t len, int per_packet_keys, int decrypt);

/* ---- device-resident batch (Token.encrypt over n packets) ---------------- */
/* pt + pt_off[i] holds pt_len[i] plaintext bytes; key_idx[i] selects the key
 * (NULL: key 0 for every packet); iv + 16*i is packet i's IV; the token is
 * written at tok + tok_off[i] (rt_token_len(pt_len[i]) bytes).  Offsets need
 * no alignment.  All pointers are device pointers. */
int rt_encrypt(const rt_keyset *ks, const uint8_t *pt, const uint64_t *pt_off, const uint32_t *pt_len,
               const uint32_t *key_idx, const uint8_t *iv, uint8_t *tok, const uint64_t *tok_off,
               uint32_t n, void *stream);
/* Fixed-length batch: packet i at pt + i*pt_stride (pt_len bytes), token at
 * tok + i*tok_stride.  pt may be null when pt_len is 0. */
int rt_encrypt_uniform(const rt_keyset *ks, const uint8_t *pt, uint64_t pt_stride, uint32_t pt_len,
                       const uint32_t *key_idx, const uint8_t *iv, uint8_t *tok, uint64_t tok_stride,
                       uint32_t n, void *stream);

/* ---- device-resident batch (Token.decrypt over n tokens) ----------------- */
/* tok + tok_off[i] holds tok_len[i] token bytes; plaintext (up to
 * tok_len[i]-48 bytes, including the pad block) is written at pt + pt_off[i];
 * pt_len[i] receives the unpadded length on RT_ST_OK, the offending pad
 * byte on RT_ST_BAD_PAD (authenticated data), 0 otherwise; status[i] one
 * of RT_ST_*.  On any non-OK status the packet's plaintext region is zeroed
 * (unauthenticated plaintext is never left behind). */
int rt_decrypt(const rt_keyset *ks, const uint8_t *tok, const uint64_t *tok_off, const uint32_t *tok_len,
               const uint32_t *key_idx, uint8_t *pt, const uint64_t *pt_off, uint32_t *pt_len,
               int32_t *status, uint32_t n, void *stream);
int rt_decrypt_uniform(const rt_keyset *ks, const uint8_t *tok, uint64_t tok_stride, uint32_t tok_len,
                       const uint32_t *key_idx, uint8_t *pt, uint64_t pt_stride, uint32_t *pt_len,
                       int32_t *status, uint32_t n, void *stream);

/* ---- device-resident batch (Token.verify_hmac over n tokens) ------------- */
/* status[i] = RT_ST_OK when token i's last 32 bytes equal HMAC-SHA256(sk,
 * token[:-32]), RT_ST_BAD_HMAC when they do not, RT_ST_TOO_SHORT when
 * tok_len[i] <= 32 (Token.py:77-84: any length above 32 is hashed, whole AES
 * blocks or not).  Runs no AES and writes nothing but the status.  DEVICE
 * pointers; rt_verify_host takes HOST pointers and returns when `status` is
 * filled. */
int rt_verify(const rt_keyset *ks, const uint8_t *tok, const uint64_t *tok_off, const uint32_t *tok_len,
              const uint32_t *key_idx, int32_t *status, uint32_t n, void *stream);
int rt_verify_host(const rt_keyset *ks, const uint8_t *tok, const uint64_t *tok_off, const uint32_t *tok_len,
                   const uint32_t *key_idx, int32_t *status, uint32_t n);

/* ---- irregular batches: length bucketing -------------------------------- */
/* With RT_F_SORT_BY_LENGTH the batch is first grouped by length on the device
 * (three small kernels on the same stream) so that the lanes of a wavefront
 * carry packets of similar length; outputs stay at their own offsets, so the
 * result is identical to rt_encrypt / rt_decrypt.  `workspace` is a DEVICE
 * buffer of at least rt_workspace_bytes(n) bytes, owned by the caller and not
 * reused until the call's work on `stream` has completed. */
#define RT_F_SORT_BY_LENGTH 1u
uint64_t rt_workspace_bytes(uint32_t n);
int rt_encrypt_ex(const rt_keyset *ks, const uint8_t *pt, const uint64_t *pt_off, const uint32_t *pt_len,
                  const uint32_t *key_idx, const uint8_t *iv, uint8_t *tok, const uint64_t *tok_off,
                  uint32_t n, uint32_t flags, void *workspace, void *stream);
int rt_decrypt_ex(const rt_keyset *ks, const uint8_t *tok, const uint64_t *tok_off, const uint32_t *tok_len,
                  const uint32_t *key_idx, uint8_t *pt, const uint64_t *pt_off, uint32_t *pt_len,
                  int32_t *status, uint32_t n, uint32_t flags, void *workspace, void *stream);

/* ---- host-buffer convenience (PCIe-inclusive path) ----------------------- */
/* Same meaning with HOST pointers; H2D, kernel, D2H on a staging lane's
 * stream, synchronised (that stream only) before return. */
int rt_encrypt_host(const rt_keyset *ks, const uint8_t *pt, const uint64_t *pt_off, const uint32_t *pt_len,
                    const uint32_t *key_idx, const uint8_t *iv, uint8_t *tok, const uint64_t *tok_off,
                    uint32_t n);
int rt_decrypt_host(const rt_keyset *ks, const uint8_t *tok, const uint64_t *tok_off, const uint32_t *tok_len,
                    const uint32_t *key_idx, uint8_t *pt, const uint64_t *pt_off, uint32_t *pt_len,
                    int32_t *status, uint32_t n);

/* ---- key derivation (RNS.Cryptography.hkdf, HKDF.py:35-62) -------------- */
/* n independent HKDF-SHA256 derivations.  Item i: input key material
 * ikm + i*ikm_stride (ikm_len bytes; 0 is allowed, as b"" is in the
 * reference), salt + i*salt_stride (salt_len bytes; salt NULL or salt_len 0
 * means the reference's default of 32 zero bytes, HKDF.py:45-46; salts over
 * 64 bytes are hashed first as HMAC.py does with long keys; salt_stride 0
 * shares one salt row across all items, as Identity.encrypt does for packets
 * to one identity, and the salt's HMAC midstates are then computed once per
 * lane rather than once per item), a context shared
 * by all items (NULL / 0: empty, HKDF.py:48-49); `length` >= 1 output bytes
 * are written at out + i*out_stride (length 0 is RT_E_INVAL, HKDF.py:40-41).
 * Output blocks past 255 wrap the counter byte exactly as HKDF.py:60 does.
 * rt_hkdf takes DEVICE pointers and only enqueues; rt_hkdf_host takes HOST
 * pointers and returns when `out` is filled. */
int rt_hkdf(rt_ctx *ctx, const uint8_t *ikm, uint64_t ikm_stride, uint32_t ikm_len,
            const uint8_t *salt, uint64_t salt_stride, uint32_t salt_len,
            const uint8_t *context, uint32_t context_len,
            uint8_t *out, uint64_t out_stride, uint32_t length, uint32_t n, void *stream);
int rt_hkdf_host(rt_ctx *ctx, const uint8_t *ikm, uint64_t ikm_stride, uint32_t ikm_len,
                 const uint8_t *salt, uint64_t salt_stride, uint32_t salt_len,
                 const uint8_t *context, uint32_t context_len,
                 uint8_t *out, uint64_t out_stride, uint32_t length, uint32_t n);
/* Per-packet keying: derive n token keys of key_len (64 or 32) bytes with
 * HKDF (arguments as rt_hkdf, DEVICE pointers) and build their key tables,
 * without the derived keys ever leaving the device: key i of the keyset is
 * Token(hkdf(key_len, ikm_i, salt_i, context)) as Identity.encrypt /
 * __decrypt construct it (Identity.py:837-846).  Encrypt with key_idx[i] = i. */
rt_keyset *rt_keyset_create_hkdf(rt_ctx *ctx, const uint8_t *ikm, uint64_t ikm_stride, uint32_t ikm_len,
                                 const uint8_t *salt, uint64_t salt_stride, uint32_t salt_len,
                                 const uint8_t *context, uint32_t context_len, uint32_t key_len, uint32_t n,
                                 void *stream);

/* ---- X25519 (RNS/Cryptography/X25519.py:49-93) -------------------------- */
/* n independent exchanges, one per lane: out_i = X25519(scalar_i, point_i),
 * 32 bytes each, by the RFC 7748 ladder.  scalar_i at scalars + i*scalar_stride
 * (stride 0: one scalar for all, the receiver's case); point_i at
 * points + point_off[i] when point_off != NULL (e.g. the ephemeral public key
 * at the head of each token, read in place), else points + i*point_stride
 * (stride 0: one point for all, the sender's target key); points == NULL: the
 * base point 9 (public keys).  A non-zero stride is at least 32.  No alignment
 * is assumed.  As the reference's internal provider: the scalar is clamped
 * (_fix_secret), bit 255 of a point is ignored and a point >= p is taken
 * mod p (_fix_base_point), and a low-order point gives 32 zero bytes without
 * an error.  Constant time: no branch or address depends on a scalar.
 * rt_x25519 takes DEVICE pointers and only enqueues; rt_x25519_host takes HOST
 * pointers and returns when `out` is filled.  n == 0 is RT_OK. */
int rt_x25519(rt_ctx *ctx, const uint8_t *scalars, uint64_t scalar_stride, const uint8_t *points,
              uint64_t point_stride, const uint64_t *point_off, uint8_t *out, uint64_t out_stride,
              uint32_t n, void *stream);
int rt_x25519_host(rt_ctx *ctx, const uint8_t *scalars, uint64_t scalar_stride, const uint8_t *points,
                   uint64_t point_stride, const uint64_t *point_off, uint8_t *out, uint64_t out_stride,
                   uint32_t n);
/* Identity.encrypt / decrypt keying in one call (Identity.py:812-829, 861-871,
 * 887-888): the n shared secrets X25519(scalar_i, point_i) (arguments as
 * rt_x25519, DEVICE pointers) go to a stream-ordered device temporary, the
 * key derivation and key setup of rt_keyset_create_hkdf run over them
 * (ikm_len 32; salt, context and key_len as there), and the temporary is
 * freed in stream order: key i of the keyset is
 * Token(hkdf(key_len, X25519(scalar_i, point_i), salt_i, context)), and
 * neither the shared secrets nor the derived keys leave the device. */
rt_keyset *rt_keyset_create_x25519(rt_ctx *ctx, const uint8_t *scalars, uint64_t scalar_stride,
                                   const uint8_t *points, uint64_t point_stride, const uint64_t *point_off,
                                   const uint8_t *salt, uint64_t salt_stride, uint32_t salt_len,
                                   const uint8_t *context, uint32_t context_len, uint32_t key_len, uint32_t n,
                                   void *stream);

/* ---- Ed25519 (RNS/Cryptography/pure25519/eddsa.py, basic.py) ------------ */
/* n independent items, one per lane.  Item i's message is the msg_len[i]
 * bytes at msgs + msg_off[i] (uint64 offsets, uint32 lengths, n each; any
 * alignment; offsets may repeat and come in any order); msgs == NULL is
 * accepted only when every length is 0 (the _host calls check that; the device
 * calls cannot, and take every message as empty then).  Keys and seeds are 32 bytes at
 * base + i*stride, signatures 64 bytes; stride 0 means one row for all items
 * (one identity's key against many proofs), a non-zero key or seed stride is
 * at least 32, sig_stride and out_stride are at least 64 when n > 1.  A NULL
 * required pointer is RT_E_INVAL; n == 0 is RT_OK.  The plain calls take
 * DEVICE pointers and only enqueue on `stream`; the _host calls take HOST
 * pointers and return when the output is filled.
 *
 * Results follow the reference's internal provider (pure25519), which is what
 * Reticulum runs where PyCA is absent; a PyCA-backed node differs on the
 * marked lines (*).  rt_ed25519_verify writes ok[i] = 1 where eddsa.checkvalid
 * returns True and 0 where it returns False or raises:
 *   - the key and R (sig[:32]) must not be the canonical encoding of the
 *     identity, 01 00 .. 00; other encodings of it pass this test;
 *   - both must decode: y is the low 255 bits, taken mod p and not required
 *     to be below p; x = xrecover(y) must satisfy the curve equation; x is
 *     negated where its parity differs from bit 255 (x = 0 with the bit set
 *     stays 0);
 *   - [L]A and [L]R must be the identity: small-order and mixed-order points
 *     are rejected even where the cofactorless equation holds (*);
 *   - S is any 256-bit integer and is used mod L, so S >= L is accepted (*);
 *     h = SHA-512(R || A || M) as a little-endian integer mod L;
 *   - [S mod L]B = R + [h mod L]A as points, whatever R's encoding;
 *   - a key that is the identity in a non-canonical encoding is rejected
 *     unless h mod L = 0 (the reference's subgroup multiplication does not
 *     hold for it).
 * rt_ed25519_sign is eddsa.signature: h = SHA-512(seed), a = clamp(h[:32]),
 * r = SHA-512(h[32:] || M) mod L, R = [r]B, S = (r + SHA-512(R || A || M) a)
 * mod L, output enc(R) || S.  pubs == NULL: A = enc([a]B) is derived per item;
 * else A is read from pubs and trusted.  rt_ed25519_public writes enc([a]B).
 * Signing and public keys are constant time: no branch, loop bound or address
 * depends on the seed or on a value derived from it. */
int rt_ed25519_verify(rt_ctx *ctx, const uint8_t *pubs, uint64_t pub_stride, const uint8_t *sigs,
                      uint64_t sig_stride, const uint8_t *msgs, const uint64_t *msg_off, const uint32_t *msg_len,
                      uint8_t *ok, uint32_t n, void *stream);
int rt_ed25519_verify_host(rt_ctx *ctx, const uint8_t *pubs, uint64_t pub_stride, const uint8_t *sigs,
                           uint64_t sig_stride, const uint8_t *msgs, const uint64_t *msg_off,
                           const uint32_t *msg_len, uint8_t *ok, uint32_t n);
int rt_ed25519_sign(rt_ctx *ctx, const uint8_t *seeds, uint64_t seed_stride, const uint8_t *pubs,
                    uint64_t pub_stride, const uint8_t *msgs, const uint64_t *msg_off, const uint32_t *msg_len,
                    uint8_t *sigs_out, uint64_t out_stride, uint32_t n, void *stream);
int rt_ed25519_sign_host(rt_ctx *ctx, const uint8_t *seeds, uint64_t seed_stride, const uint8_t *pubs,
                         uint64_t pub_stride, const uint8_t *msgs, const uint64_t *msg_off,
                         const uint32_t *msg_len, uint8_t *sigs_out, uint64_t out_stride, uint32_t n);
int rt_ed25519_public(rt_ctx *ctx, const uint8_t *seeds, uint64_t seed_stride, uint8_t *out, uint64_t out_stride,
                      uint32_t n, void *stream);
int rt_ed25519_public_host(rt_ctx *ctx, const uint8_t *seeds, uint64_t seed_stride, uint8_t *out,
                           uint64_t out_stride, uint32_t n);

/* ---- ratchet trials (Identity.decrypt, RNS/Identity.py:865-878) --------- */
/* Identity.decrypt tries the receiver's ratchets in order and keeps the first
 * whose derived token key opens the token.  Token t has the candidate keys
 * pair_key[pair_off[t] .. pair_off[t+1]) of the key set, in the caller's
 * ratchet order (pair_off: n_tok + 1 entries from 0 to n_pairs).  first[t]
 * receives the rank (0-based, within token t's candidates) of the first
 * candidate whose HMAC-SHA256 tag verifies over a well-formed token
 * (len >= 64, len - 48 a multiple of 16; Token.py:77-84,114), or 0xFFFFFFFF.
 * Decrypting each opened token with that key (rt_decrypt* with key_idx)
 * completes the loop: a BAD_PAD there means no ratchet opens it, as every
 * later candidate that verifies is the same key.  rt_verify_trials takes
 * DEVICE pointers and only enqueues; _host takes HOST pointers, validates
 * the CSR and key indices, and returns when `first` is filled. */
int rt_verify_trials(const rt_keyset *ks, const uint8_t *tok, const uint64_t *tok_off, const uint32_t *tok_len,
                     const uint32_t *pair_off, const uint32_t *pair_key, uint32_t *first, uint32_t n_tok,
                     uint32_t n_pairs, void *stream);
int rt_verify_trials_host(const rt_keyset *ks, const uint8_t *tok, const uint64_t *tok_off, const uint32_t *tok_len,
                          const uint32_t *pair_off, const uint32_t *pair_key, uint32_t *first, uint32_t n_tok,
                          uint32_t n_pairs);

/* ---- Resource hashmap (RNS/Resource.py:426-468, 505-506) ---------------- */
/* map_hash_j = SHA-256(part_j || salt)[:4] for n_parts parts, DEVICE pointers.
 * Part j is data + part_off[j] (part_len[j] bytes) when part_off/part_len are
 * given, else the uniform segmentation of one resource that the sender uses:
 * data[j*sdu, min((j+1)*sdu, size)) with n_parts = ceil(size / sdu).  The
 * salt is the resource's random_hash (RANDOM_HASH_SIZE = 4 bytes): salts +
 * part_res[j]*salt_len (part_res NULL: every part uses salts[0..salt_len)).
 * map_hashes receives 4 bytes per part (MAPHASH_LEN).  If first_collision is
 * not NULL it receives, per resource, the first (batch-wide) part index whose map hash
 * equals one of the previous `guard` map hashes of the same resource
 * (ResourceAdvertisement.COLLISION_GUARD_SIZE = 224 in the reference), or
 * 0xFFFFFFFF: the point where the reference's loop breaks to draw a new
 * random_hash.  Parts of one resource must be contiguous and in order. */
int rt_map_hashes(rt_ctx *ctx, const uint8_t *data, const uint64_t *part_off, const uint32_t *part_len,
                  uint64_t size, uint32_t sdu, const uint8_t *salts, uint32_t salt_len, const uint32_t *part_res,
                  uint32_t n_res, uint32_t guard, uint8_t *map_hashes, uint32_t *first_collision, uint32_t n_parts,
                  void *stream);
/* One resource in HOST memory (uniform segmentation); returns when the
 * hashmap (4*ceil(size/sdu) bytes) and *first_collision are written. */
int rt_resource_hashmap_host(rt_ctx *ctx, const uint8_t *data, uint64_t size, uint32_t sdu,
                             const uint8_t *random_hash, uint32_t rh_len, uint32_t guard, uint8_t *hashmap,
                             uint32_t *first_collision);

/* ---- Resource integrity hash and proof (RNS/Resource.py:436-439, 698-699, 759-760) */
/* For n segments, DEVICE pointers, enqueued on the stream: segment i is
 * data + seg_off[i] (seg_len[i] bytes, any alignment, 0 allowed) and
 *   hash[i]  = SHA-256(segment_i || random_hashes[i*rh_len .. +rh_len))   (32 bytes)
 *   proof[i] = SHA-256(segment_i || hash[i])                              (32 bytes)
 * in one pass over the segment (rh_len <= 32; RANDOM_HASH_SIZE = 4 in the
 * reference).  Sender: expect_hash NULL; hash[i][:16] is the truncated_hash
 * and proof[i] the expected_proof.  Receiver: expect_hash (n x 32) holds the
 * advertised hashes; status[i] = 0 when the computed hash equals it, else 1
 * (Resource.CORRUPT), and proof[i] is computed over expect_hash[i]: the second
 * half of the proof packet hash || proof for an intact segment, 32 zero bytes
 * for a corrupt one (the reference never proves a corrupt resource).  proof
 * may be NULL; status may be NULL unless expect_hash is given. */
int rt_resource_hashes(rt_ctx *ctx, const uint8_t *data, const uint64_t *seg_off, const uint32_t *seg_len,
                       const uint8_t *random_hashes, uint32_t rh_len, const uint8_t *expect_hash, uint8_t *hash,
                       uint8_t *proof, int32_t *status, uint32_t n, void *stream);
/* One segment in HOST memory; returns when hash (32 bytes), proof (32 bytes,
 * may be NULL) and *status (may be NULL without expect_hash) are written. */
int rt_resource_hashes_host(rt_ctx *ctx, const uint8_t *data, uint64_t size, const uint8_t *random_hash,
                            uint32_t rh_len, const uint8_t *expect_hash, uint8_t *hash, uint8_t *proof,
                            int32_t *status);
/* Batches of fewer segments than this run one workgroup per segment
 * (k_resource_hashes_split) instead of one lane per segment; same results. */
uint32_t rt_resource_hash_split_below(void);

/* ---- wire-side neighbours (framing, IFAC, packet header) --------------- */
/* HDLC framing of n packets into one stream, in order: frame i is
 * 7E || escape(packet i) || 7E (escape: 7D -> 7D 5D, 7E -> 7D 5E) at
 * out + frame_off[i]; frame_off has n+1 entries, frame_off[n] = total bytes.
 * out needs at most sum(2*len+2) bytes.  DEVICE pointers; `workspace` of
 * rt_hdlc_frame_workspace_bytes(n) bytes. */
uint64_t rt_hdlc_frame_workspace_bytes(uint32_t n);
int rt_hdlc_frame(rt_ctx *ctx, const uint8_t *pkt, const uint64_t *pkt_off, const uint32_t *pkt_len, uint32_t n,
                  uint8_t *out, uint64_t *frame_off, void *workspace, void *stream);
/* rt_hdlc_frame with the packet count on the device: only the first
 * m = min(max(*n_dev, 0), n) entries are packets (n_dev: a device int64, e.g.
 * reply_counts of rt_reply_gather).  Entries m .. n-1 contribute no bytes at
 * all, whatever their pkt_len and pkt_off hold (they are not read), and
 * frame_off[i] = frame_off[n] = the total for every i >= m, so
 * out[0, frame_off[n]) is exactly the m frames.  With *n_dev >= n the result is
 * rt_hdlc_frame's.  n = 0 writes frame_off[0] = 0.  Same workspace. */
int rt_hdlc_frame_counted(rt_ctx *ctx, const uint8_t *pkt, const uint64_t *pkt_off, const uint32_t *pkt_len,
                          uint32_t n, const int64_t *n_dev, uint8_t *out, uint64_t *frame_off, void *workspace,
                          void *stream);
/* One pass of the HDLC read loop over buf[0, len) (everything received so
 * far).  For every pair of consecutive 7E flags k, k+1 (at most max_pairs):
 * the frame between them, unescaped with the loop's two replace passes, is
 * written at out + frame_off[k] (its position in buf, so `out` needs len
 * bytes), frame_len[k] bytes, and status[k] is RT_FRAME_OK (handed to
 * process_incoming), RT_FRAME_BAD_LEN (dropped by check_frame_len: length <=
 * HEADER_MINSIZE = 19 or > hw_mtu + ifac_size) or RT_FRAME_EMPTY (skipped).
 * counts[0] = number of pairs, counts[1] = bytes consumed: the loop keeps
 * buf[counts[1], len) for the next read (all of it is dropped when no flag is
 * present or the tail from the last flag exceeds 2*hw_mtu).  DEVICE
 * pointers; `workspace` of rt_hdlc_deframe_workspace_bytes(len) bytes. */
#define RT_FRAME_OK      0
#define RT_FRAME_BAD_LEN 1
#define RT_FRAME_EMPTY   2
uint64_t rt_hdlc_deframe_workspace_bytes(uint64_t len);
int rt_hdlc_deframe(rt_ctx *ctx, const uint8_t *buf, uint64_t len, uint32_t hw_mtu, uint32_t ifac_size, uint8_t *out,
                    uint64_t *frame_off, uint32_t *frame_len, int32_t *status, uint64_t *counts, uint64_t max_pairs,
                    void *workspace, void *stream);
/* rt_hdlc_deframe with every frame in its own 128-B-aligned slot instead of
 * at its position in buf: frame k is written at the first offset >=
 * pos_k + 1 + 128*k (pos_k: its opening flag) at which byte line_phase (< 128)
 * of the frame starts a 128-B line of memory, so `out` needs
 * len + 128 * (max_pairs + 1) bytes.  Frame bytes, lengths, statuses and
 * counts are those of rt_hdlc_deframe; only frame_off differs.  With
 * line_phase = 35 a HEADER_1 packet at the frame's offset (as it is, or
 * IFAC-unmasked into another buffer at the same offset) has its token
 * ciphertext on a line. */
int rt_hdlc_deframe_slots(rt_ctx *ctx, const uint8_t *buf, uint64_t len, uint32_t hw_mtu, uint32_t ifac_size,
                          uint32_t line_phase, uint8_t *out, uint64_t *frame_off, uint32_t *frame_len, int32_t *status,
                          uint64_t *counts, uint64_t max_pairs, void *workspace, void *stream);
/* The frames one rt_hdlc_deframe pass hands on (pair k < counts[0] with
 * status[k] == RT_FRAME_OK), in stream order, to the front of f_off / f_len
 * (their offsets and lengths in the deframed buffer) and frame_pair (k);
 * *n_frames (device int64) = their number.  Entries n_frames .. max_pairs-1
 * are f_off 0, f_len 0, frame_pair -1, so per-packet stages can run over all
 * max_pairs entries without the host learning n_frames.  The outputs must not
 * overlap frame_off / frame_len (compaction in place would race; RT_E_INVAL).
 * DEVICE pointers; `workspace` of rt_frames_compact_workspace_bytes(max_pairs)
 * bytes. */
uint64_t rt_frames_compact_workspace_bytes(uint64_t max_pairs);
int rt_frames_compact(rt_ctx *ctx, const uint64_t *frame_off, const uint32_t *frame_len, const int32_t *status,
                      const uint64_t *counts, uint64_t max_pairs, uint64_t *f_off, uint32_t *f_len,
                      int64_t *frame_pair, int64_t *n_frames, void *workspace, void *stream);
/* IFAC on transmit: packet i (pkt + pkt_off[i], pkt_len[i] >= 2 bytes) with
 * its access code ifac + i*ifac_size (the last ifac_size bytes of the
 * interface identity's Ed25519 signature of the packet: rt_ifac_sign makes it
 * on the device, or the caller supplies its own) becomes pkt_len[i] + ifac_size bytes at
 * out + out_off[i]: IFAC flag set, IFAC inserted after the 2 header bytes,
 * all but the IFAC masked with HKDF(len + ifac_size, ifac, ifac_key).
 * ifac_key: key_len (<= 64) bytes shared by the batch.  DEVICE pointers. */
int rt_ifac_mask(rt_ctx *ctx, const uint8_t *pkt, const uint64_t *pkt_off, const uint32_t *pkt_len,
                 const uint8_t *ifac, uint32_t ifac_size, const uint8_t *ifac_key, uint32_t key_len, uint8_t *out,
                 const uint64_t *out_off, uint32_t n, void *stream);
/* IFAC on inbound: status[i] = 0 when the packet carries the IFAC flag and
 * is longer than 2 + ifac_size; then its IFAC goes to ifac_out + i*ifac_size
 * and the unmasked packet without it (pkt_len[i] - ifac_size bytes, flag
 * cleared) to out + out_off[i].  status 1: the reference drops the packet
 * before signing.  out_len (may be NULL) receives the unmasked length,
 * pkt_len[i] - ifac_size, where status[i] is 0 and 0 elsewhere, ready as
 * rt_packet_unpack's pkt_len.  The access code is then compared with the tail
 * of sign(unmasked packet) (Transport.py:1470-1474): rt_ifac_check does that
 * on the device over (out, out_off, out_len, ifac_out, status). */
#define RT_IFAC_OK       0   /* unmasked (and, after rt_ifac_check, the access code matches) */
#define RT_IFAC_DROPPED  1   /* no IFAC flag, or not longer than 2 + ifac_size */
#define RT_IFAC_MISMATCH 2   /* rt_ifac_check: access code does not match */
int rt_ifac_unmask(rt_ctx *ctx, const uint8_t *pkt, const uint64_t *pkt_off, const uint32_t *pkt_len,
                   uint32_t ifac_size, const uint8_t *ifac_key, uint32_t key_len, uint8_t *ifac_out, uint8_t *out,
                   const uint64_t *out_off, int32_t *status, uint32_t *out_len, uint32_t n, void *stream);
/* The access code of an interface with IFAC, made and checked on the device:
 * ifac = sign(packet)[-ifac_size:] with the interface identity's Ed25519 key
 * (Transport.transmit, Transport.py:1073; Transport.inbound's
 * expected_ifac, Transport.py:1470-1474).  One 32-byte seed (ifac_key[32:64]
 * of Identity.from_bytes(ifac_key), Reticulum.py:968-971) and its 32-byte
 * public key (rt_ed25519_public of the seed; trusted) serve the whole batch;
 * packet i is pkt + pkt_off[i], pkt_len[i] bytes at any alignment, and an item
 * with pkt_len[i] == 0 is skipped without its offset being used.  The
 * signature is rt_ed25519_sign's (the reference's internal provider), with the
 * fixed-base multiplication from a table of [2^i]B; constant time in the seed
 * as rt_ed25519_sign is.  ifac_size is 1..64 (above 32 the code reaches into
 * R).  DEVICE pointers, enqueued on the stream.
 *   rt_ifac_sign   writes the code to ifac_out + i*ifac_size (zeros for a
 *                  skipped item), ready as rt_ifac_mask's ifac.
 *   rt_ifac_check  where status[i] == RT_IFAC_OK and the code differs from
 *                  ifac + i*ifac_size: status[i] = RT_IFAC_MISMATCH and
 *                  pkt_len[i] = 0, so that rt_packet_unpack and everything
 *                  after it drop the packet as the reference's `return` does.
 *                  Items with another status keep status and length. */
int rt_ifac_sign(rt_ctx *ctx, const uint8_t *seed, const uint8_t *pub, const uint8_t *pkt, const uint64_t *pkt_off,
                 const uint32_t *pkt_len, uint8_t *ifac_out, uint32_t ifac_size, uint32_t n, void *stream);
int rt_ifac_check(rt_ctx *ctx, const uint8_t *seed, const uint8_t *pub, const uint8_t *pkt, const uint64_t *pkt_off,
                  uint32_t *pkt_len, const uint8_t *ifac, uint32_t ifac_size, int32_t *status, uint32_t n,
                  void *stream);
/* Packet.unpack + get_hash per packet (96 bytes).  ok = 0 where unpack
 * returns False (hop count >= 128, packet too short for its header). */
typedef struct rt_packet_fields {
    uint8_t  ok, flags, hops, header_type, context_flag, transport_type, destination_type, packet_type;
    uint8_t  context, reserved[3];
    uint32_t data_offset, data_len;     /* data = packet[data_offset : data_offset + data_len] */
    uint8_t  transport_id[16];          /* HEADER_2 only */
    uint8_t  destination_hash[16];
    uint8_t  packet_hash[32];           /* SHA-256(flags & 0x0F || packet[2 or 18:]) */
    uint8_t  reserved2[12];
} rt_packet_fields;
int rt_packet_unpack(rt_ctx *ctx, const uint8_t *pkt, const uint64_t *pkt_off, const uint32_t *pkt_len,
                     rt_packet_fields *fields, uint32_t n, void *stream);
/* The token inside each unpacked packet: tok_off[i] = pkt_off[i] +
 * fields[i].data_offset, tok_len[i] = fields[i].data_len where fields[i].ok;
 * tok_off[i] = pkt_off[i], tok_len[i] = 0 (rejected by rt_decrypt as too
 * short) elsewhere.  Feeds rt_decrypt straight from rt_packet_unpack's
 * records.  DEVICE pointers. */
int rt_token_spans(rt_ctx *ctx, const rt_packet_fields *fields, const uint64_t *pkt_off, uint32_t n,
                   uint64_t *tok_off, uint32_t *tok_len, void *stream);
/* Packet.pack's header for n packets at out + out_off[i]: flags, hops (NULL:
 * 0), [transport_id (16 B each; NULL: HEADER_1 for all)], destination hash
 * (16 B each), context — 19 or 35 bytes; the payload (a token from
 * rt_encrypt, written at out_off[i] + header length) follows. */
int rt_packet_pack_headers(rt_ctx *ctx, const uint8_t *flags, const uint8_t *hops, const uint8_t *transport_id,
                           const uint8_t *destination_hash, const uint8_t *context, uint8_t *out,
                           const uint64_t *out_off, uint32_t n, void *stream);

/* ---- link table and dispatch (Transport.py:2161-2176, Link.py:941-1148) -- */
/* A node has many links at once.  Transport.inbound finds the link of a DATA
 * packet as the first link in active_links whose link_id equals the packet's
 * destination hash; a link table does that on the device: 16-byte link id ->
 * a uint32 value of the caller's (the index of the link's key in its key set).
 * It is an open-addressing hash table in device memory with a fixed number of
 * slots, the smallest power of two that is at least 2 * max_links
 * (rt_linktable_capacity); max_links is 1 .. 2^29.  No id value is special.
 *
 * The calls below take DEVICE pointers and a stream and only enqueue; ids are
 * n x 16 bytes at any alignment; n == 0 is RT_OK, n is at most 2^30 - 2.  The
 * _host forms take HOST pointers and return when the outputs are filled.
 * Calls on one table take effect in the order the host makes them, whatever
 * their streams: a call on another stream than the one before it first waits
 * for that one.  rt_linktable_destroy never blocks: the memory is released
 * once the last call has completed (the key sets' rule, above).
 *
 * rt_linktable_insert writes status[i]:
 *   RT_LINK_OK         entered with values[i];
 *   RT_LINK_DUPLICATE  the id is already present, or appears at a lower index
 *                      of this batch: the earlier one stays, as the first
 *                      match in active_links wins.  Within a batch the lowest
 *                      index wins whatever the scheduling;
 *   RT_LINK_FULL       no free slot.  A table that holds at most max_links
 *                      entries never gives it.  When the new ids of one batch
 *                      outnumber the free slots, which of them get the last
 *                      slots is not specified.
 * rt_linktable_remove writes RT_LINK_OK, or RT_LINK_MISSING where the id is not
 * present or is removed at a lower index of this batch.  Ids further along the
 * probe chain are still found, and the id can be inserted again.  The slots
 * removals leave behind are reclaimed by a rebuild in place, enqueued ahead of
 * an insert when removals came since the last rebuild and the host's upper
 * bound on used slots plus n passes 3/4 of the capacity.
 * rt_linktable_lookup writes values_out[i] (0xFFFFFFFF on a miss) and
 * found_out[i] (1 / 0).  rt_linktable_count copies the number of entries
 * present to *count_out (DEVICE) on the stream.  Every probe is bounded by the
 * capacity. */
#define RT_LINK_OK        0
#define RT_LINK_DUPLICATE 1
#define RT_LINK_FULL      2
#define RT_LINK_MISSING   3
typedef struct rt_linktable rt_linktable;
rt_linktable *rt_linktable_create(rt_ctx *ctx, uint32_t max_links);
void          rt_linktable_destroy(rt_linktable *tab);
uint32_t      rt_linktable_capacity(const rt_linktable *tab);
int rt_linktable_insert(rt_linktable *tab, const uint8_t *ids, const uint32_t *values, int32_t *status, uint32_t n,
                        void *stream);
int rt_linktable_remove(rt_linktable *tab, const uint8_t *ids, int32_t *status, uint32_t n, void *stream);
int rt_linktable_lookup(rt_linktable *tab, const uint8_t *ids, uint32_t *values_out, uint8_t *found_out, uint32_t n,
                        void *stream);
int rt_linktable_count(rt_linktable *tab, uint32_t *count_out, void *stream);
int rt_linktable_insert_host(rt_linktable *tab, const uint8_t *ids, const uint32_t *values, int32_t *status,
                             uint32_t n);
int rt_linktable_remove_host(rt_linktable *tab, const uint8_t *ids, int32_t *status, uint32_t n);
int rt_linktable_lookup_host(rt_linktable *tab, const uint8_t *ids, uint32_t *values_out, uint8_t *found_out,
                             uint32_t n);
/* rt_token_spans plus the dispatch, one pass over rt_packet_unpack's records.
 * Per packet: route[i] (below), link[i] = the table's value for the packet's
 * destination hash or -1, and the span and key for rt_decrypt: tok_off[i] /
 * tok_len[i] = the packet's data and key_idx[i] = the value where route is
 * RT_ROUTE_LINK_DECRYPT; an empty span at pkt_off[i] and key_idx 0 elsewhere
 * (RT_ST_TOO_SHORT in the decrypt, as every dropped packet).  n_keys is the
 * size of the key set the batch is decrypted with: a found link whose value is
 * not below it is never decrypted (RT_ROUTE_LINK_PLAIN).
 * The initiator-only and responder-only rules (LRRTT, the 0xFF keepalive),
 * whether a channel exists, and the attached-interface check
 * (Transport.py:2166) stay with the caller, who filters by link[i]. */
#define RT_ROUTE_NOT_LINK     0  /* unpack failed, destination type not LINK, or neither DATA nor PROOF */
#define RT_ROUTE_NO_LINK      1  /* a link packet whose id is not in the table: dropped */
#define RT_ROUTE_LINK_PLAIN   2  /* link found, Link.receive does not decrypt: every PROOF; DATA with context
                                    KEEPALIVE, RESOURCE, CACHE_REQUEST or one Link.receive has no branch for */
#define RT_ROUTE_LINK_DECRYPT 3  /* DATA with context NONE, LINKIDENTIFY, REQUEST, RESPONSE, LRRTT, LINKCLOSE,
                                    RESOURCE_ADV, RESOURCE_REQ, RESOURCE_HMU, RESOURCE_ICL, RESOURCE_RCL, CHANNEL */
int rt_link_spans(rt_linktable *tab, const rt_packet_fields *fields, const uint64_t *pkt_off, uint32_t n,
                  uint32_t n_keys, uint64_t *tok_off, uint32_t *tok_len, uint32_t *key_idx, int32_t *link,
                  uint8_t *route, void *stream);

/* ---- packet hash list and packet filter (Transport.py:1377-1427, 1525-1545, 656-658) */
/* Transport.inbound drops the packets it has seen before.  A hash list is
 * Transport.packet_hashlist and packet_hashlist_prev in device memory: two
 * generations, current and previous, of a set of 32-byte packet hashes, each an
 * open-addressing table of the link table's build with the smallest power of
 * two of slots that is at least 2 * max_hashes (rt_hashlist_capacity), holding
 * at most max_hashes entries; max_hashes is 1 .. 2^29 (the reference's
 * hashlist_maxsize is 1 000 000).  No hash value is special.
 *
 * The calls take DEVICE pointers and a stream and only enqueue; hashes are
 * n x 32 bytes at any alignment; n == 0 is RT_OK, n is at most 2^30 - 2.  The
 * _host forms take HOST pointers and return when the outputs are filled.
 * Calls on one list take effect in the order the host makes them, whatever
 * their streams, and rt_hashlist_destroy never blocks (the link table's rules).
 *
 * rt_packet_filter is packet_filter plus the remember step of
 * Transport.inbound for the n records rt_packet_unpack wrote, as if the
 * packets were processed one after another in index order, with
 * hops = fields[i].hops + 1 (Transport.py:1496).  status[i]:
 *   RT_FILTER_PASS             handed on;
 *   RT_FILTER_NO_PACKET        fields[i].ok was 0;
 *   RT_FILTER_OTHER_TRANSPORT  HEADER_2, not an ANNOUNCE, and the transport id
 *                              is not transport_identity (16 bytes);
 *   RT_FILTER_BAD_ANNOUNCE     a PLAIN or GROUP announce, or an announce for
 *                              another destination type than SINGLE whose hash
 *                              is in the list;
 *   RT_FILTER_HOPS             a PLAIN or GROUP packet with hops > 1;
 *   RT_FILTER_DUPLICATE        the hash is in either generation, or belongs to
 *                              a packet at a lower index of this batch that
 *                              passed and was remembered.
 * Contexts KEEPALIVE, RESOURCE_REQ, RESOURCE_PRF, RESOURCE, CACHE_REQUEST and
 * CHANNEL, and the PLAIN and GROUP packets that pass, do not consult the list;
 * a SINGLE announce passes even when its hash is present.  Every packet that
 * passes is entered into the current generation, except a PROOF with context
 * LRPROOF and a packet whose destination hash is found in `transit` (an
 * rt_linktable of the list's context standing for Transport.link_table, the
 * links this node carries for others; NULL: none).  A hash present in the
 * previous generation alone makes a duplicate and is not moved; a SINGLE
 * announce found there passes and is entered into the current one.
 * A dropped packet also gets fields[i].ok = 0, so that rt_link_spans and
 * rt_token_spans give it an empty span; the rest of its record stays.
 * A packet that would be entered when the current generation already holds
 * max_hashes entries (or finds no free slot) still passes, is not entered, and
 * adds one to the overflow count.  When the new hashes of one batch outnumber
 * the room left, as many as there is room for are entered and which of them is
 * not specified; the caller avoids all this with rt_hashlist_cull.
 *
 * rt_hashlist_cull is the job loop's step: when the current generation holds
 * more than max_hashes / 2 entries it becomes the previous one and the current
 * one becomes empty; otherwise nothing changes.  Decided on the device: the
 * call reads nothing back.
 * rt_hashlist_add enters hashes into the current generation (add_packet_hash:
 * reloading a saved list, hashes the caller deferred), under the same rule for
 * a full generation.  rt_hashlist_remove removes from the current generation
 * only (Transport.py:2186-2187) and writes RT_LINK_OK, or RT_LINK_MISSING where
 * the hash is not there or is removed at a lower index of this batch.
 * rt_hashlist_contains writes 0, 1 (current generation) or 2 (previous only).
 * rt_hashlist_counts writes three words: entries in the current generation,
 * in the previous one, and the overflow count. */
#define RT_FILTER_PASS            0
#define RT_FILTER_NO_PACKET       1
#define RT_FILTER_OTHER_TRANSPORT 2
#define RT_FILTER_BAD_ANNOUNCE    3
#define RT_FILTER_HOPS            4
#define RT_FILTER_DUPLICATE       5
typedef struct rt_hashlist rt_hashlist;
rt_hashlist *rt_hashlist_create(rt_ctx *ctx, uint32_t max_hashes);
void         rt_hashlist_destroy(rt_hashlist *list);
uint32_t     rt_hashlist_capacity(const rt_hashlist *list);
int rt_packet_filter(rt_hashlist *list, rt_linktable *transit, const uint8_t *transport_identity,
                     rt_packet_fields *fields, uint32_t n, int32_t *status, void *stream);
int rt_hashlist_cull(rt_hashlist *list, void *stream);
int rt_hashlist_add(rt_hashlist *list, const uint8_t *hashes, uint32_t n, void *stream);
int rt_hashlist_remove(rt_hashlist *list, const uint8_t *hashes, uint32_t n, int32_t *status, void *stream);
int rt_hashlist_contains(rt_hashlist *list, const uint8_t *hashes, uint32_t n, uint8_t *found_out, void *stream);
int rt_hashlist_counts(rt_hashlist *list, uint32_t *out, void *stream);
int rt_hashlist_add_host(rt_hashlist *list, const uint8_t *hashes, uint32_t n);
int rt_hashlist_remove_host(rt_hashlist *list, const uint8_t *hashes, uint32_t n, int32_t *status);
int rt_hashlist_contains_host(rt_hashlist *list, const uint8_t *hashes, uint32_t n, uint8_t *found_out);

/* ---- announce validation (Identity.py:505-606; Transport.py:1748-1750, 1772) */
/* Transport.inbound runs Identity.validate_announce(packet,
 * only_validate_signature=True) on every announce (Transport.py:1748-1750) and
 * the full validate_announce on those not addressed to a local destination
 * (:1772).  rt_announce_validate answers both for the n records
 * rt_packet_unpack wrote (after rt_packet_filter where there is one: a dropped
 * packet has ok = 0), reading each announce inside its packet at
 * pkt + pkt_off[i]: data = public key (64) ‖ name hash (10) ‖ random hash (10)
 * ‖ [ratchet (32), with the context flag] ‖ signature (64) ‖ app data, the
 * signed data being destination hash ‖ data without the signature
 * (Identity.py:505-545), verified as rt_ed25519_verify verifies (the
 * reference's internal provider, every acceptance rule of it).  status[i]:
 *   only_validate_signature=True returns True  for RT_ANNOUNCE_VALID and
 *                                              RT_ANNOUNCE_BAD_DESTINATION;
 *   the full check returns True                for RT_ANNOUNCE_VALID alone,
 * given that nothing of the caller's part below rejects the announce.
 * identity_hash (n x 16, may be NULL) receives the announced identity's hash,
 * SHA-256(public key)[:16], for every record whose signature was checked
 * (VALID, BAD_SIGNATURE, BAD_DESTINATION) and zeros for the others.  It is the
 * handle for what stays with the caller: Transport.blackholed_identities
 * (Identity.py:553-556), the known_destinations public-key collision check
 * (:569-575), Identity.remember (:577), ratchet bookkeeping (:595) and ingress
 * limiting (Transport.py:1752-1768).
 * DEVICE pointers; the call only enqueues on the stream and never
 * synchronises (its temporary, n + 16 words, comes from the context's
 * stream-ordered pool).  n == 0 is RT_OK; pkt, pkt_off, fields or status NULL
 * is RT_E_INVAL. */
#define RT_ANNOUNCE_VALID            0
#define RT_ANNOUNCE_NOT_ANNOUNCE     1   /* fields[i].ok == 0 or another packet type: nothing checked */
#define RT_ANNOUNCE_SHORT            2   /* data shorter than key, name hash, random hash, [ratchet,] signature */
#define RT_ANNOUNCE_BAD_SIGNATURE    3
#define RT_ANNOUNCE_BAD_DESTINATION  4   /* signature valid (line 1749 passes), destination hash not of this identity (line 1772 fails) */
int rt_announce_validate(rt_ctx *ctx, const uint8_t *pkt, const uint64_t *pkt_off, const rt_packet_fields *fields,
                         uint32_t n, int32_t *status, uint8_t *identity_hash /* n x 16, may be NULL */, void *stream);

/* ---- packet proofs on a link (Link.py:378-389, 943-955, 1140-1145; Transport.py:2326-2363) */
/* Both directions of the packet proof, over the n records rt_packet_unpack
 * wrote and what rt_link_spans made of them.  The links' signing rows are
 * indexed by the link table's value l (the index of the link's key): seeds
 * and publics 32 bytes each at l*key_stride (key_stride 0: one row for every
 * link, responder links that share their owner's key; else at least 32;
 * publics is rt_ed25519_public of seeds and trusted), flags one byte each,
 * peer_publics 32 bytes each at 32*l (the link's peer_sig_pub).  DEVICE
 * pointers; the calls only enqueue on the stream and never synchronise (their
 * temporaries, n + 16 and 2n + 16 words, come from the context's
 * stream-ordered pool).  n == 0 is RT_OK; a NULL required pointer is RT_E_INVAL.
 *
 * rt_link_prove is Link.receive's packet.prove().  Record i is proved when
 * fields[i].ok, it is a DATA packet, link[i] is 0 .. n_links-1 and either
 *   - its context is NONE, route[i] is RT_ROUTE_LINK_DECRYPT, token_status[i]
 *     (rt_decrypt's) is RT_ST_OK and flags[link[i]] has RT_LINK_PROVE_ALL, or
 *   - its context is CHANNEL and flags[link[i]] has RT_LINK_HAS_CHANNEL,
 *     whatever the token's status: the reference proves before it decrypts.
 * Then proof_len[i] = 115 and proofs + i*proof_stride (proof_stride >= 115)
 * receives the packet Link.prove_packet sends: flags 0x0F, hops 0, the link id
 * (the record's destination hash), context 0x00, the packet hash and its
 * signature under seeds[link[i]], rt_ed25519_sign's bit for bit with the
 * fixed-base multiplication from a table, constant time in the seed.  Every
 * other record gets proof_len[i] = 0 and its row is not written.  Links whose
 * destination proves by callback (PROVE_APP) get flags 0; the caller signs
 * what its callback picks with rt_ed25519_sign over the records' packet_hash.
 *
 * A receipt table is Transport.receipts on the device: an rt_linktable whose
 * ids are the first 16 bytes of a packet hash and whose values are receipt ids
 * 0 .. max_receipts-1 of the caller's choosing, beside receipt_hashes
 * (max_receipts x 32 bytes, DEVICE, the caller's), the full hash by id.
 * Adding receipts is rt_linktable_insert (hash[:16], id) followed by
 * rt_receipt_store over the same batch and the status the insert wrote:
 * receipt_hashes[ids[i]] = hashes[i] (n x 32) where status[i] is RT_LINK_OK
 * and ids[i] < max_receipts, so a duplicate leaves the earlier entry and its
 * hash untouched.  Timeouts and culling are rt_linktable_remove.
 *
 * rt_proof_settle is the last branch of Transport.inbound's PROOF handling
 * with PacketReceipt.validate_link_proof, as if the packets came one after
 * another in index order.  proof_status[i], the first rule that applies:
 *   RT_PROOF_NOT_PROOF      fields[i].ok == 0, not a PROOF, or context LRPROOF
 *                           (0xFF) or RESOURCE_PRF (0x05);
 *   RT_PROOF_NOT_LINK       a PROOF whose destination type is not LINK: proofs
 *                           for SINGLE destinations stay with the caller;
 *   RT_PROOF_NO_LINK        link[i] is not 0 .. n_links-1 (rt_link_spans gives
 *                           -1 for an id that is not in the link table);
 *   RT_PROOF_SHORT          data shorter than 96 bytes;
 *   RT_PROOF_NO_RECEIPT     no receipt holds data[:32], compared in full, or a
 *                           proof at a lower index of this batch delivered it;
 *   RT_PROOF_BAD_SIGNATURE  data[32:96] is not peer_publics[link[i]]'s
 *                           signature of data[:32], as rt_ed25519_verify judges;
 *   RT_PROOF_DELIVERED      verified: receipt[i] is the receipt's id and the
 *                           entry is removed from the table inside the call.
 * receipt[i] is -1 for every other status.  Data past 96 bytes is ignored
 * (Transport.py:2334-2335 tries every receipt then, Packet.py:436-441 slices).
 * When one valid proof comes several times in a batch the lowest index is
 * delivered whatever the scheduling, and a copy with a bad signature below it
 * does not stand in its way. */
#define RT_LINK_PROVE_ALL   1u
#define RT_LINK_HAS_CHANNEL 2u
#define RT_PROOF_DELIVERED     0
#define RT_PROOF_NOT_PROOF     1
#define RT_PROOF_NOT_LINK      2
#define RT_PROOF_NO_LINK       3
#define RT_PROOF_SHORT         4
#define RT_PROOF_NO_RECEIPT    5
#define RT_PROOF_BAD_SIGNATURE 6
int rt_link_prove(rt_ctx *ctx, const rt_packet_fields *fields, const uint8_t *route, const int32_t *link,
                  const int32_t *token_status, const uint8_t *seeds, const uint8_t *publics, uint64_t key_stride,
                  const uint8_t *flags, uint32_t n_links, uint8_t *proofs, uint64_t proof_stride, uint32_t *proof_len,
                  uint32_t n, void *stream);
int rt_receipt_store(rt_linktable *receipts, uint8_t *receipt_hashes, uint32_t max_receipts, const uint8_t *hashes,
                     const uint32_t *ids, const int32_t *status, uint32_t n, void *stream);
int rt_proof_settle(rt_linktable *receipts, const uint8_t *receipt_hashes, uint32_t max_receipts, const uint8_t *pkt,
                    const uint64_t *pkt_off, const rt_packet_fields *fields, const int32_t *link,
                    const uint8_t *peer_publics, uint32_t n_links, int32_t *proof_status, int32_t *receipt, uint32_t n,
                    void *stream);

/* ---- link requests (Transport.py:2127-2158, Destination.py:414-435, Link.py:186-227, 336-376) */
/* The responder side of link establishment for the node's own SINGLE
 * destinations, over the n records rt_packet_unpack wrote (after
 * rt_packet_filter where there is one: a dropped packet has ok = 0) and before
 * rt_link_spans, so that the read's own packets on a new link find it.
 *
 * The destinations are an rt_linktable from 16-byte destination hash to a row
 * 0 .. n_dests-1 of dest_seeds / dest_publics (32 bytes each: the identity's
 * Ed25519 seed and rt_ed25519_public of it, trusted) and dest_flags (one byte:
 * RT_DEST_ACCEPTS, accept_link_requests; RT_LINK_PROVE_ALL and
 * RT_LINK_HAS_CHANNEL, which a new link's signer flags inherit).  nh_mtu is
 * the receiving interface's next-hop MTU as Transport.py:2138-2141 computes it
 * (HW_MTU when autoconfigured or fixed, else 500), or negative for an
 * interface without HW_MTU.  status[i], the first rule that applies:
 *   RT_LINKREQ_NOT_REQUEST      fields[i].ok == 0 or not a LINKREQUEST;
 *   RT_LINKREQ_OTHER_TRANSPORT  HEADER_2 and the transport id is not
 *                               transport_identity (16 bytes);
 *   RT_LINKREQ_NO_DESTINATION   destination type not SINGLE, or the hash is not
 *                               in `dests`;
 *   RT_LINKREQ_NOT_ACCEPTING    the destination's RT_DEST_ACCEPTS is clear;
 *   RT_LINKREQ_BAD_MODE         a path MTU (67 bytes of data, its 21-bit value
 *                               not 0) above nh_mtu whose mode bits are not
 *                               AES-256-CBC: the clamp's signalling_bytes raises;
 *   RT_LINKREQ_BAD_SIZE         the data is neither 64 nor 67 bytes.  With a
 *                               path MTU and no nh_mtu the three signalling
 *                               bytes are cut off first (64 bytes, default mode
 *                               and MTU), and the link id then covers them;
 *   RT_LINKREQ_BAD_MODE         mode bits (data[64] >> 5 of 67 bytes) not 1;
 *   RT_LINKREQ_NO_SLOT          valid request r in index order has no slot:
 *                               r >= m, slots[r] not below n_keys and n_links,
 *                               or the link table has no room;
 *   RT_LINKREQ_DUPLICATE        its link id is in the link table already, or
 *                               belongs to a request at a lower index that holds
 *                               a slot: the lowest index wins whatever the
 *                               scheduling, the duplicate's slot stays unused;
 *   RT_LINKREQ_ACCEPTED         the link exists when the call has run.
 * For every valid request (the last three) link_id[i] (n x 16) is the link id
 * (Link.link_id_from_lr_packet on the packet as received) and mtu[i] the
 * link's MTU (the path MTU clamped to nh_mtu, or 500); zeros elsewhere.  For an
 * accepted one, with l = slots[r] = accepted[i] (-1 elsewhere):
 *   - `links` maps link_id[i] to l (rt_linktable_insert's semantics);
 *   - record l of `ks` (64-byte keys, l < rt_keyset_size) is Token(hkdf(64,
 *     X25519(ephemeral[r], data[:32]), salt = link id)), Link.handshake's key
 *     (data[:32] as a 256-bit value mod p, bit 255 not masked, as
 *     X25519PrivateKey.exchange of the internal provider takes it),
 *     where ephemeral (m x 32) is the caller's randomness for
 *     X25519PrivateKey.generate, clamped by the ladder, row r for request r;
 *   - proofs + i*proof_stride (proof_stride >= 118) holds the LRPROOF packet
 *     Link.prove sends and proof_len[i] is 118 (0 elsewhere, row untouched):
 *     0x0F, hops 0, link id, context 0xFF, then signature ‖ pub ‖ signalling
 *     with pub = X25519(ephemeral[r], 9), signalling the three bytes of
 *     Link.signalling_bytes(mtu, mode) and the signature rt_ed25519_sign's of
 *     link id ‖ pub ‖ dest_publics[row] ‖ signalling under dest_seeds[row]
 *     (fixed-base table; constant time in the seed and in ephemeral[r]);
 *   - with sg_peer_publics given (n_links x 32) the signers' rows of l are
 *     filled: sg_peer_publics[l] = data[32:64], sg_flags[l] = the destination's
 *     flags & 3, and, where sg_stride is not 0, sg_seeds / sg_publics at
 *     l*sg_stride = the destination's (sg_stride 0: one shared row, untouched).
 * Neither shared secrets nor derived keys leave the device.  DEVICE pointers;
 * the call only enqueues on the stream (its temporary comes from the context's
 * stream-ordered pool) and takes its place in the host order of `links` and
 * `dests`.  The key records are written in stream order: launches on this
 * stream after the call see them, ordering other streams is the caller's part.
 * n == 0 is RT_OK; n is at most 2^30 - 2. */
#define RT_DEST_ACCEPTS 4u
#define RT_LINKREQ_ACCEPTED        0
#define RT_LINKREQ_NOT_REQUEST     1
#define RT_LINKREQ_OTHER_TRANSPORT 2
#define RT_LINKREQ_NO_DESTINATION  3
#define RT_LINKREQ_NOT_ACCEPTING   4
#define RT_LINKREQ_BAD_SIZE        6
#define RT_LINKREQ_BAD_MODE        7
#define RT_LINKREQ_DUPLICATE       8
#define RT_LINKREQ_NO_SLOT         9
int rt_link_accept(rt_linktable *links, rt_keyset *ks, rt_linktable *dests, const uint8_t *dest_seeds,
                   const uint8_t *dest_publics, const uint8_t *dest_flags, uint32_t n_dests,
                   const uint8_t *transport_identity, int64_t nh_mtu, const uint8_t *pkt, const uint64_t *pkt_off,
                   const rt_packet_fields *fields, uint32_t n, const int32_t *slots, const uint8_t *ephemeral,
                   uint32_t m, uint32_t n_links, uint8_t *sg_seeds, uint8_t *sg_publics, uint64_t sg_stride,
                   uint8_t *sg_peer_publics, uint8_t *sg_flags, int32_t *status, int32_t *accepted, uint8_t *link_id,
                   int32_t *mtu, uint8_t *proofs, uint64_t proof_stride, uint32_t *proof_len, void *stream);
/* Records of an existing key set of 64-byte keys, rewritten on the device:
 * for every item i of n that `mask` selects (mask[i] != 0; mask NULL: all)
 * with rows[i] < rt_keyset_size, record rows[i] becomes Token(hkdf(64,
 * X25519(scalar_i, point_i), salt_i)) (scalars, points, point_off and salt as
 * rt_keyset_create_x25519, one salt row per item in whole aligned words, no
 * context).  The selected rows are distinct.  Enqueued on `stream`, ordered
 * after the key set's build: launches on that stream after the call read the
 * new records, ordering other streams is the caller's part (the link table's
 * rule), and rt_keyset_destroy still frees after it.  The exchange is
 * rt_x25519's: bit 255 of a point is masked, where rt_link_accept takes a
 * peer_pub's 256 bits mod p as they are (X25519PrivateKey.exchange). */
int rt_keyset_set_rows_x25519(rt_keyset *ks, const uint8_t *scalars, uint64_t scalar_stride, const uint8_t *points,
                              uint64_t point_stride, const uint64_t *point_off, const uint8_t *salt,
                              uint64_t salt_stride, uint32_t salt_len, const uint32_t *rows, const uint8_t *mask,
                              uint32_t n, void *stream);

/* ---- link request proofs (Transport.py:2270-2318, Link.py:391-451, 326-333, 348-361) */
/* The initiator side of link establishment: the LRPROOF packets of a read that
 * answer the node's own link requests, over the n records rt_packet_unpack
 * wrote (after rt_packet_filter where there is one, which defers the proofs'
 * hashes to this stage) and before rt_link_spans, so that the read's own
 * packets on a link that comes up find it.
 *
 * The pending links are an rt_linktable from 16-byte link id to a row
 * 0 .. n_rows-1 of per-row arrays in device memory: row_privates (32 B: the
 * link's ephemeral X25519 private key), row_dest_publics (32 B: the
 * destination identity's Ed25519 public key), row_sig_seeds / row_sig_publics
 * (32 B each: the link's own Ed25519 seed and rt_ed25519_public of it),
 * row_flags (one byte, RT_LINK_PROVE_ALL | RT_LINK_HAS_CHANNEL: the new link's
 * signer flags), row_slots (int32: the slot the link takes in `links`, `ks`
 * and the signers; distinct among the pending links, as a free list gives
 * them: rows that share a slot would write one key record), and the link's state, which the call changes: row_hops
 * (int32: Link.expected_hops, compared with the received hop count + 1 as
 * Transport.inbound counts it), row_rebalanced (one byte), row_state (one byte,
 * RT_PENDING_*: Link.PENDING, HANDSHAKE, ACTIVE, CLOSED) and row_mtu (int32).
 * The records are taken as if the packets came one after another in index
 * order.  status[i], the first rule that applies:
 *   RT_LRPROOF_NOT_LRPROOF    fields[i].ok == 0, not a PROOF, or context not
 *                             LRPROOF (0xFF); the destination type is not
 *                             read, as the reference does not read it;
 *   RT_LRPROOF_NO_LINK        the destination hash is not in `pending`;
 *   RT_LRPROOF_NOT_PENDING    the row's state is not PENDING, or a record at a
 *                             lower index of the batch decided the link;
 *   with hops + 1 == row_hops:
 *   RT_LRPROOF_BAD_MODE       data longer than 96 bytes whose mode bits
 *                             (data[96] >> 5) are not AES-256-CBC: the link is
 *                             CLOSED;
 *   RT_LRPROOF_BAD_SIZE       data of neither 96 nor 99 bytes: ignored, the
 *                             link stays PENDING;
 *   RT_LRPROOF_BAD_SIGNATURE  data[:64] is no signature of  link id ‖
 *                             data[64:96] ‖ row_dest_publics ‖ signalling  under
 *                             row_dest_publics, where signalling is nothing (96
 *                             bytes) or Link.signalling_bytes of the 21-bit MTU
 *                             in data[96:99], encoded anew: the link stays in
 *                             HANDSHAKE for good (the reference has derived
 *                             its key by then; the device settles the
 *                             signature first and runs no ladder for it);
 *   RT_LRPROOF_NO_SLOT        the signature holds and row_slots is not below
 *                             rt_keyset_size and n_links, or `links` has no
 *                             room or holds the id: the row stays PENDING;
 *   RT_LRPROOF_ACTIVATED      the link is ACTIVE when the call has run;
 *   with another hop count:
 *   RT_LRPROOF_ACTIVATED      96 or 99 bytes, the right mode, a row that was
 *                             not rebalanced before and a signature that
 *                             holds: row_rebalanced = 1, row_hops = hops + 1,
 *                             then as above (NO_SLOT leaves the row untouched);
 *   RT_LRPROOF_HOPS           anything else: ignored, the link stays PENDING.
 * The lowest index that decides a link (BAD_MODE, BAD_SIGNATURE, NO_SLOT,
 * ACTIVATED) does so whatever the scheduling.  established[i] is the slot of an
 * activated link (-1 elsewhere) and mtu[i] its MTU (the confirmed MTU, or 500;
 * 0 elsewhere), which is also row_mtu.  For an activated link, with l its slot:
 *   - `links` maps the link id to l (rt_linktable_insert's semantics);
 *   - record l of `ks` (64-byte keys) is Token(hkdf(64, X25519(row_privates,
 *     data[64:96]), salt = link id)), Link.handshake's key (data[64:96] as a
 *     256-bit value mod p, bit 255 not masked; constant time in the private key);
 *   - with sg_peer_publics given (n_links x 32) the signers' rows of l are
 *     filled: sg_peer_publics[l] = row_dest_publics, sg_flags[l] = row_flags & 3
 *     and, where sg_stride is not 0, sg_seeds / sg_publics at l*sg_stride = the
 *     row's seed and public key.
 * With `seen` (or NULL) the packet hashes of the records that reached
 * validate_proof are entered into the hash list as rt_hashlist_add does
 * (Transport.py:2314): those whose hop count matched, after the rebalance where
 * one fired, on a link still among the pending ones (not ACTIVE before the
 * record), NO_SLOT excepted so that a proof sent again can bring the link up.
 * The pending table itself is not changed: removing a row (the caller's
 * watchdog, or after reading an ACTIVE state back) is rt_linktable_remove.
 * Nothing private leaves the device.  DEVICE pointers; the call only enqueues
 * on the stream and takes its place in the host order of `pending`, `links` and
 * `seen`; key records are written in stream order.  n == 0 is RT_OK. */
#define RT_PENDING_PENDING   0
#define RT_PENDING_HANDSHAKE 1
#define RT_PENDING_ACTIVE    2
#define RT_PENDING_CLOSED    4
#define RT_LRPROOF_ACTIVATED     0
#define RT_LRPROOF_NOT_LRPROOF   1
#define RT_LRPROOF_NO_LINK       2
#define RT_LRPROOF_NOT_PENDING   3
#define RT_LRPROOF_HOPS          4
#define RT_LRPROOF_BAD_SIZE      6
#define RT_LRPROOF_BAD_MODE      7
#define RT_LRPROOF_BAD_SIGNATURE 8
#define RT_LRPROOF_NO_SLOT       9
int rt_link_establish(rt_linktable *pending, uint32_t n_rows, const uint8_t *row_privates,
                      const uint8_t *row_dest_publics, const uint8_t *row_sig_seeds, const uint8_t *row_sig_publics,
                      const uint8_t *row_flags, const int32_t *row_slots, int32_t *row_hops, uint8_t *row_rebalanced,
                      uint8_t *row_state, int32_t *row_mtu, rt_linktable *links, rt_keyset *ks, uint32_t n_links,
                      const uint8_t *pkt, const uint64_t *pkt_off, const rt_packet_fields *fields, uint32_t n,
                      uint8_t *sg_seeds, uint8_t *sg_publics, uint64_t sg_stride, uint8_t *sg_peer_publics,
                      uint8_t *sg_flags, rt_hashlist *seen, int32_t *status, int32_t *established, int32_t *mtu,
                      void *stream);

/* ---- destination delivery (RNS/Transport.py:2188-2202) -------------------- */
/* The DATA packets of a read that are addressed to the node's own SINGLE
 * destinations: opened as Destination.receive and Identity.decrypt open them
 * (Destination.py:414-429, 622-654; Identity.py:848-898) and, for a PROVE_ALL
 * destination, proved as Packet.prove does (Packet.py:327-336, 376-381;
 * Identity.py:942-953), over the records rt_packet_unpack wrote, each packet
 * read inside pkt + pkt_off[i].  DEVICE pointers; only enqueues.
 *
 * The destinations: `dests` maps the 16-byte destination hash to a row
 * < n_dests; per row the identity's X25519 private key (privates, 32 B), its
 * hash (identity_hashes, 16 B on words: the HKDF salt of Identity.get_salt),
 * its Ed25519 seed and public key (32 B each), a flags byte (RT_LINK_PROVE_ALL
 * | RT_DEST_ENFORCE_RATCHETS; a PROVE_APP or PROVE_NONE destination has no
 * proof flag) and its ratchet private keys ratchets[ratchet_off[row] ..
 * ratchet_off[row + 1]) (32 B each, n_ratchets rows in all), newest first as
 * Destination.ratchets is ordered.
 *
 * Record i: RT_DELIVER_NOT_DATA where fields[i].ok is 0, the packet is no DATA
 * packet or its destination type is LINK; NO_DESTINATION where the hash is not
 * in the table; TYPE_MISMATCH where it is and the packet's destination type is
 * not SINGLE (Transport.py:2194); SHORT for data of 32 bytes or fewer
 * (Identity.py:858).  Otherwise the candidates are the ratchets in order and
 * then the identity's key (left out with ENFORCE_RATCHETS; none at all opens
 * nothing), candidate key = Token(hkdf(64, X25519(candidate, data[:32]),
 * identity hash)) with the exchange X25519PrivateKey.exchange performs (bit
 * 255 of the peer's value counts), and the first candidate whose tag verifies
 * over a well-formed token data[32:] (rt_verify_trials' rule) decrypts it:
 * DELIVERED, or NOT_OPENED where none does or the padding fails under that key.
 * The first pass keys and tries candidate 0 of every such frame in scratch
 * records 0 .. ; the second lays the remaining candidates of the frames still
 * undecided, in stream order, into records max_frames .. max_frames +
 * retry_trials - 1: only whole frames, and a frame that does not fit is
 * DEFERRED with every undecided frame behind it, nothing written for them but
 * deliver_status and destination.
 *
 * For DELIVERED and NOT_OPENED frames status[i] and pt_len[i] are the token
 * decrypt's (RT_ST_*; RT_ST_BAD_HMAC, or TOO_SHORT for a token of 32 bytes or
 * fewer, where no candidate verified) and pt_off[i] = the token's offset +
 * pt_shift (0..16), where the plaintext is written into `pt`; for every other
 * frame the three are left as they are.  destination[i] is the row or -1;
 * ratchet[i] the rank of the ratchet that opened the frame, -1 for the
 * identity's key or for nothing.  A DELIVERED frame of a PROVE_ALL destination
 * has proof_len[i] = 83 (implicit_proof) or 115 and the PROOF packet at proofs
 * + i*proof_stride (>= 115): 0x03, hops 0, packet hash[:16], context 0,
 * [packet hash,] signature; elsewhere proof_len[i] = 0 and the row is not
 * written.  `scratch` is a key set of 64-byte keys with at least max_frames +
 * retry_trials records, `work` 16-byte aligned device memory of
 * rt_destination_deliver_workspace_bytes(max_frames, retry_trials); both are the
 * stage's until the call's work on `stream` has run.  n <= max_frames. */
#define RT_DEST_ENFORCE_RATCHETS 8u
#define RT_DELIVER_DELIVERED      0
#define RT_DELIVER_NOT_DATA       1
#define RT_DELIVER_NO_DESTINATION 2
#define RT_DELIVER_TYPE_MISMATCH  3
#define RT_DELIVER_SHORT          4
#define RT_DELIVER_NOT_OPENED     5
#define RT_DELIVER_DEFERRED       6
uint64_t rt_destination_deliver_workspace_bytes(uint32_t max_frames, uint32_t retry_trials);
int rt_destination_deliver(rt_linktable *dests, uint32_t n_dests, const uint8_t *privates,
                           const uint8_t *identity_hashes, const uint8_t *seeds, const uint8_t *publics,
                           const uint8_t *flags, const uint32_t *ratchet_off, const uint8_t *ratchets,
                           uint32_t n_ratchets, rt_keyset *scratch, uint32_t max_frames, uint32_t retry_trials,
                           void *work, uint64_t work_bytes, const uint8_t *pkt, const uint64_t *pkt_off,
                           const rt_packet_fields *fields, uint32_t n, int implicit_proof, uint32_t pt_shift,
                           uint8_t *pt, uint64_t *pt_off, uint32_t *pt_len, int32_t *status, int32_t *deliver_status,
                           int32_t *destination, int32_t *ratchet, uint8_t *proofs, uint64_t proof_stride,
                           uint32_t *proof_len, void *stream);

/* ---- proofs for packets sent to SINGLE destinations (Transport.py:2326-2363, Packet.py:480-524) */
/* The other end of rt_destination_deliver's proof rows: the PROOF packets of a
 * read that are neither link request proofs nor resource proofs and arrive on
 * no active link, settled against the receipts of the packets this node sent
 * to SINGLE destinations (PacketReceipt.validate_proof), over the records
 * rt_packet_unpack wrote, each proof read inside pkt + pkt_off[i], as if the
 * packets came one after another in index order.  DEVICE pointers; only
 * enqueues.
 *
 * Keyed receipts are a receipt table (above) with two more arrays by id, the
 * caller's: receipt_keys (max_receipts x 32 bytes), the Ed25519 public key of
 * the identity the packet went to (Identity.get_public_key()[32:64]), and
 * receipt_keyed (max_receipts bytes), 0 for a receipt without an identity (one
 * sent on a link), which no proof of this kind delivers.  Adding receipts is
 * rt_linktable_insert (packet hash[:16], id) followed by rt_receipt_store_keyed
 * over the same batch and the status the insert wrote: hash, key (keys n x 32,
 * or NULL: keyed 0) and keyed are written where status[i] is RT_LINK_OK and
 * ids[i] < max_receipts, so a duplicate leaves the earlier entry untouched.
 *
 * dproof_status[i], the first rule that applies:
 *   RT_DPROOF_NOT_PROOF      fields[i].ok == 0, not a PROOF, or context LRPROOF
 *                            (0xFF) or RESOURCE_PRF (0x05);
 *   RT_DPROOF_ON_LINK        destination type LINK and link[i] in 0 .. n_links-1:
 *                            rt_proof_settle's business.  link NULL: no link is
 *                            active and this never applies;
 *   RT_DPROOF_BAD_LENGTH     data of neither 64 nor 96 bytes;
 *   RT_DPROOF_NO_RECEIPT     explicit (96): no keyed receipt holds data[:32],
 *                            compared in full, or a lower index of the batch
 *                            delivered it.  Implicit (64): every keyed receipt
 *                            was tried and none validated, or the one that
 *                            would have was delivered to a lower index;
 *   RT_DPROOF_BAD_SIGNATURE  explicit only: the receipt is there and data[32:96]
 *                            is not its key's signature of its hash, as
 *                            rt_ed25519_verify judges;
 *   RT_DPROOF_DEFERRED       implicit: the proof had to be tried against the
 *                            whole table and its frame did not fit scan_trials;
 *                            nothing else is written for it;
 *   RT_DPROOF_DELIVERED      receipt[i] is the receipt's id and the entry has
 *                            left the table inside the call.
 * receipt[i] is -1 for every other status.  An implicit proof is first tried
 * against the keyed receipt at its own destination hash (an honest proof is
 * addressed to hash[:16] of the packet it proves): one verification.  The
 * proofs that fail there or find no keyed receipt there, the strays, are
 * ranked in index order, and stray r is tried against all L live keyed
 * receipts when (r + 1) * L <= scan_trials: only whole frames, and every stray
 * behind the first that does not fit is DEFERRED.  With L = 0 every stray is
 * NO_RECEIPT.  The lowest index that validates a receipt is delivered whatever
 * the scheduling.  `work` is 16-byte aligned device memory of
 * rt_destination_proof_workspace_bytes(n, max_receipts), the stage's until the
 * call's work on `stream` has run. */
#define RT_DPROOF_DELIVERED     0
#define RT_DPROOF_NOT_PROOF     1
#define RT_DPROOF_ON_LINK       2
#define RT_DPROOF_BAD_LENGTH    3
#define RT_DPROOF_NO_RECEIPT    4
#define RT_DPROOF_BAD_SIGNATURE 5
#define RT_DPROOF_DEFERRED      6
uint64_t rt_destination_proof_workspace_bytes(uint32_t n, uint32_t max_receipts);
int rt_receipt_store_keyed(rt_linktable *receipts, uint8_t *receipt_hashes, uint8_t *receipt_keys,
                           uint8_t *receipt_keyed, uint32_t max_receipts, const uint8_t *hashes, const uint8_t *keys,
                           const uint32_t *ids, const int32_t *status, uint32_t n, void *stream);
int rt_destination_proof_settle(rt_linktable *receipts, const uint8_t *receipt_hashes, const uint8_t *receipt_keys,
                                const uint8_t *receipt_keyed, uint32_t max_receipts, uint32_t scan_trials, void *work,
                                uint64_t work_bytes, const uint8_t *pkt, const uint64_t *pkt_off,
                                const rt_packet_fields *fields, const int32_t *link, uint32_t n_links,
                                int32_t *dproof_status, int32_t *receipt, uint32_t n, void *stream);

/* ---- the replies of a read (Transport.py:1069-1104, 1199-1356; Identity.py:942-953; Link.py:366-389) */
/* The stages of the inbound path leave what the node has to send as sparse
 * rows, one per frame with a length column: the LRPROOFs of rt_link_accept, the
 * LINK PROOFs of rt_link_prove, the PROOFs of rt_destination_deliver.  The
 * reference transmits each of them on the interface its frame came in on, in
 * the order of its loop over the frames, so one read has one reply stream.
 *
 * rt_reply_gather makes the dense batch.  There are n_sources (1..4) sources
 * over the same n frames (at most 2^31 - 1); rows, row_stride, row_width and
 * len are HOST arrays of n_sources entries.  Source s holds for frame k the
 * len[s][k] bytes at rows[s] + k * row_stride[s] (rows[s], len[s]: DEVICE
 * pointers; any alignment; row_width[s] <= row_stride[s] is the bytes a row
 * holds).  A length of 0 means nothing for that frame, and so does any length
 * outside 1 .. min(128, row_width[s]); no byte at or past a row's length is
 * read.  The replies are ordered by frame, then by source index, and every
 * non-zero source of a frame is one reply.  Reply j < written goes to
 * out + 128 j (out: cap x 128 bytes, 128-byte aligned; the row's bytes past the
 * reply are zeroed) with reply_len[j], reply_frame[j] (k) and reply_source[j]
 * (s); reply_counts (device int64[2]) = [written = min(found, cap), found].
 * Entries written .. cap-1 get reply_len 0, reply_frame -1 and reply_source
 * 0xFF, and their rows are not written.  n = 0 and cap = 0 are valid.  The
 * outputs must not overlap the sources.  `workspace` of
 * rt_reply_gather_workspace_bytes(n, n_sources) bytes (0 for arguments the call
 * refuses), 8-byte aligned.
 *
 * The batch then goes through rt_ifac_sign and rt_ifac_mask where the interface
 * has access codes, with pkt_off[j] = 128 j (entries past `written` have length
 * 0 and an offset inside the buffer, which is what those calls need), and
 * through rt_hdlc_frame_counted with n_dev = reply_counts.
 *
 * rt_reply_remember enters the packet hashes of the first
 * min(reply_counts[0], cap) rows (row j at rows + j * row_stride, row_stride >=
 * 128; the unmasked packets, as rt_reply_gather wrote them) into the hash
 * list's current generation, as Transport.outbound does for what it broadcasts
 * (Transport.py:1343-1345, add_packet_hash) and as rt_hashlist_add does: the
 * node then drops its own reply when a shared medium echoes it.  The hash is
 * rt_packet_unpack's; a row too short to be a packet is left out.  The call
 * takes its place in the list's host order. */
#define RT_REPLY_LRPROOF    0   /* the source order of the inbound path's stages */
#define RT_REPLY_LINK_PROOF 1
#define RT_REPLY_DEST_PROOF 2
uint64_t rt_reply_gather_workspace_bytes(uint32_t n, uint32_t n_sources);
int rt_reply_gather(rt_ctx *ctx, uint32_t n_sources, const uint8_t *const *rows, const uint64_t *row_stride,
                    const uint32_t *row_width, const int32_t *const *len, uint32_t n, uint8_t *out, int32_t *reply_len,
                    int32_t *reply_frame, uint8_t *reply_source, int64_t *reply_counts, uint32_t cap, void *workspace,
                    void *stream);
int rt_reply_remember(rt_hashlist *list, const uint8_t *rows, uint64_t row_stride, const int32_t *reply_len,
                      const int64_t *reply_counts, uint32_t cap, void *stream);

/* ---- memory helpers (so a non-torch host can drive the device API) ------- */
/* rt_memcpy_d2h: a pinned (page-locked, mapped) destination, e.g. from
 * rt_host_alloc, is written by GPU stores into the mapped buffer on `stream`
 * (faster than the copy engine's device-to-host path on MI355X, and it
 * shares the link with a copy-engine H2D); a pageable one is copied with
 * hipMemcpyAsync.  Either way `dst` is valid once `stream` has run. */
void *rt_device_alloc(rt_ctx *ctx, uint64_t bytes);
void  rt_device_free(rt_ctx *ctx, void *p);
void *rt_host_alloc(uint64_t bytes);            /* pinned */
void  rt_host_free(void *p);
int   rt_memcpy_h2d(rt_ctx *ctx, void *dst, const void *src, uint64_t bytes, void *stream);
int   rt_memcpy_d2h(rt_ctx *ctx, void *dst, const void *src, uint64_t bytes, void *stream);
/* rt_memcpy_d2h_upto: min(max_bytes, *d_bytes) bytes, the count read on the
 * device at run time (d_bytes: a DEVICE 64-bit count on the context's GPU,
 * e.g. frame_off[n] of rt_hdlc_frame, a size the host does not know without
 * a sync; read as signed, so zero or negative copies nothing), as GPU stores
 * into a pinned `dst` (RT_E_INVAL for any other destination); bytes of `dst`
 * past the count are not written. */
int   rt_memcpy_d2h_upto(rt_ctx *ctx, void *dst, const void *src, uint64_t max_bytes, const uint64_t *d_bytes,
                         void *stream);
int   rt_stream_sync(rt_ctx *ctx, void *stream);

/* ---- launch clock (measurement; no reference counterpart) ----------------
 * rt_clock_stamps: from the next launch on, every workgroup of the context's
 * encrypt and decrypt kernels (the one-packet-per-lane, split and long-token
 * kernels of rt_encrypt* / rt_decrypt*) adds its span to `acc`, a DEVICE buffer of
 * RT_CLOCK_WORDS uint64 on the context's GPU (null: stop stamping).  Words
 * [4k .. 4k+3], k = RT_CLOCK_ENCRYPT / RT_CLOCK_DECRYPT: the sum of the
 * workgroups' spans in shader clock cycles, the same spans in 100 MHz
 * real-time ticks, the number of workgroups stamped, the number of launches.
 * The run's sustained shader clock is words[0] / words[1] x 100 MHz and the
 * cycles per launch words[0] / words[2] (one persistent workgroup per CU).
 * The caller zeroes `acc` and reads it after the stamped launches complete. */
#define RT_CLOCK_WORDS 8
#define RT_CLOCK_ENCRYPT 0
#define RT_CLOCK_DECRYPT 1
int   rt_clock_stamps(rt_ctx *ctx, uint64_t *acc);

#ifdef __cplusplus
}
#endif
#endif /* RNSTOK_H */

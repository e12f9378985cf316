// capi_wire.hip — the wire path of the C-ABI: HDLC framing and deframing,
// frame compaction, IFAC, packet headers, and the Resource hashmap, integrity
// hash and proof.  Device pointers on the caller's stream; the two *_host
// calls go through a staging lane (capi_internal.h).
#include "capi_internal.h"

extern "C" {

// ------------------------------------------------------------------ wire --

static_assert(sizeof(rt_packet_fields) == 96, "rt_packet_fields layout");

uint64_t rt_hdlc_frame_workspace_bytes(uint32_t n) { return hdlc_frame_workspace_bytes(n); }
uint64_t rt_hdlc_deframe_workspace_bytes(uint64_t len) { return hdlc_deframe_workspace_bytes(len); }

int rt_hdlc_frame(rt_ctx *c, const uint8_t *pkt, const uint64_t *pkt_off, const uint32_t *pkt_len, uint32_t n,
                  uint8_t *out, uint64_t *frame_off, void *workspace, void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (!frame_off) return fail(RT_E_INVAL, "rt_hdlc_frame: null frame_off");
    if (n == 0) return RT_OK;
    if (!pkt || !pkt_off || !pkt_len || !out || !workspace) return fail(RT_E_INVAL, "rt_hdlc_frame: null buffer");
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    RT_HIP(launch_hdlc_frame(pkt, pkt_off, pkt_len, n, out, frame_off, workspace, as_stream(stream)), "hdlc frame");
    return RT_OK;
}

static int deframe_common(rt_ctx *c, const uint8_t *buf, uint64_t len, uint32_t hw_mtu, uint32_t ifac_size,
                          uint8_t *out, uint64_t *frame_off, uint32_t *frame_len, int32_t *status, uint64_t *counts,
                          uint64_t max_pairs, void *workspace, void *stream, uint32_t line_phase) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (!counts || !workspace) return fail(RT_E_INVAL, "rt_hdlc_deframe: null counts/workspace");
    if (len && (!buf || !out)) return fail(RT_E_INVAL, "rt_hdlc_deframe: null buffer");
    if (max_pairs && (!frame_off || !frame_len || !status)) return fail(RT_E_INVAL, "rt_hdlc_deframe: null frame arrays");
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    RT_HIP(launch_hdlc_deframe(buf, len, hw_mtu, ifac_size, out, frame_off, frame_len, status, counts, max_pairs,
                               workspace, as_stream(stream), line_phase),
           "hdlc deframe");
    return RT_OK;
}

int rt_hdlc_deframe(rt_ctx *c, const uint8_t *buf, uint64_t len, uint32_t hw_mtu, uint32_t ifac_size, uint8_t *out,
                    uint64_t *frame_off, uint32_t *frame_len, int32_t *status, uint64_t *counts, uint64_t max_pairs,
                    void *workspace, void *stream) {
    return deframe_common(c, buf, len, hw_mtu, ifac_size, out, frame_off, frame_len, status, counts, max_pairs,
                          workspace, stream, 0xFFFFFFFFu);
}

int rt_hdlc_deframe_slots(rt_ctx *c, const uint8_t *buf, uint64_t len, uint32_t hw_mtu, uint32_t ifac_size,
                          uint32_t line_phase, uint8_t *out, uint64_t *frame_off, uint32_t *frame_len, int32_t *status,
                          uint64_t *counts, uint64_t max_pairs, void *workspace, void *stream) {
    if (line_phase >= 128u) return fail(RT_E_INVAL, "rt_hdlc_deframe_slots: line_phase must be < 128");
    return deframe_common(c, buf, len, hw_mtu, ifac_size, out, frame_off, frame_len, status, counts, max_pairs,
                          workspace, stream, line_phase);
}

static bool overlaps(const void *a, const void *b, uint64_t a_bytes, uint64_t b_bytes = 0) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (b_bytes ? b_bytes : a_bytes) && y < x + a_bytes;
}

uint64_t rt_frames_compact_workspace_bytes(uint64_t max_pairs) { return frames_compact_workspace_bytes(max_pairs); }

int rt_frames_compact(rt_ctx *c, const uint64_t *frame_off, const uint32_t *frame_len, const int32_t *status,
                      const uint64_t *counts, uint64_t max_pairs, uint64_t *f_off, uint32_t *f_len,
                      int64_t *frame_pair, int64_t *n_frames, void *workspace, void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (!counts || !n_frames) return fail(RT_E_INVAL, "rt_frames_compact: null counts/n_frames");
    if (max_pairs && (!frame_off || !frame_len || !status || !f_off || !f_len || !frame_pair || !workspace))
        return fail(RT_E_INVAL, "rt_frames_compact: null buffer");
    // k_compact_write reads frame_off[k] / frame_len[k] while other threads
    // write f_off[r] / f_len[r] for r <= k: in-place compaction would race
    if (max_pairs && (overlaps(f_off, frame_off, 8 * max_pairs) || overlaps(f_len, frame_len, 4 * max_pairs) ||
                      overlaps(f_off, frame_len, 8 * max_pairs, 4 * max_pairs) ||
                      overlaps(f_len, frame_off, 4 * max_pairs, 8 * max_pairs)))
        return fail(RT_E_INVAL, "rt_frames_compact: outputs must not overlap the frame arrays");
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    RT_HIP(launch_frames_compact(frame_off, frame_len, status, counts, max_pairs, f_off, f_len, frame_pair, n_frames,
                                 workspace, as_stream(stream)),
           "frames compact");
    return RT_OK;
}

int rt_ifac_mask(rt_ctx *c, const uint8_t *pkt, const uint64_t *pkt_off, const uint32_t *pkt_len, const uint8_t *ifac,
                 uint32_t ifac_size, const uint8_t *ifac_key, uint32_t key_len, uint8_t *out, const uint64_t *out_off,
                 uint32_t n, void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (key_len > 64) return fail(RT_E_INVAL, "rt_ifac_mask: ifac_key longer than 64 bytes");
    if (ifac_size == 0 || ifac_size > 64) return fail(RT_E_INVAL, "rt_ifac_mask: ifac_size must be 1..64");
    if (n == 0) return RT_OK;
    if (!pkt || !pkt_off || !pkt_len || !ifac || !out || !out_off || (key_len && !ifac_key))
        return fail(RT_E_INVAL, "rt_ifac_mask: null buffer");
    IfacArgs a{pkt, pkt_off, pkt_len, const_cast<uint8_t *>(ifac), ifac_size, ifac_key, key_len, out, out_off,
               nullptr, nullptr, n};
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    RT_HIP(launch_ifac(a, true, as_stream(stream)), "ifac mask");
    return RT_OK;
}

int rt_ifac_unmask(rt_ctx *c, const uint8_t *pkt, const uint64_t *pkt_off, const uint32_t *pkt_len, uint32_t ifac_size,
                   const uint8_t *ifac_key, uint32_t key_len, uint8_t *ifac_out, uint8_t *out, const uint64_t *out_off,
                   int32_t *status, uint32_t *out_len, uint32_t n, void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (key_len > 64) return fail(RT_E_INVAL, "rt_ifac_unmask: ifac_key longer than 64 bytes");
    if (ifac_size == 0 || ifac_size > 64) return fail(RT_E_INVAL, "rt_ifac_unmask: ifac_size must be 1..64");
    if (n == 0) return RT_OK;
    if (!pkt || !pkt_off || !pkt_len || !ifac_out || !out || !out_off || !status || (key_len && !ifac_key))
        return fail(RT_E_INVAL, "rt_ifac_unmask: null buffer");
    IfacArgs a{pkt, pkt_off, pkt_len, ifac_out, ifac_size, ifac_key, key_len, out, out_off, status, out_len, n};
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    RT_HIP(launch_ifac(a, false, as_stream(stream)), "ifac unmask");
    return RT_OK;
}

int rt_packet_unpack(rt_ctx *c, const uint8_t *pkt, const uint64_t *pkt_off, const uint32_t *pkt_len,
                     rt_packet_fields *fields, uint32_t n, void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (n == 0) return RT_OK;
    if (!pkt || !pkt_off || !pkt_len || !fields) return fail(RT_E_INVAL, "rt_packet_unpack: null buffer");
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    RT_HIP(launch_unpack(pkt, pkt_off, pkt_len, fields, n, as_stream(stream)), "packet unpack");
    return RT_OK;
}

int rt_token_spans(rt_ctx *c, const rt_packet_fields *fields, const uint64_t *pkt_off, uint32_t n, uint64_t *tok_off,
                   uint32_t *tok_len, void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (n == 0) return RT_OK;
    if (!fields || !pkt_off || !tok_off || !tok_len) return fail(RT_E_INVAL, "rt_token_spans: null buffer");
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    RT_HIP(launch_token_spans(fields, pkt_off, n, tok_off, tok_len, as_stream(stream)), "token spans");
    return RT_OK;
}

int rt_packet_pack_headers(rt_ctx *c, const uint8_t *flags, const uint8_t *hops, const uint8_t *transport_id,
                           const uint8_t *destination_hash, const uint8_t *context, uint8_t *out,
                           const uint64_t *out_off, uint32_t n, void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (n == 0) return RT_OK;
    if (!flags || !destination_hash || !context || !out || !out_off)
        return fail(RT_E_INVAL, "rt_packet_pack_headers: null buffer");
    PackArgs a{flags, hops, context, destination_hash, transport_id, out, out_off, n};
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    RT_HIP(launch_pack_headers(a, as_stream(stream)), "pack headers");
    return RT_OK;
}

// --------------------------------------------------------- Resource hashmap --

int rt_map_hashes(rt_ctx *c, const uint8_t *data, const uint64_t *part_off, const uint32_t *part_len, uint64_t size,
                  uint32_t sdu, const uint8_t *salts, uint32_t salt_len, const uint32_t *part_res, uint32_t n_res,
                  uint32_t guard, uint8_t *map_hashes, uint32_t *first_collision, uint32_t n_parts, void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (n_parts == 0) return RT_OK;
    if (!data || !map_hashes) return fail(RT_E_INVAL, "rt_map_hashes: null data or output");
    if ((part_off == nullptr) != (part_len == nullptr))
        return fail(RT_E_INVAL, "rt_map_hashes: part_off and part_len go together");
    if (!part_off) {
        if (sdu == 0 || (size + sdu - 1) / sdu != n_parts)
            return fail(RT_E_INVAL, "rt_map_hashes: n_parts must be ceil(size / sdu)");
        if (part_res) return fail(RT_E_INVAL, "rt_map_hashes: uniform segmentation is one resource");
    }
    if (salt_len && !salts) return fail(RT_E_INVAL, "rt_map_hashes: null salts");
    if (n_res == 0) n_res = 1;
    MapArgs m{};
    m.data = data; m.part_off = part_off; m.part_len = part_len; m.size = size; m.sdu = sdu;
    m.salts = salts; m.salt_len = salts ? salt_len : 0; m.part_res = part_res; m.n_res = n_res; m.guard = guard;
    m.out = map_hashes; m.first_collision = first_collision; m.n_parts = n_parts;
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    RT_HIP(launch_map_hashes(m, as_stream(stream)), "map hash launch");
    return RT_OK;
}

int rt_resource_hashmap_host(rt_ctx *c, const uint8_t *data, uint64_t size, uint32_t sdu, const uint8_t *random_hash,
                             uint32_t rh_len, uint32_t guard, uint8_t *hashmap, uint32_t *first_collision) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (sdu == 0) return fail(RT_E_INVAL, "rt_resource_hashmap_host: sdu must be > 0");
    const uint64_t parts = (size + sdu - 1) / sdu;
    if (parts > 0xffffffffull) return fail(RT_E_INVAL, "rt_resource_hashmap_host: too many parts");
    if (first_collision) *first_collision = 0xffffffffu;
    if (parts == 0) return RT_OK;
    if (!data || !hashmap || (rh_len && !random_hash)) return fail(RT_E_INVAL, "rt_resource_hashmap_host: null buffer");
    HostCall hc(c, HostCall::PER_ARRAY);
    const uint64_t o_data = hc.add(size), o_salt = hc.add(rh_len), o_out = hc.add(4 * parts), o_col = hc.add(4);
    RT_TRY(hc.open());
    hc.put(o_data, data, size, "H2D data");
    hc.put(o_salt, random_hash, rh_len, "H2D salt");
    RT_TRY(hc.send());
    MapArgs m{};
    m.data = hc.dev<uint8_t>(o_data); m.size = size; m.sdu = sdu; m.salts = hc.dev<uint8_t>(o_salt);
    m.salt_len = rh_len; m.n_res = 1; m.guard = guard; m.out = hc.dev<uint8_t>(o_out);
    m.first_collision = hc.dev<uint32_t>(o_col); m.n_parts = (uint32_t)parts;
    RT_HIP(launch_map_hashes(m, hc.stream()), "map hash launch");
    uint32_t col = 0xffffffffu;
    hc.get(hashmap, o_out, 4 * parts, "D2H hashmap");
    hc.get(&col, o_col, 4, "D2H collision");
    RT_TRY(hc.finish());
    if (first_collision) *first_collision = col;
    return RT_OK;
}

// ------------------------------------------- Resource hash and proof --

uint32_t rt_resource_hash_split_below(void) { return resource_hash_split_below(); }

int rt_resource_hashes(rt_ctx *c, const uint8_t *data, const uint64_t *seg_off, const uint32_t *seg_len,
                       const uint8_t *random_hashes, uint32_t rh_len, const uint8_t *expect_hash, uint8_t *hash,
                       uint8_t *proof, int32_t *status, uint32_t n, void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (n == 0) return RT_OK;
    if (!data || !seg_off || !seg_len || !hash)
        return fail(RT_E_INVAL, "rt_resource_hashes: null data, segments or output");
    if (rh_len > 32) return fail(RT_E_INVAL, "rt_resource_hashes: rh_len must be <= 32");
    if (rh_len && !random_hashes) return fail(RT_E_INVAL, "rt_resource_hashes: null random_hashes");
    if (expect_hash && !status) return fail(RT_E_INVAL, "rt_resource_hashes: expect_hash needs status");
    ResHashArgs a{data, seg_off, seg_len, random_hashes, rh_len, expect_hash, hash, proof, status, n};
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    RT_HIP(launch_resource_hashes(a, as_stream(stream)), "resource hash launch");
    return RT_OK;
}

int rt_resource_hashes_host(rt_ctx *c, const uint8_t *data, uint64_t size, const uint8_t *random_hash,
                            uint32_t rh_len, const uint8_t *expect_hash, uint8_t *hash, uint8_t *proof,
                            int32_t *status) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (size > 0xffffffffull) return fail(RT_E_INVAL, "rt_resource_hashes_host: segment too large");
    if ((size && !data) || !hash || (rh_len && !random_hash))
        return fail(RT_E_INVAL, "rt_resource_hashes_host: null buffer");
    if (rh_len > 32) return fail(RT_E_INVAL, "rt_resource_hashes_host: rh_len must be <= 32");
    if (expect_hash && !status) return fail(RT_E_INVAL, "rt_resource_hashes_host: expect_hash needs status");
    HostCall hc(c, HostCall::PER_ARRAY);
    // hash, proof and status come back as one 80-byte region
    const uint64_t o_data = hc.add(size), o_rh = hc.add(32), o_exp = hc.add(32), o_seg = hc.add(16), o_out = hc.add(80);
    RT_TRY(hc.open());
    struct { uint64_t off; uint32_t len, pad; } seg = {o_data, (uint32_t)size, 0u};
    hc.put(o_data, data, size, "H2D data");
    hc.put(o_rh, random_hash, rh_len, "H2D random_hash");
    if (expect_hash) hc.put(o_exp, expect_hash, 32, "H2D expect_hash");
    hc.put(o_seg, &seg, 16, "H2D segment");
    RT_TRY(hc.send());
    uint8_t *out = hc.dev<uint8_t>(o_out);
    ResHashArgs a{hc.dev<uint8_t>(0), hc.dev<uint64_t>(o_seg), hc.dev<uint32_t>(o_seg + 8), hc.dev<uint8_t>(o_rh), rh_len,
                  expect_hash ? hc.dev<uint8_t>(o_exp) : nullptr, out, proof ? out + 32 : nullptr,
                  (int32_t *)(out + 64), 1u};
    RT_HIP(launch_resource_hashes(a, hc.stream()), "resource hash launch");
    uint8_t back[80];
    hc.get(back, o_out, 80, "D2H digests");
    RT_TRY(hc.finish());
    memcpy(hash, back, 32);
    if (proof) memcpy(proof, back + 32, 32);
    if (status) memcpy(status, back + 64, 4);
    return RT_OK;
}

}  // extern "C"

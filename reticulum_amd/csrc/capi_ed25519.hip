// capi_ed25519.hip — Ed25519 in the C-ABI: verify, sign and public keys in
// batches (ed25519_kernels.hip).  Device pointers on the caller's stream; the
// *_host calls go through a staging lane (capi_internal.h).
#include "capi_internal.h"

namespace {

int key_stride_check(uint64_t stride, const char *msg) {
    return stride && stride < 32 ? fail(RT_E_INVAL, msg) : RT_OK;
}

int msgs_check(const char *fn, const uint64_t *msg_off, const uint32_t *msg_len) {
    if (!msg_off || !msg_len) return fail(RT_E_INVAL, std::string(fn) + ": null message offsets or lengths");
    return RT_OK;
}

int verify_check(rt_ctx *c, const uint8_t *pubs, uint64_t pub_stride, const uint8_t *sigs, uint64_t sig_stride,
                 const uint64_t *msg_off, const uint32_t *msg_len, const uint8_t *ok, uint32_t n) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (n == 0) return RT_OK;
    if (!pubs || !sigs || !ok) return fail(RT_E_INVAL, "rt_ed25519_verify: null keys, signatures or output");
    RT_TRY(msgs_check("rt_ed25519_verify", msg_off, msg_len));
    RT_TRY(key_stride_check(pub_stride, "rt_ed25519_verify: pub_stride is 0 (one key for all) or at least 32"));
    if (sig_stride < 64 && n > 1) return fail(RT_E_INVAL, "rt_ed25519_verify: sig_stride smaller than 64");
    return RT_OK;
}

int sign_check(rt_ctx *c, const uint8_t *seeds, uint64_t seed_stride, const uint8_t *pubs, uint64_t pub_stride,
               const uint64_t *msg_off, const uint32_t *msg_len, const uint8_t *out, uint64_t out_stride, uint32_t n) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (n == 0) return RT_OK;
    if (!seeds || !out) return fail(RT_E_INVAL, "rt_ed25519_sign: null seeds or output");
    RT_TRY(msgs_check("rt_ed25519_sign", msg_off, msg_len));
    RT_TRY(key_stride_check(seed_stride, "rt_ed25519_sign: seed_stride is 0 (one seed for all) or at least 32"));
    if (pubs) RT_TRY(key_stride_check(pub_stride, "rt_ed25519_sign: pub_stride is 0 (one key for all) or at least 32"));
    if (out_stride < 64 && n > 1) return fail(RT_E_INVAL, "rt_ed25519_sign: out_stride smaller than 64");
    return RT_OK;
}

int public_check(rt_ctx *c, const uint8_t *seeds, uint64_t seed_stride, const uint8_t *out, uint64_t out_stride,
                 uint32_t n) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (n == 0) return RT_OK;
    if (!seeds || !out) return fail(RT_E_INVAL, "rt_ed25519_public: null seeds or output");
    RT_TRY(key_stride_check(seed_stride, "rt_ed25519_public: seed_stride is 0 (one seed for all) or at least 32"));
    if (out_stride < 32 && n > 1) return fail(RT_E_INVAL, "rt_ed25519_public: out_stride smaller than 32");
    return RT_OK;
}

int ifac_sign_check(const char *fn, rt_ctx *c, const uint8_t *seed, const uint8_t *pub, const uint8_t *pkt,
                    const uint64_t *pkt_off, const uint32_t *pkt_len, const uint8_t *ifac, uint32_t ifac_size,
                    uint32_t n) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (ifac_size < 1 || ifac_size > 64) return fail(RT_E_INVAL, std::string(fn) + ": ifac_size outside 1..64");
    if (n == 0) return RT_OK;
    if (!seed || !pub) return fail(RT_E_INVAL, std::string(fn) + ": null seed or public key");
    if (!pkt || !pkt_off || !pkt_len) return fail(RT_E_INVAL, std::string(fn) + ": null packets, offsets or lengths");
    if (!ifac) return fail(RT_E_INVAL, std::string(fn) + ": null access codes");
    return RT_OK;
}

// The messages of a host call: the bytes [0, extent) of msgs that the n spans
// cover, with their offsets and lengths, staged next to each other.
struct HostMsgs {
    uint64_t extent = 0, o_msgs = 0, o_off = 0, o_len = 0;
    int plan(HostCall &hc, const char *fn, const uint8_t *msgs, const uint64_t *msg_off, const uint32_t *msg_len,
             uint32_t n) {
        for (uint32_t i = 0; i < n; ++i) {
            if (!msg_len[i]) continue;
            if (!msgs) return fail(RT_E_INVAL, std::string(fn) + ": null messages with a non-zero length");
            extent = std::max(extent, msg_off[i] + msg_len[i]);
        }
        o_msgs = hc.add(extent);
        o_off = hc.add(8ull * n);
        o_len = hc.add(4ull * n);
        return RT_OK;
    }
    void put(HostCall &hc, const uint8_t *msgs, const uint64_t *msg_off, const uint32_t *msg_len, uint32_t n) const {
        hc.put(o_msgs, msgs, extent, "H2D messages");
        hc.put(o_off, msg_off, 8ull * n, "H2D message offsets");
        hc.put(o_len, msg_len, 4ull * n, "H2D message lengths");
    }
};

}  // namespace

extern "C" {

int rt_ed25519_verify(rt_ctx *c, const uint8_t *pubs, uint64_t pub_stride, const uint8_t *sigs, uint64_t sig_stride,
                      const uint8_t *msgs, const uint64_t *msg_off, const uint32_t *msg_len, uint8_t *ok, uint32_t n,
                      void *stream) {
    int rc = verify_check(c, pubs, pub_stride, sigs, sig_stride, msg_off, msg_len, ok, n);
    if (rc || n == 0) return rc;
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    // msgs == NULL: the lengths live on the device and cannot be checked here;
    // the kernel then takes every message as empty and reads no length
    const Ed25519VerifyArgs a{pubs, pub_stride, sigs, sig_stride, msgs, msg_off, msg_len, ok, n};
    RT_HIP(launch_ed25519_verify(a, as_stream(stream)), "ed25519 verify launch");
    return RT_OK;
}

int rt_ed25519_verify_host(rt_ctx *c, const uint8_t *pubs, uint64_t pub_stride, const uint8_t *sigs,
                           uint64_t sig_stride, const uint8_t *msgs, const uint64_t *msg_off, const uint32_t *msg_len,
                           uint8_t *ok, uint32_t n) {
    int rc = verify_check(c, pubs, pub_stride, sigs, sig_stride, msg_off, msg_len, ok, n);
    if (rc || n == 0) return rc;
    // packed rows on the device: keys (n or 1) x 32, signatures n x 64, the messages, ok n
    const uint64_t n_pk = pub_stride ? n : 1u;
    HostCall hc(c, HostCall::PER_ARRAY);
    HostMsgs m;
    RT_TRY(m.plan(hc, "rt_ed25519_verify_host", msgs, msg_off, msg_len, n));
    const uint64_t o_pk = hc.add(32 * n_pk), o_sig = hc.add(64ull * n), o_ok = hc.add(n);
    RT_TRY(hc.open());
    m.put(hc, msgs, msg_off, msg_len, n);
    hc.put_rows(o_pk, pubs, pub_stride ? pub_stride : 32, 32, n_pk, "H2D keys");
    hc.put_rows(o_sig, sigs, sig_stride < 64 ? 64 : sig_stride, 64, n, "H2D signatures");
    RT_TRY(hc.send());
    const Ed25519VerifyArgs a{hc.dev<uint8_t>(o_pk), pub_stride ? 32u : 0u, hc.dev<uint8_t>(o_sig), 64,
                              m.extent ? hc.dev<uint8_t>(m.o_msgs) : nullptr, hc.dev<uint64_t>(m.o_off),
                              hc.dev<uint32_t>(m.o_len), hc.dev<uint8_t>(o_ok), n};
    RT_HIP(launch_ed25519_verify(a, hc.stream()), "ed25519 verify launch");
    hc.get(ok, o_ok, n, "D2H ok");
    return hc.finish();
}

int rt_ed25519_sign(rt_ctx *c, const uint8_t *seeds, uint64_t seed_stride, const uint8_t *pubs, uint64_t pub_stride,
                    const uint8_t *msgs, const uint64_t *msg_off, const uint32_t *msg_len, uint8_t *sigs_out,
                    uint64_t out_stride, uint32_t n, void *stream) {
    int rc = sign_check(c, seeds, seed_stride, pubs, pub_stride, msg_off, msg_len, sigs_out, out_stride, n);
    if (rc || n == 0) return rc;
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    const Ed25519SignArgs a{seeds, seed_stride, pubs, pub_stride, msgs, msg_off, msg_len, sigs_out, out_stride, n};
    RT_HIP(launch_ed25519_sign(a, as_stream(stream)), "ed25519 sign launch");
    return RT_OK;
}

int rt_ed25519_sign_host(rt_ctx *c, const uint8_t *seeds, uint64_t seed_stride, const uint8_t *pubs,
                         uint64_t pub_stride, const uint8_t *msgs, const uint64_t *msg_off, const uint32_t *msg_len,
                         uint8_t *sigs_out, uint64_t out_stride, uint32_t n) {
    int rc = sign_check(c, seeds, seed_stride, pubs, pub_stride, msg_off, msg_len, sigs_out, out_stride, n);
    if (rc || n == 0) return rc;
    const uint64_t n_seed = seed_stride ? n : 1u, n_pk = !pubs ? 0u : pub_stride ? n : 1u;
    HostCall hc(c, HostCall::PER_ARRAY);
    HostMsgs m;
    RT_TRY(m.plan(hc, "rt_ed25519_sign_host", msgs, msg_off, msg_len, n));
    const uint64_t o_seed = hc.add(32 * n_seed), o_pk = hc.add(32 * n_pk), o_out = hc.add(64ull * n);
    RT_TRY(hc.open());
    m.put(hc, msgs, msg_off, msg_len, n);
    hc.put_rows(o_seed, seeds, seed_stride ? seed_stride : 32, 32, n_seed, "H2D seeds");
    hc.put_rows(o_pk, pubs, pub_stride ? pub_stride : 32, 32, n_pk, "H2D keys");
    RT_TRY(hc.send());
    const Ed25519SignArgs a{hc.dev<uint8_t>(o_seed), seed_stride ? 32u : 0u, n_pk ? hc.dev<uint8_t>(o_pk) : nullptr,
                            pub_stride ? 32u : 0u,
                            m.extent ? hc.dev<uint8_t>(m.o_msgs) : nullptr, hc.dev<uint64_t>(m.o_off),
                            hc.dev<uint32_t>(m.o_len), hc.dev<uint8_t>(o_out), 64, n};
    RT_HIP(launch_ed25519_sign(a, hc.stream()), "ed25519 sign launch");
    hc.get_rows(sigs_out, out_stride < 64 ? 64 : out_stride, o_out, 64, n, "D2H signatures");
    return hc.finish();
}

int rt_ed25519_public(rt_ctx *c, const uint8_t *seeds, uint64_t seed_stride, uint8_t *out, uint64_t out_stride,
                      uint32_t n, void *stream) {
    int rc = public_check(c, seeds, seed_stride, out, out_stride, n);
    if (rc || n == 0) return rc;
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    const Ed25519PublicArgs a{seeds, seed_stride, out, out_stride, n};
    RT_HIP(launch_ed25519_public(a, as_stream(stream)), "ed25519 public launch");
    return RT_OK;
}

int rt_ed25519_public_host(rt_ctx *c, const uint8_t *seeds, uint64_t seed_stride, uint8_t *out, uint64_t out_stride,
                           uint32_t n) {
    int rc = public_check(c, seeds, seed_stride, out, out_stride, n);
    if (rc || n == 0) return rc;
    const uint64_t n_seed = seed_stride ? n : 1u;
    HostCall hc(c, HostCall::PER_ARRAY);
    const uint64_t o_seed = hc.add(32 * n_seed), o_out = hc.add(32ull * n);
    RT_TRY(hc.open());
    hc.put_rows(o_seed, seeds, seed_stride ? seed_stride : 32, 32, n_seed, "H2D seeds");
    RT_TRY(hc.send());
    const Ed25519PublicArgs a{hc.dev<uint8_t>(o_seed), seed_stride ? 32u : 0u, hc.dev<uint8_t>(o_out), 32, n};
    RT_HIP(launch_ed25519_public(a, hc.stream()), "ed25519 public launch");
    hc.get_rows(out, out_stride < 32 ? 32 : out_stride, o_out, 32, n, "D2H public keys");
    return hc.finish();
}

int rt_ifac_sign(rt_ctx *c, const uint8_t *seed, const uint8_t *pub, const uint8_t *pkt, const uint64_t *pkt_off,
                 const uint32_t *pkt_len, uint8_t *ifac_out, uint32_t ifac_size, uint32_t n, void *stream) {
    int rc = ifac_sign_check("rt_ifac_sign", c, seed, pub, pkt, pkt_off, pkt_len, ifac_out, ifac_size, n);
    if (rc || n == 0) return rc;
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    const IfacSignArgs a{seed, pub, 0, pkt, pkt_off, pkt_len, ifac_size, ifac_out, nullptr, nullptr, nullptr, n};
    RT_HIP(launch_ifac_sign(a, as_stream(stream)), "ifac sign launch");
    return RT_OK;
}

int rt_ifac_check(rt_ctx *c, const uint8_t *seed, const uint8_t *pub, const uint8_t *pkt, const uint64_t *pkt_off,
                  uint32_t *pkt_len, const uint8_t *ifac, uint32_t ifac_size, int32_t *status, uint32_t n,
                  void *stream) {
    int rc = ifac_sign_check("rt_ifac_check", c, seed, pub, pkt, pkt_off, pkt_len, ifac, ifac_size, n);
    if (rc || n == 0) return rc;
    if (!status) return fail(RT_E_INVAL, "rt_ifac_check: null status");
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    const IfacSignArgs a{seed, pub, 0, pkt, pkt_off, pkt_len, ifac_size, nullptr, ifac, status, pkt_len, n};
    RT_HIP(launch_ifac_sign(a, as_stream(stream)), "ifac check launch");
    return RT_OK;
}

}  // extern "C"

// capi_derive.hip — key derivation in the C-ABI: HKDF, X25519, and the key
// sets derived from them on the device.  Device pointers on the caller's
// stream; the *_host calls go through a staging lane (capi_internal.h).
#include "capi_internal.h"

extern "C" {

// ------------------------------------------------------------------ HKDF --

static int hkdf_check(rt_ctx *c, const uint8_t *ikm, uint32_t ikm_len, const uint8_t *context, uint32_t context_len,
                      uint32_t length) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (length < 1) return fail(RT_E_INVAL, "Invalid output key length");          // HKDF.py:40-41
    if (ikm_len && !ikm) return fail(RT_E_INVAL, "Cannot derive key from empty input material");   // HKDF.py:43-44
    if (context_len && !context) return fail(RT_E_INVAL, "rt_hkdf: null context bytes");
    return RT_OK;
}

static HkdfArgs hkdf_args(const uint8_t *ikm, uint64_t ikm_stride, uint32_t ikm_len, const uint8_t *salt,
                          uint64_t salt_stride, uint32_t salt_len, const uint8_t *context, uint32_t context_len,
                          uint8_t *out, uint64_t out_stride, uint32_t length, uint32_t n) {
    HkdfArgs a{};
    a.ikm = ikm; a.ikm_stride = ikm_stride; a.ikm_len = ikm_len;
    a.salt = salt_len ? salt : nullptr; a.salt_stride = salt_stride; a.salt_len = salt ? salt_len : 0;
    a.context = context_len ? context : nullptr; a.context_len = context ? context_len : 0;
    a.out = out; a.out_stride = out_stride; a.length = length; a.n = n;
    return a;
}

int rt_hkdf(rt_ctx *c, const uint8_t *ikm, uint64_t ikm_stride, uint32_t ikm_len, const uint8_t *salt,
            uint64_t salt_stride, uint32_t salt_len, const uint8_t *context, uint32_t context_len, uint8_t *out,
            uint64_t out_stride, uint32_t length, uint32_t n, void *stream) {
    int rc = hkdf_check(c, ikm, ikm_len, context, context_len, length);
    if (rc || n == 0) return rc;
    if (!out) return fail(RT_E_INVAL, "rt_hkdf: null output");
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    const HkdfArgs a = hkdf_args(ikm, ikm_stride, ikm_len, salt, salt_stride, salt_len, context, context_len, out,
                                 out_stride, length, n);
    RT_HIP(launch_hkdf(a, as_stream(stream)), "hkdf launch");
    return RT_OK;
}

int rt_hkdf_host(rt_ctx *c, const uint8_t *ikm, uint64_t ikm_stride, uint32_t ikm_len, const uint8_t *salt,
                 uint64_t salt_stride, uint32_t salt_len, const uint8_t *context, uint32_t context_len, uint8_t *out,
                 uint64_t out_stride, uint32_t length, uint32_t n) {
    int rc = hkdf_check(c, ikm, ikm_len, context, context_len, length);
    if (rc || n == 0) return rc;
    if (!out) return fail(RT_E_INVAL, "rt_hkdf: null output");
    if (!salt) salt_len = 0;
    if (!context) context_len = 0;
    // packed copies on the device: ikm n x ikm_len, salt n x salt_len, context, out n x length
    const uint64_t b_ikm = (uint64_t)n * ikm_len, b_salt = (salt_stride ? (uint64_t)n : 1ull) * salt_len,
                   b_out = (uint64_t)n * length;   // salt_stride 0: one shared salt row
    HostCall hc(c, HostCall::PER_ARRAY);
    const uint64_t o_ikm = hc.add(b_ikm), o_salt = hc.add(b_salt), o_ctx = hc.add(context_len), o_out = hc.add(b_out);
    RT_TRY(hc.open());
    hc.put_rows(o_ikm, ikm, ikm_stride, ikm_len, n, "H2D ikm");
    hc.put_rows(o_salt, salt, salt_stride ? salt_stride : salt_len, salt_len, salt_stride ? n : 1u, "H2D salt");
    hc.put(o_ctx, context, context_len, "H2D context");
    RT_TRY(hc.send());
    const HkdfArgs a = hkdf_args(hc.dev<uint8_t>(o_ikm), ikm_len, ikm_len, b_salt ? hc.dev<uint8_t>(o_salt) : nullptr,
                                 salt_stride ? salt_len : 0, salt_len, context_len ? hc.dev<uint8_t>(o_ctx) : nullptr,
                                 context_len, hc.dev<uint8_t>(o_out), length, length, n);
    RT_HIP(launch_hkdf(a, hc.stream()), "hkdf launch");
    hc.get_rows(out, out_stride, o_out, length, n, "D2H out");
    return hc.finish();
}

// Enqueues on s the kernels that write k's records from the keys `a` derives
// (a.length = the key length, a.out unused).
static hipError_t hkdf_records(rt_ctx *c, const HkdfArgs &a, rt_keyset *k, hipStream_t s) {
    // one launch: derive each key in registers and build its record
    hipError_t e = launch_hkdf_key_setup(a, c->d_sbox, k->d_rec, c->n_cu, s);
    if (e != hipErrorNotSupported) return e;
    // other shapes (context, long or unaligned ikm/salt): HKDF into a
    // stream-ordered temporary, then the key setup
    uint8_t *d_keys = nullptr;
    if ((e = hipMallocAsync((void **)&d_keys, (uint64_t)a.n * a.length, s)) != hipSuccess) return e;
    HkdfArgs t = a;
    t.out = d_keys;
    e = launch_hkdf(t, s);
    if (e == hipSuccess) e = launch_key_setup(d_keys, a.length, a.n, c->d_sbox, k->d_rec, s);
    hipFreeAsync(d_keys, s);     // freed after the key setup has consumed it
    return e;
}

rt_keyset *rt_keyset_create_hkdf(rt_ctx *c, const uint8_t *ikm, uint64_t ikm_stride, uint32_t ikm_len,
                                 const uint8_t *salt, uint64_t salt_stride, uint32_t salt_len,
                                 const uint8_t *context, uint32_t context_len, uint32_t key_len, uint32_t n,
                                 void *stream) {
    if (hkdf_check(c, ikm, ikm_len, context, context_len, key_len)) return nullptr;
    if (n == 0) {
        fail(RT_E_INVAL, "rt_keyset_create_hkdf: zero keys");
        return nullptr;
    }
    if (check_key_len(key_len)) return nullptr;
    hipSetDevice(c->device);
    hipStream_t s = as_stream(stream);
    const HkdfArgs a = hkdf_args(ikm, ikm_stride, ikm_len, salt, salt_stride, salt_len, context, context_len, nullptr,
                                 key_len, key_len, n);
    return keyset_on(c, key_len, n, s, [&](rt_keyset *k) { return hkdf_records(c, a, k, s); });
}

// ---------------------------------------------------------------- X25519 --

static int x25519_check(rt_ctx *c, const uint8_t *scalars, uint64_t scalar_stride, const uint8_t *points,
                        uint64_t point_stride, const uint64_t *point_off) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (!scalars) return fail(RT_E_INVAL, "rt_x25519: null scalars");
    if (point_off && !points) return fail(RT_E_INVAL, "rt_x25519: point_off without points");
    if ((scalar_stride && scalar_stride < 32) || (points && !point_off && point_stride && point_stride < 32))
        return fail(RT_E_INVAL, "rt_x25519: a stride is 0 (one row for all) or at least 32");
    return RT_OK;
}

int rt_x25519(rt_ctx *c, const uint8_t *scalars, uint64_t scalar_stride, const uint8_t *points, uint64_t point_stride,
              const uint64_t *point_off, uint8_t *out, uint64_t out_stride, uint32_t n, void *stream) {
    int rc = x25519_check(c, scalars, scalar_stride, points, point_stride, point_off);
    if (rc || n == 0) return rc;
    if (!out) return fail(RT_E_INVAL, "rt_x25519: null output");
    if (out_stride < 32 && n > 1) return fail(RT_E_INVAL, "rt_x25519: out_stride smaller than 32");
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    const X25519Args a{scalars, scalar_stride, points, point_stride, point_off, out, out_stride, n};
    RT_HIP(launch_x25519(a, as_stream(stream)), "x25519 launch");
    return RT_OK;
}

int rt_x25519_host(rt_ctx *c, const uint8_t *scalars, uint64_t scalar_stride, const uint8_t *points,
                   uint64_t point_stride, const uint64_t *point_off, uint8_t *out, uint64_t out_stride, uint32_t n) {
    int rc = x25519_check(c, scalars, scalar_stride, points, point_stride, point_off);
    if (rc || n == 0) return rc;
    if (!out) return fail(RT_E_INVAL, "rt_x25519: null output");
    if (out_stride < 32 && n > 1) return fail(RT_E_INVAL, "rt_x25519: out_stride smaller than 32");
    // packed rows on the device: scalars (n or 1) x 32, points (n or 1) x 32, out n x 32
    const uint64_t n_sc = scalar_stride ? n : 1u, n_pt = !points ? 0u : (point_off || point_stride) ? n : 1u;
    std::vector<uint8_t> gathered;     // rows named by point_off, packed (alive until finish() has synchronised)
    if (point_off) {
        gathered.resize(32ull * n);
        for (uint32_t i = 0; i < n; ++i) memcpy(&gathered[32ull * i], points + point_off[i], 32);
    }
    HostCall hc(c, HostCall::PER_ARRAY);
    const uint64_t o_sc = hc.add(32 * n_sc), o_pt = hc.add(32 * n_pt), o_out = hc.add(32ull * n);
    RT_TRY(hc.open());
    hc.put_rows(o_sc, scalars, scalar_stride ? scalar_stride : 32, 32, n_sc, "H2D scalars");
    if (point_off)
        hc.put(o_pt, gathered.data(), 32ull * n, "H2D points");
    else
        hc.put_rows(o_pt, points, point_stride ? point_stride : 32, 32, n_pt, "H2D points");
    RT_TRY(hc.send());
    const X25519Args a{hc.dev<uint8_t>(o_sc), scalar_stride ? 32u : 0u, n_pt ? hc.dev<uint8_t>(o_pt) : nullptr,
                       n_pt > 1 ? 32u : 0u, nullptr, hc.dev<uint8_t>(o_out), 32, n};
    RT_HIP(launch_x25519(a, hc.stream()), "x25519 launch");
    hc.get_rows(out, out_stride < 32 ? 32 : out_stride, o_out, 32, n, "D2H out");
    return hc.finish();
}

rt_keyset *rt_keyset_create_x25519(rt_ctx *c, const uint8_t *scalars, uint64_t scalar_stride, const uint8_t *points,
                                   uint64_t point_stride, const uint64_t *point_off, const uint8_t *salt,
                                   uint64_t salt_stride, uint32_t salt_len, const uint8_t *context,
                                   uint32_t context_len, uint32_t key_len, uint32_t n, void *stream) {
    if (x25519_check(c, scalars, scalar_stride, points, point_stride, point_off)) return nullptr;
    if (context_len && !context) {
        fail(RT_E_INVAL, "rt_keyset_create_x25519: null context bytes");
        return nullptr;
    }
    if (n == 0) {
        fail(RT_E_INVAL, "rt_keyset_create_x25519: zero keys");
        return nullptr;
    }
    if (check_key_len(key_len)) return nullptr;
    hipSetDevice(c->device);
    hipStream_t s = as_stream(stream);
    return keyset_on(c, key_len, n, s, [&](rt_keyset *k) {
        // the shared secrets live in a stream-ordered temporary: written by
        // the exchange, read by the key derivation, freed after it
        uint8_t *d_shared = nullptr;
        hipError_t e = hipMallocAsync((void **)&d_shared, 32ull * n, s);
        if (e != hipSuccess) return e;
        const X25519Args x{scalars, scalar_stride, points, point_stride, point_off, d_shared, 32, n};
        e = launch_x25519(x, s);
        if (e == hipSuccess)
            e = hkdf_records(c, hkdf_args(d_shared, 32, 32, salt, salt_stride, salt_len, context, context_len, nullptr,
                                          key_len, key_len, n), k, s);
        hipFreeAsync(d_shared, s);
        return e;
    });
}

}  // extern "C"

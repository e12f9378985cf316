// capi_token.hip — the Token entry points of the C-ABI: encrypt, decrypt,
// verify and the ratchet trials, on device pointers (enqueued on the caller's
// stream) and on host pointers (through a staging lane, capi_internal.h).
#include "capi_internal.h"

extern "C" {

int rt_plan_uniform(const rt_ctx *c, uint32_t n, uint32_t len, int per_packet_keys, int decrypt) {
    if (!c) return fail(RT_E_INVAL, "rt_plan_uniform: no context");
    return decrypt ? plan_decrypt(n, false, len, per_packet_keys != 0, c->n_cu)
                   : plan_encrypt(n, false, len, per_packet_keys != 0, c->n_cu);
}

uint64_t rt_token_len(uint64_t pt_len) { return 16u + 16u * (pt_len / 16u + 1u) + 32u; }

static int enc_common(const rt_keyset *k, EncArgs &a, void *stream) {
    RT_TRY(check_keyset(k));
    if (a.n == 0) return RT_OK;
    // a uniform batch of empty plaintexts reads no plaintext bytes
    if ((!a.pt && (a.pt_len || a.uni_len)) || !a.iv || !a.tok) return fail(RT_E_INVAL, "rt_encrypt: null buffer");
    a.rec = k->d_rec;
    a.sbox = k->ctx->d_sbox;
    if (unsigned long long *w = k->ctx->clk.load(std::memory_order_acquire)) a.clk = w + 4 * RT_CLOCK_ENCRYPT;
    return launch_with_keys(k, stream, "encrypt launch", [&](hipStream_t s) {
        return launch_encrypt(a, k->nr, k->ctx->n_cu, &k->ctx->queues, s);
    });
}

static int dec_common(const rt_keyset *k, DecArgs &a, void *stream) {
    RT_TRY(check_keyset(k));
    if (a.n == 0) return RT_OK;
    if (!a.tok || !a.pt || !a.out_len || !a.status) return fail(RT_E_INVAL, "rt_decrypt: null buffer");
    a.rec = k->d_rec;
    a.sbox = k->ctx->d_sbox;
    if (unsigned long long *w = k->ctx->clk.load(std::memory_order_acquire)) a.clk = w + 4 * RT_CLOCK_DECRYPT;
    return launch_with_keys(k, stream, "decrypt launch", [&](hipStream_t s) {
        return launch_decrypt(a, k->nr, k->ctx->n_cu, &k->ctx->queues, s);
    });
}

int rt_encrypt(const rt_keyset *k, const uint8_t *pt, const uint64_t *pt_off, const uint32_t *pt_len,
               const uint32_t *key_idx, const uint8_t *iv, uint8_t *tok, const uint64_t *tok_off, uint32_t n,
               void *stream) {
    if (n && (!pt_off || !pt_len || !tok_off)) return fail(RT_E_INVAL, "rt_encrypt: null offset/length array");
    EncArgs a{};
    a.pt = pt; a.pt_off = pt_off; a.pt_len = pt_len; a.key_idx = key_idx; a.iv = iv;
    a.tok = tok; a.tok_off = tok_off; a.n = n;
    return enc_common(k, a, stream);
}

int rt_encrypt_uniform(const rt_keyset *k, const uint8_t *pt, uint64_t pt_stride, uint32_t pt_len,
                       const uint32_t *key_idx, const uint8_t *iv, uint8_t *tok, uint64_t tok_stride, uint32_t n,
                       void *stream) {
    if (n > 1 && (pt_stride < pt_len || tok_stride < rt_token_len(pt_len)))
        return fail(RT_E_INVAL, "rt_encrypt_uniform: stride smaller than packet/token");
    EncArgs a{};
    a.pt = pt; a.pt_stride = pt_stride; a.uni_len = pt_len; a.key_idx = key_idx; a.iv = iv;
    a.tok = tok; a.tok_stride = tok_stride; a.n = n;
    return enc_common(k, a, stream);
}

int rt_encrypt_interleaved(const rt_keyset *k, const uint8_t *pt, uint32_t pt_len, const uint32_t *key_idx,
                           const uint8_t *iv, uint8_t *tok, uint32_t n, void *stream) {
    EncArgs a{};
    a.pt = pt; a.uni_len = pt_len; a.key_idx = key_idx; a.iv = iv; a.tok = tok; a.n = n; a.ilv = 1;
    return enc_common(k, a, stream);
}

int rt_decrypt_interleaved(const rt_keyset *k, const uint8_t *tok, uint32_t tok_len, const uint32_t *key_idx,
                           uint8_t *pt, uint32_t *pt_len, int32_t *status, uint32_t n, void *stream) {
    if (tok_len < 64u || (tok_len & 15u))
        return fail(RT_E_INVAL, "rt_decrypt_interleaved: token length must be 48 + 16*k, k >= 1");
    DecArgs a{};
    a.tok = tok; a.uni_len = tok_len; a.key_idx = key_idx; a.pt = pt; a.out_len = pt_len; a.status = status; a.n = n;
    a.ilv = 1;
    return dec_common(k, a, stream);
}

int rt_decrypt(const rt_keyset *k, const uint8_t *tok, const uint64_t *tok_off, const uint32_t *tok_len,
               const uint32_t *key_idx, uint8_t *pt, const uint64_t *pt_off, uint32_t *pt_len, int32_t *status,
               uint32_t n, void *stream) {
    if (n && (!tok_off || !tok_len || !pt_off)) return fail(RT_E_INVAL, "rt_decrypt: null offset/length array");
    DecArgs a{};
    a.tok = tok; a.tok_off = tok_off; a.tok_len = tok_len; a.key_idx = key_idx; a.pt = pt; a.pt_off = pt_off;
    a.out_len = pt_len; a.status = status; a.n = n;
    return dec_common(k, a, stream);
}

int rt_decrypt_uniform(const rt_keyset *k, const uint8_t *tok, uint64_t tok_stride, uint32_t tok_len,
                       const uint32_t *key_idx, uint8_t *pt, uint64_t pt_stride, uint32_t *pt_len, int32_t *status,
                       uint32_t n, void *stream) {
    if (n > 1 && (tok_stride < tok_len || (tok_len > 48 && pt_stride < tok_len - 48)))
        return fail(RT_E_INVAL, "rt_decrypt_uniform: stride smaller than token/plaintext");
    DecArgs a{};
    a.tok = tok; a.tok_stride = tok_stride; a.uni_len = tok_len; a.key_idx = key_idx; a.pt = pt;
    a.pt_stride = pt_stride; a.out_len = pt_len; a.status = status; a.n = n;
    return dec_common(k, a, stream);
}

uint64_t rt_workspace_bytes(uint32_t n) { return sort_workspace_bytes(n); }

int rt_encrypt_ex(const rt_keyset *k, const uint8_t *pt, const uint64_t *pt_off, const uint32_t *pt_len,
                  const uint32_t *key_idx, const uint8_t *iv, uint8_t *tok, const uint64_t *tok_off, uint32_t n,
                  uint32_t flags, void *workspace, void *stream) {
    if (n && (!pt_off || !pt_len || !tok_off)) return fail(RT_E_INVAL, "rt_encrypt_ex: null offset/length array");
    if (flags & ~RT_F_SORT_BY_LENGTH) return fail(RT_E_INVAL, "rt_encrypt_ex: unknown flags");
    RT_TRY(check_keyset(k));
    EncArgs a{};
    a.pt = pt; a.pt_off = pt_off; a.pt_len = pt_len; a.key_idx = key_idx; a.iv = iv;
    a.tok = tok; a.tok_off = tok_off; a.n = n;
    if ((flags & RT_F_SORT_BY_LENGTH) && n > 1) {
        if (!workspace) return fail(RT_E_INVAL, "rt_encrypt_ex: RT_F_SORT_BY_LENGTH needs a workspace");
        RT_HIP(hipSetDevice(k->ctx->device), "hipSetDevice");
        RT_HIP(launch_length_order(pt_len, n, 0, workspace, &a.order, &a.queue, k->ctx->n_cu, as_stream(stream)),
               "length order");
    }
    return enc_common(k, a, stream);
}

int rt_decrypt_ex(const rt_keyset *k, const uint8_t *tok, const uint64_t *tok_off, const uint32_t *tok_len,
                  const uint32_t *key_idx, uint8_t *pt, const uint64_t *pt_off, uint32_t *pt_len, int32_t *status,
                  uint32_t n, uint32_t flags, void *workspace, void *stream) {
    if (n && (!tok_off || !tok_len || !pt_off)) return fail(RT_E_INVAL, "rt_decrypt_ex: null offset/length array");
    if (flags & ~RT_F_SORT_BY_LENGTH) return fail(RT_E_INVAL, "rt_decrypt_ex: unknown flags");
    RT_TRY(check_keyset(k));
    DecArgs a{};
    a.tok = tok; a.tok_off = tok_off; a.tok_len = tok_len; a.key_idx = key_idx; a.pt = pt; a.pt_off = pt_off;
    a.out_len = pt_len; a.status = status; a.n = n;
    if ((flags & RT_F_SORT_BY_LENGTH) && n > 1) {
        if (!workspace) return fail(RT_E_INVAL, "rt_decrypt_ex: RT_F_SORT_BY_LENGTH needs a workspace");
        RT_HIP(hipSetDevice(k->ctx->device), "hipSetDevice");
        RT_HIP(launch_length_order(tok_len, n, 1, workspace, &a.order, &a.queue, k->ctx->n_cu, as_stream(stream)),
               "length order");
    }
    return dec_common(k, a, stream);
}

// ------------------------------------------------------------- verify_hmac

static int verify_common(const rt_keyset *k, VerifyArgs &a, void *stream) {
    RT_TRY(check_keyset(k));
    if (a.n == 0) return RT_OK;
    if (!a.status) return fail(RT_E_INVAL, "rt_verify: null status");
    a.rec = k->d_rec;
    return launch_with_keys(k, stream, "verify launch", [&](hipStream_t s) { return launch_verify(a, s); });
}

int rt_verify(const rt_keyset *k, const uint8_t *tok, const uint64_t *tok_off, const uint32_t *tok_len,
              const uint32_t *key_idx, int32_t *status, uint32_t n, void *stream) {
    if (n && (!tok_off || !tok_len)) return fail(RT_E_INVAL, "rt_verify: null offset/length array");
    VerifyArgs a{};
    a.tok = tok; a.tok_off = tok_off; a.tok_len = tok_len; a.key_idx = key_idx; a.status = status; a.n = n;
    return verify_common(k, a, stream);
}

// ----------------------------------------------------------- ratchet trials

int rt_verify_trials(const rt_keyset *k, const uint8_t *tok, const uint64_t *tok_off, const uint32_t *tok_len,
                     const uint32_t *pair_off, const uint32_t *pair_key, uint32_t *first, uint32_t n_tok,
                     uint32_t n_pairs, void *stream) {
    RT_TRY(check_keyset(k));
    if (n_tok == 0) return RT_OK;
    if (!tok_off || !tok_len || !pair_off || !first || (n_pairs && (!tok || !pair_key)))
        return fail(RT_E_INVAL, "rt_verify_trials: null argument");
    TrialArgs a{};
    a.rec = k->d_rec; a.tok = tok; a.tok_off = tok_off; a.tok_len = tok_len; a.pair_off = pair_off;
    a.pair_key = pair_key; a.first = first; a.n_tok = n_tok; a.n_pairs = n_pairs;
    return launch_with_keys(k, stream, "verify trials launch",
                            [&](hipStream_t s) { return launch_verify_trials(a, s); });
}

// ---------------------------------------------------------------- host path
//
// One packet per call (Token.encrypt / Token.decrypt): the token kernel reads
// its inputs from the lane's mapped pinned staging buffer and writes its
// outputs there (host_direct: HostCall::open(true)), instead of a copy kernel
// in, the token kernel, and a store kernel out (the runtime's H2D of a small
// pinned buffer is itself a blit kernel, 2.4 us, and the store kernel 3.6 us,
// each plus its dispatch).  383-B packets, one thread: Token.encrypt 57.8 ->
// 50.1 us, Token.decrypt 45.5 -> 38.6 us, 19 100 -> 21 800 calls/s (three runs
// each, profiles/r06_host_direct_ab.txt).  Batches keep the copies (their
// kernels would read every packet across PCIe; not measured).

int rt_verify_trials_host(const rt_keyset *k, const uint8_t *tok, const uint64_t *tok_off, const uint32_t *tok_len,
                          const uint32_t *pair_off, const uint32_t *pair_key, uint32_t *first, uint32_t n_tok,
                          uint32_t n_pairs) {
    RT_TRY(check_keyset(k));
    if (n_tok == 0) return RT_OK;
    if (!tok_off || !tok_len || !pair_off || !first || (n_pairs && !pair_key))
        return fail(RT_E_INVAL, "rt_verify_trials_host: null argument");
    if (pair_off[0] != 0 || pair_off[n_tok] != n_pairs)
        return fail(RT_E_INVAL, "rt_verify_trials_host: pair_off must run from 0 to n_pairs");
    uint64_t tok_ext = 0;
    for (uint32_t t = 0; t < n_tok; ++t) {
        if (pair_off[t + 1] < pair_off[t]) return fail(RT_E_INVAL, "rt_verify_trials_host: pair_off not ascending");
        tok_ext = std::max<uint64_t>(tok_ext, tok_off[t] + tok_len[t]);
    }
    for (uint32_t j = 0; j < n_pairs; ++j)
        if (pair_key[j] >= k->n_keys) return fail(RT_E_INVAL, "pair_key out of range");
    if (tok_ext && !tok) return fail(RT_E_INVAL, "rt_verify_trials_host: null tokens");
    HostCall hc(k->ctx, HostCall::PER_ARRAY);
    const uint64_t o_tok = hc.add(tok_ext), o_to = hc.add(8ull * n_tok), o_tl = hc.add(4ull * n_tok),
                   o_po = hc.add(4ull * (n_tok + 1)), o_pk = hc.add(4ull * n_pairs), o_fi = hc.add(4ull * n_tok);
    RT_TRY(hc.open());
    hc.put(o_tok, tok, tok_ext, "H2D tok");
    hc.put(o_to, tok_off, 8ull * n_tok, "H2D tok_off");
    hc.put(o_tl, tok_len, 4ull * n_tok, "H2D tok_len");
    hc.put(o_po, pair_off, 4ull * (n_tok + 1), "H2D pair_off");
    hc.put(o_pk, pair_key, 4ull * n_pairs, "H2D pair_key");
    RT_TRY(hc.send());
    RT_TRY(rt_verify_trials(k, hc.dev<uint8_t>(o_tok), hc.dev<uint64_t>(o_to), hc.dev<uint32_t>(o_tl),
                            hc.dev<uint32_t>(o_po), hc.dev<uint32_t>(o_pk), hc.dev<uint32_t>(o_fi), n_tok, n_pairs,
                            hc.stream()));
    hc.get(first, o_fi, 4ull * n_tok, "D2H first");
    return hc.finish();
}

int rt_encrypt_host(const rt_keyset *k, const uint8_t *pt, const uint64_t *pt_off, const uint32_t *pt_len,
                    const uint32_t *key_idx, const uint8_t *iv, uint8_t *tok, const uint64_t *tok_off, uint32_t n) {
    RT_TRY(check_keyset(k));
    if (n == 0) return RT_OK;
    if (!pt_off || !pt_len || !tok_off || !iv || !tok) return fail(RT_E_INVAL, "rt_encrypt_host: null argument");
    uint64_t pt_ext = 0, tok_ext = 0, tok_sum = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (key_idx && key_idx[i] >= k->n_keys) return fail(RT_E_INVAL, "key_idx out of range");
        pt_ext = std::max<uint64_t>(pt_ext, pt_off[i] + pt_len[i]);
        const uint64_t tl = rt_token_len(pt_len[i]);
        tok_ext = std::max<uint64_t>(tok_ext, tok_off[i] + tl);
        tok_sum += tl;
    }
    if (pt_ext && !pt) return fail(RT_E_INVAL, "rt_encrypt_host: null plaintext");
    const bool gaps = tok_sum != tok_ext;   // gaps between tokens: keep the caller's bytes there
    HostCall hc(k->ctx, HostCall::MIRROR);
    // inputs first, the token region last: one copy in, one copy out
    const uint64_t o_pt = hc.add(pt_ext), o_iv = hc.add(16ull * n), o_po = hc.add(8ull * n), o_pl = hc.add(4ull * n),
                   o_to = hc.add(8ull * n), o_ki = key_idx ? hc.add(4ull * n) : 0, o_tok = hc.add(tok_ext);
    RT_TRY(hc.open(n == 1));
    hc.put(o_pt, pt, pt_ext, "H2D pt");
    if (gaps) hc.put(o_tok, tok, tok_ext, "H2D tok");
    hc.put(o_iv, iv, 16ull * n, "H2D iv");
    hc.put(o_po, pt_off, 8ull * n, "H2D pt_off");
    hc.put(o_pl, pt_len, 4ull * n, "H2D pt_len");
    hc.put(o_to, tok_off, 8ull * n, "H2D tok_off");
    if (key_idx) hc.put(o_ki, key_idx, 4ull * n, "H2D key_idx");
    RT_TRY(hc.send(gaps ? hc.total() : o_tok));
    EncArgs a{};
    a.pt = hc.dev<uint8_t>(o_pt); a.pt_off = hc.dev<uint64_t>(o_po); a.pt_len = hc.dev<uint32_t>(o_pl);
    a.key_idx = key_idx ? hc.dev<uint32_t>(o_ki) : nullptr; a.iv = hc.dev<uint8_t>(o_iv);
    a.tok = hc.dev<uint8_t>(o_tok); a.tok_off = hc.dev<uint64_t>(o_to); a.n = n;
    if (n == 1) {       // one packet (Token.encrypt): a uniform batch of one, so the latency-shaped kernels apply
        a.pt += pt_off[0]; a.pt_off = nullptr; a.pt_len = nullptr; a.uni_len = pt_len[0];
        a.tok += tok_off[0]; a.tok_off = nullptr;
    }
    RT_TRY(enc_common(k, a, hc.stream()));
    hc.get(tok, o_tok, tok_ext, "D2H tok");
    return hc.finish();
}

int rt_decrypt_host(const rt_keyset *k, const uint8_t *tok, const uint64_t *tok_off, const uint32_t *tok_len,
                    const uint32_t *key_idx, uint8_t *pt, const uint64_t *pt_off, uint32_t *pt_len, int32_t *status,
                    uint32_t n) {
    RT_TRY(check_keyset(k));
    if (n == 0) return RT_OK;
    if (!tok_off || !tok_len || !pt_off || !pt_len || !status) return fail(RT_E_INVAL, "rt_decrypt_host: null argument");
    uint64_t tok_ext = 0, pt_ext = 0, pt_sum = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (key_idx && key_idx[i] >= k->n_keys) return fail(RT_E_INVAL, "key_idx out of range");
        tok_ext = std::max<uint64_t>(tok_ext, tok_off[i] + tok_len[i]);
        const uint64_t pl = tok_len[i] > 48 ? tok_len[i] - 48 : 0;
        pt_ext = std::max<uint64_t>(pt_ext, pt_off[i] + pl);
        pt_sum += pl;
    }
    if ((tok_ext && !tok) || (pt_ext && !pt)) return fail(RT_E_INVAL, "rt_decrypt_host: null buffer");
    const bool gaps = pt_ext && pt_sum != pt_ext;   // gaps between plaintexts: keep the caller's bytes there
    HostCall hc(k->ctx, HostCall::MIRROR);
    // inputs first, the outputs (plaintexts, lengths, status) last: one copy
    // in, one copy out
    const uint64_t o_tok = hc.add(tok_ext), o_to = hc.add(8ull * n), o_tl = hc.add(4ull * n), o_po = hc.add(8ull * n),
                   o_ki = key_idx ? hc.add(4ull * n) : 0, o_pt = hc.add(pt_ext), o_ol = hc.add(4ull * n),
                   o_st = hc.add(4ull * n);
    RT_TRY(hc.open(n == 1));
    hc.put(o_tok, tok, tok_ext, "H2D tok");
    if (gaps) hc.put(o_pt, pt, pt_ext, "H2D pt");
    hc.put(o_to, tok_off, 8ull * n, "H2D tok_off");
    hc.put(o_tl, tok_len, 4ull * n, "H2D tok_len");
    hc.put(o_po, pt_off, 8ull * n, "H2D pt_off");
    if (key_idx) hc.put(o_ki, key_idx, 4ull * n, "H2D key_idx");
    RT_TRY(hc.send(gaps ? o_ol : o_pt));
    DecArgs a{};
    a.tok = hc.dev<uint8_t>(o_tok); a.tok_off = hc.dev<uint64_t>(o_to); a.tok_len = hc.dev<uint32_t>(o_tl);
    a.key_idx = key_idx ? hc.dev<uint32_t>(o_ki) : nullptr; a.pt = hc.dev<uint8_t>(o_pt);
    a.pt_off = hc.dev<uint64_t>(o_po); a.out_len = hc.dev<uint32_t>(o_ol); a.status = hc.dev<int32_t>(o_st);
    a.n = n;
    if (n == 1) {       // one token (Token.decrypt): a uniform batch of one
        a.tok += tok_off[0]; a.tok_off = nullptr; a.tok_len = nullptr; a.uni_len = tok_len[0];
        a.pt += pt_off[0]; a.pt_off = nullptr;
    }
    RT_TRY(dec_common(k, a, hc.stream()));
    hc.get(pt, o_pt, pt_ext, "D2H pt");
    hc.get(pt_len, o_ol, 4ull * n, "D2H pt_len");
    hc.get(status, o_st, 4ull * n, "D2H status");
    return hc.finish();
}

int rt_verify_host(const rt_keyset *k, const uint8_t *tok, const uint64_t *tok_off, const uint32_t *tok_len,
                   const uint32_t *key_idx, int32_t *status, uint32_t n) {
    RT_TRY(check_keyset(k));
    if (n == 0) return RT_OK;
    if (!tok_off || !tok_len || !status) return fail(RT_E_INVAL, "rt_verify_host: null argument");
    uint64_t tok_ext = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (key_idx && key_idx[i] >= k->n_keys) return fail(RT_E_INVAL, "key_idx out of range");
        tok_ext = std::max<uint64_t>(tok_ext, tok_off[i] + tok_len[i]);
    }
    if (tok_ext && !tok) return fail(RT_E_INVAL, "rt_verify_host: null tokens");
    HostCall hc(k->ctx, HostCall::MIRROR);
    const uint64_t o_tok = hc.add(tok_ext), o_to = hc.add(8ull * n), o_tl = hc.add(4ull * n),
                   o_ki = key_idx ? hc.add(4ull * n) : 0, o_st = hc.add(4ull * n);
    RT_TRY(hc.open());
    hc.put(o_tok, tok, tok_ext, "H2D tok");
    hc.put(o_to, tok_off, 8ull * n, "H2D tok_off");
    hc.put(o_tl, tok_len, 4ull * n, "H2D tok_len");
    if (key_idx) hc.put(o_ki, key_idx, 4ull * n, "H2D key_idx");
    RT_TRY(hc.send(o_st));
    VerifyArgs a{};
    a.tok = hc.dev<uint8_t>(o_tok); a.tok_off = hc.dev<uint64_t>(o_to); a.tok_len = hc.dev<uint32_t>(o_tl);
    a.key_idx = key_idx ? hc.dev<uint32_t>(o_ki) : nullptr; a.status = hc.dev<int32_t>(o_st); a.n = n;
    RT_TRY(verify_common(k, a, hc.stream()));
    hc.get(status, o_st, 4ull * n, "D2H status");
    return hc.finish();
}

}  // extern "C"

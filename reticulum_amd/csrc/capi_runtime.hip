// capi_runtime.hip — the runtime under librnstok's C-ABI (include/rnstok.h):
// error reporting, device contexts, key sets built from raw keys, the staging
// lanes of the host-pointer calls (HostCall), memory helpers, clock stamps.
#include "capi_internal.h"

// ------------------------------------------------------------------ errors

static thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
int hip_fail(hipError_t e, const char *what) {
    return fail(RT_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// ------------------------------------------------------------ chunk queues

uint32_t *QueueRing::acquire(hipStream_t s, uint32_t *slot) {
    if (!d) return nullptr;
    for (uint32_t tries = 0; tries < SLOTS; ++tries) {
        const uint32_t i = next.fetch_add(1u, std::memory_order_relaxed) % SLOTS;
        uint32_t free_ = 0u;
        if (!busy[i].compare_exchange_strong(free_, 1u, std::memory_order_acquire)) continue;
        if (recorded[i] && hipStreamWaitEvent(s, ev[i], 0) != hipSuccess) {
            busy[i].store(0u, std::memory_order_release);
            return nullptr;
        }
        *slot = i;
        return d + 16u * i;
    }
    return nullptr;
}
void QueueRing::release(hipStream_t s, uint32_t slot) {
    if (hipEventRecord(ev[slot], s) == hipSuccess) recorded[slot] = true;
    busy[slot].store(0u, std::memory_order_release);
}

// ---------------------------------------------------------------- key sets

hipError_t rec_alloc(rt_ctx *c, uint64_t bytes, uint32_t **p, hipStream_t s) {
    *p = nullptr;
    return c->pool ? hipMallocFromPoolAsync((void **)p, bytes, c->pool, s) : hipMallocAsync((void **)p, bytes, s);
}

int check_keyset(const rt_keyset *k) {
    if (!k || !k->ctx || !k->d_rec) return fail(RT_E_INVAL, "null keyset");
    return RT_OK;
}

int check_key_len(uint32_t key_len) {
    if (key_len == 64 || key_len == 32) return RT_OK;
    return fail(RT_E_INVAL, "Token key must be 128 or 256 bits, not " + std::to_string(key_len * 8));
}

hipError_t after_setup(const rt_keyset *k, hipStream_t s) {
    return s == k->home ? hipSuccess : hipStreamWaitEvent(s, k->ready, 0);
}
// Entries of other streams whose last recorded launch has completed are
// dropped on the way (their event destroyed), so a long-lived key set used
// from many short-lived streams keeps one entry per stream still in flight,
// and rt_keyset_destroy never waits on events of streams that are gone.
hipError_t note_use(rt_keyset *k, hipStream_t s) {
    std::lock_guard<std::mutex> g(k->mu);
    for (auto &u : k->uses)
        if (u.first == s) return hipEventRecord(u.second, s);
    if (k->uses.size() >= 4) {
        auto done = [](const std::pair<hipStream_t, hipEvent_t> &u) {
            if (hipEventQuery(u.second) != hipSuccess) return false;
            hipEventDestroy(u.second);
            return true;
        };
        k->uses.erase(std::remove_if(k->uses.begin(), k->uses.end(), done), k->uses.end());
    }
    hipEvent_t e = nullptr;
    hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (r != hipSuccess) return r;
    k->uses.emplace_back(s, e);
    return hipEventRecord(e, s);
}

// ------------------------------------------------------------- D2H copies

// Device -> host copy on stream s.  A pinned (page-locked, mapped) destination
// is written by GPU stores (launch_store_host: 54 GB/s, and it shares the
// link with a copy-engine H2D at 87 GB/s in total, against 30 GB/s for the
// copy engine's D2H, profiles/r03n_pcie_probe.json); a pageable one goes
// through hipMemcpyAsync.  The store kernel runs on the stream's GPU, so it
// is used only when src is device memory of that GPU (`device`); any other
// source (host memory, another GPU's buffer) takes hipMemcpyAsync, which
// handles every source the copy engine can read.
bool query(hipPointerAttribute_t *at, const void *p) {
    if (hipPointerGetAttributes(at, p) == hipSuccess) return true;
    (void)hipGetLastError();       // a pageable pointer is an "invalid value" to the query: clear only that
    return false;
}
hipError_t copy_d2h(void *dst, const void *src, uint64_t bytes, hipStream_t s, int device) {
    if (!bytes) return hipSuccess;
    hipPointerAttribute_t ad, as;
    if (query(&ad, dst) && ad.type == hipMemoryTypeHost && ad.devicePointer && query(&as, src) &&
        as.type == hipMemoryTypeDevice && as.device == device)
        return launch_store_host((uint8_t *)ad.devicePointer, (const uint8_t *)src, bytes, s);
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
}

// ---------------------------------------------------------------- host path

static int ensure_work(Stager &g, uint64_t bytes) {
    if (bytes <= g.work_cap) return RT_OK;
    uint64_t cap = std::max<uint64_t>(bytes, g.work_cap * 2);
    cap = (cap + 4095) & ~4095ull;
    if (g.d_work) {
        RT_HIP(hipStreamSynchronize(g.stream), "stream sync");   // queued work may still read the old workspace
        hipFree(g.d_work);
    }
    g.d_work = nullptr;
    g.work_cap = 0;
    if (hipMalloc(&g.d_work, cap) != hipSuccess) return fail(RT_E_NOMEM, "workspace allocation failed");
    g.work_cap = cap;
    return RT_OK;
}

// The pinned stage for a host call of `bytes`, or null (too large, or the
// pinned allocation failed): the caller then copies from its own pageable
// arrays.  Called with the lane locked.
static uint8_t *stage(Stager &g, uint64_t bytes) {
    if (bytes > STAGE_MAX) return nullptr;
    if (g.stage_busy) {            // a copy from h_stage may still be queued
        if (hipStreamSynchronize(g.stream) != hipSuccess) return nullptr;
        g.stage_busy = false;
    }
    if (bytes > g.stage_cap) {
        const uint64_t cap = std::min<uint64_t>(STAGE_MAX, std::max<uint64_t>({bytes, 2 * g.stage_cap, 64ull << 10}));
        if (g.h_stage) hipHostFree(g.h_stage);
        g.h_stage = nullptr;
        g.stage_cap = 0;
        if (hipHostMalloc(&g.h_stage, cap, hipHostMallocDefault) != hipSuccess) {
            g.h_stage = nullptr;
            return nullptr;
        }
        if (hipHostGetDevicePointer((void **)&g.h_stage_dev, g.h_stage, 0) != hipSuccess) {
            hipHostFree(g.h_stage);
            g.h_stage = g.h_stage_dev = nullptr;
            return nullptr;
        }
        g.stage_cap = cap;
    }
    return g.h_stage;
}

HostCall::HostCall(rt_ctx *c, Transport t) : c_(c), transport_(t) {
    const uint32_t start = c->stager_rr.fetch_add(1);
    for (int i = 0; i < N_STAGERS && !g_; ++i) {
        Stager &g = c->stagers[(start + i) % N_STAGERS];
        if (g.mu.try_lock()) g_ = &g;
    }
    if (!g_) {
        g_ = &c->stagers[start % N_STAGERS];
        g_->mu.lock();
    }
}

HostCall::~HostCall() {
    if (open_ && hipStreamSynchronize(g_->stream) == hipSuccess) g_->stage_busy = false;
    g_->mu.unlock();
}

int HostCall::open(bool one_packet) {
    RT_HIP(hipSetDevice(c_->device), "hipSetDevice");
    RT_TRY(ensure_work(*g_, end_));
    open_ = true;
    if (transport_ == MIRROR && (h_ = stage(*g_, end_))) {
        g_->stage_busy = true;
        direct_ = one_packet;
    }
    return RT_OK;
}

void HostCall::put(uint64_t off, const void *src, uint64_t bytes, const char *what) {
    if (!bytes || put_err_ != hipSuccess) return;
    if (h_) {
        memcpy(h_ + off, src, bytes);
    } else if ((put_err_ = hipMemcpyAsync(g_->d_work + off, src, bytes, hipMemcpyHostToDevice, g_->stream)) != hipSuccess) {
        put_what_ = what;
    }
}

void HostCall::put_rows(uint64_t off, const void *src, uint64_t src_pitch, uint64_t row, uint64_t rows,
                        const char *what) {
    if (!row || !rows || put_err_ != hipSuccess) return;
    if (h_) {
        for (uint64_t r = 0; r < rows; ++r) memcpy(h_ + off + r * row, (const uint8_t *)src + r * src_pitch, row);
    } else if ((put_err_ = hipMemcpy2DAsync(g_->d_work + off, row, src, src_pitch, row, rows, hipMemcpyHostToDevice,
                                            g_->stream)) != hipSuccess) {
        put_what_ = what;
    }
}

int HostCall::send(uint64_t upto) {
    if (put_err_ != hipSuccess) return hip_fail(put_err_, put_what_);
    if (h_ && !direct_ && upto)
        RT_HIP(hipMemcpyAsync(g_->d_work, h_, upto, hipMemcpyHostToDevice, g_->stream), "H2D stage");
    return RT_OK;
}

int HostCall::finish() {
    hipStream_t s = g_->stream;
    if (h_) {
        uint64_t lo = ~0ull, hi = 0;
        for (int i = 0; i < n_outs_; ++i) {
            lo = std::min(lo, outs_[i].off);
            hi = std::max(hi, outs_[i].off + outs_[i].row * outs_[i].rows);
        }
        if (!direct_ && hi > lo) RT_HIP(launch_store_host(g_->h_stage_dev + lo, g_->d_work + lo, hi - lo, s), "D2H stage");
    } else {
        for (int i = 0; i < n_outs_; ++i) {
            const Out &o = outs_[i];
            const uint8_t *src = g_->d_work + o.off;
            hipError_t e;
            if (o.strided)
                e = hipMemcpy2DAsync(o.dst, o.dst_pitch, src, o.row, o.row, o.rows, hipMemcpyDeviceToHost, s);
            else if (transport_ == MIRROR)
                e = copy_d2h(o.dst, src, o.row, s, c_->device);
            else
                e = hipMemcpyAsync(o.dst, src, o.row, hipMemcpyDeviceToHost, s);
            RT_HIP(e, o.what);
        }
    }
    RT_HIP(hipStreamSynchronize(s), "stream sync");
    open_ = false;
    g_->stage_busy = false;
    if (h_)
        for (int i = 0; i < n_outs_; ++i) {
            const Out &o = outs_[i];
            for (uint64_t r = 0; r < o.rows; ++r)
                memcpy((uint8_t *)o.dst + r * o.dst_pitch, h_ + o.off + r * o.row, o.row);
        }
    return RT_OK;
}

// ---------------------------------------------------------------- contexts

// S-box from its definition (FIPS-197 §5.1.1): GF(2^8) inverse then affine map.
static void make_sbox(uint8_t s[256], uint8_t inv[256]) {
    uint8_t exp[256], log[256];
    uint8_t x = 1;
    for (int i = 0; i < 255; ++i) {          // generator 3
        exp[i] = x;
        log[x] = (uint8_t)i;
        x = (uint8_t)(x ^ (uint8_t)((x << 1) ^ ((x & 0x80) ? 0x1b : 0)));
    }
    for (int v = 0; v < 256; ++v) {
        uint8_t b = v ? exp[(255 - log[v]) % 255] : 0;
        uint8_t r = b;
        for (int i = 0; i < 4; ++i) {
            b = (uint8_t)((b << 1) | (b >> 7));
            r ^= b;
        }
        r ^= 0x63;
        s[v] = r;
        inv[r] = (uint8_t)v;
    }
}

extern "C" {

int rt_abi_version(void) { return RNSTOK_ABI_VERSION; }
const char *rt_last_error(void) { return g_err.c_str(); }

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

rt_ctx *rt_create(int device) {
    int n = rt_device_count();
    if (device < 0 || device >= n) {
        fail(RT_E_NODEV, "no HIP device " + std::to_string(device) + " (found " + std::to_string(n) + ")");
        return nullptr;
    }
    hipDeviceProp_t prop;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) {
        fail(RT_E_HIP, "hipGetDeviceProperties failed");
        return nullptr;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fail(RT_E_NODEV, std::string("librnstok is built for gfx950, device is ") + prop.gcnArchName);
        return nullptr;
    }
    static std::once_flag once;
    static hipError_t cfg = hipSuccess;
    std::call_once(once, [] { cfg = configure_kernels(); });
    if (cfg != hipSuccess) {
        hip_fail(cfg, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
        return nullptr;
    }
    rt_ctx *c = new rt_ctx();
    c->device = device;
    c->n_cu = prop.multiProcessorCount;
    uint8_t tables[512];
    make_sbox(tables, tables + 256);
    bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
              hipMalloc(&c->d_sbox, 512) == hipSuccess &&
              hipMalloc(&c->queues.d, 64ull * QueueRing::SLOTS) == hipSuccess &&
              hipMemcpy(c->d_sbox, tables, 512, hipMemcpyHostToDevice) == hipSuccess;
    for (uint32_t i = 0; ok && i < QueueRing::SLOTS; ++i)
        ok = hipEventCreateWithFlags(&c->queues.ev[i], hipEventDisableTiming) == hipSuccess;
    for (int i = 0; ok && i < N_STAGERS; ++i)
        ok = hipStreamCreateWithFlags(&c->stagers[i].stream, hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
        fail(RT_E_HIP, "context setup failed");
        rt_destroy(c);
        return nullptr;
    }
    // Key-record pool: keep freed memory for the next key set (no release
    // on synchronisation), reuse across streams through the stream-ordered
    // dependencies.  Without a pool the records come from the device's
    // default one.
    hipMemPoolProps props = {};
    props.allocType = hipMemAllocationTypePinned;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = device;
    if (hipMemPoolCreate(&c->pool, &props) == hipSuccess) {
        uint64_t keep = ~0ull;
        int on = 1;
        hipMemPoolSetAttribute(c->pool, hipMemPoolAttrReleaseThreshold, &keep);
        hipMemPoolSetAttribute(c->pool, hipMemPoolReuseFollowEventDependencies, &on);
        hipMemPoolSetAttribute(c->pool, hipMemPoolReuseAllowOpportunistic, &on);
        hipMemPoolSetAttribute(c->pool, hipMemPoolReuseAllowInternalDependencies, &on);
    } else {
        c->pool = nullptr;
        (void)hipGetLastError();
    }
    return c;
}

void rt_destroy(rt_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    for (auto &g : c->stagers) {
        if (g.stream) hipStreamSynchronize(g.stream);
        hipFree(g.d_work);
        if (g.h_stage) hipHostFree(g.h_stage);
        if (g.stream) hipStreamDestroy(g.stream);
    }
    if (c->stream) hipStreamSynchronize(c->stream);
    hipDeviceSynchronize();            // launches on callers' streams may still use the ring
    hipFree(c->d_sbox);
    hipFree(c->queues.d);
    if (c->h_link_report) hipHostFree(c->h_link_report);
    for (auto &e : c->queues.ev)
        if (e) hipEventDestroy(e);
    if (c->pool) hipMemPoolDestroy(c->pool);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

int rt_num_cus(const rt_ctx *c) { return c ? c->n_cu : 0; }

// ------------------------------------------------- key sets from raw keys

rt_keyset *rt_keyset_create_device(rt_ctx *c, const uint8_t *d_keys, uint32_t key_len, uint32_t n_keys,
                                   void *stream) {
    if (!c || !d_keys || n_keys == 0) {
        fail(RT_E_INVAL, "rt_keyset_create: null context/keys or zero keys");
        return nullptr;
    }
    if (check_key_len(key_len)) return nullptr;
    hipSetDevice(c->device);
    hipStream_t s = as_stream(stream);
    return keyset_on(c, key_len, n_keys, s, [&](rt_keyset *k) {
        return launch_key_setup(d_keys, key_len, n_keys, c->d_sbox, k->d_rec, s);
    });
}

// Host keys: staged through a lane's pinned mirror and workspace; the key set
// is built on that lane's stream and this call does not block (later launches
// on other streams wait on the key set's ready event).
rt_keyset *rt_keyset_create(rt_ctx *c, const uint8_t *keys, uint32_t key_len, uint32_t n_keys) {
    if (!c || !keys || n_keys == 0) {
        fail(RT_E_INVAL, "rt_keyset_create: null context/keys or zero keys");
        return nullptr;
    }
    if (check_key_len(key_len)) return nullptr;
    const uint64_t bytes = (uint64_t)n_keys * key_len;
    HostCall hc(c, HostCall::MIRROR);
    const uint64_t o_keys = hc.add(bytes);
    if (hc.open()) return nullptr;
    hc.put(o_keys, keys, bytes, "key upload failed");
    if (hc.send(bytes)) return nullptr;
    hipStream_t s = hc.stream();
    rt_keyset *k = keyset_on(c, key_len, n_keys, s, [&](rt_keyset *ks) {
        return launch_key_setup(hc.dev<uint8_t>(o_keys), key_len, n_keys, c->d_sbox, ks->d_rec, s);
    });
    // the mirror holds the keys: return with the work queued.  The caller's
    // pageable keys were read in place: the frame synchronises on the way out
    if (k && hc.mirrored()) hc.leave_queued();
    return k;
}

// No synchronisation: the records go back to the pool on the reclaim stream
// once the key setup and the last launch on every stream that used them are
// done.
void rt_keyset_destroy(rt_keyset *k) {
    if (!k) return;
    rt_ctx *c = k->ctx;
    hipSetDevice(c->device);
    hipStreamWaitEvent(c->stream, k->ready, 0);
    {
        std::lock_guard<std::mutex> g(k->mu);
        for (auto &u : k->uses) {
            hipStreamWaitEvent(c->stream, u.second, 0);
            hipEventDestroy(u.second);
        }
        k->uses.clear();
    }
    hipFreeAsync(k->d_rec, c->stream);
    hipEventDestroy(k->ready);
    delete k;
}

uint32_t rt_keyset_size(const rt_keyset *k) { return k ? k->n_keys : 0; }

// ------------------------------------------------------------------ memory

void *rt_device_alloc(rt_ctx *c, uint64_t bytes) {
    if (!c) return nullptr;
    void *p = nullptr;
    hipSetDevice(c->device);
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) {
        fail(RT_E_NOMEM, "hipMalloc failed");
        return nullptr;
    }
    return p;
}
void rt_device_free(rt_ctx *c, void *p) {
    if (c) hipSetDevice(c->device);
    hipFree(p);
}
void *rt_host_alloc(uint64_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        fail(RT_E_NOMEM, "hipHostMalloc failed");
        return nullptr;
    }
    return p;
}
void rt_host_free(void *p) { hipHostFree(p); }
int rt_memcpy_h2d(rt_ctx *c, void *dst, const void *src, uint64_t bytes, void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    RT_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, as_stream(stream)), "H2D");
    return RT_OK;
}
int rt_memcpy_d2h(rt_ctx *c, void *dst, const void *src, uint64_t bytes, void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    RT_HIP(copy_d2h(dst, src, bytes, as_stream(stream), c->device), "D2H");
    return RT_OK;
}
int rt_memcpy_d2h_upto(rt_ctx *c, void *dst, const void *src, uint64_t max_bytes, const uint64_t *d_bytes,
                       void *stream) {
    if (!c || !dst || !src || !d_bytes) return fail(RT_E_INVAL, "rt_memcpy_d2h_upto: null argument");
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    hipPointerAttribute_t ad, as, an;
    if (!(query(&ad, dst) && ad.type == hipMemoryTypeHost && ad.devicePointer && query(&as, src) &&
          as.type == hipMemoryTypeDevice && as.device == c->device))
        return fail(RT_E_INVAL, "rt_memcpy_d2h_upto: dst must be pinned host memory and src device memory of the "
                                "context's GPU");
    if (!(query(&an, d_bytes) && an.type == hipMemoryTypeDevice && an.device == c->device))
        return fail(RT_E_INVAL, "rt_memcpy_d2h_upto: d_bytes must be device memory of the context's GPU");
    RT_HIP(launch_store_host((uint8_t *)ad.devicePointer, (const uint8_t *)src, max_bytes, as_stream(stream), d_bytes),
           "D2H");
    return RT_OK;
}
int rt_clock_stamps(rt_ctx *c, uint64_t *acc) {
    if (!c) return fail(RT_E_INVAL, "null context");
    if (acc) {
        RT_HIP(hipSetDevice(c->device), "hipSetDevice");
        hipPointerAttribute_t at;
        if (((uintptr_t)acc & 7u) || !(query(&at, acc) && at.type == hipMemoryTypeDevice && at.device == c->device))
            return fail(RT_E_INVAL, "rt_clock_stamps: acc must be 8-byte aligned device memory of the context's GPU");
    }
    c->clk.store((unsigned long long *)acc, std::memory_order_release);
    return RT_OK;
}
int rt_stream_sync(rt_ctx *c, void *stream) {
    if (!c) return fail(RT_E_INVAL, "null context");
    RT_HIP(hipSetDevice(c->device), "hipSetDevice");
    RT_HIP(hipStreamSynchronize(as_stream(stream)), "stream sync");
    return RT_OK;
}

}  // extern "C"

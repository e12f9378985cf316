// capi_internal.h — what the C-ABI's translation units (capi_*.hip) share:
// the context and key-set records, error reporting, the envelope of a launch
// that reads a key set, and HostCall, the staging frame of every host-pointer
// entry point.  Definitions live in capi_runtime.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rnstok.h"
#include "token_device.h"
#include "token_launch.h"

using namespace rnstok;

// ------------------------------------------------------------------ errors
// No exceptions cross the boundary: negative RT_E_* codes plus rt_last_error().
int fail(int code, const std::string &msg);
int hip_fail(hipError_t e, const char *what);
#define RT_HIP(call, what)                         \
    do {                                           \
        hipError_t e_ = (call);                    \
        if (e_ != hipSuccess) return hip_fail(e_, what); \
    } while (0)
#define RT_TRY(call)              \
    do {                          \
        int rc_ = (call);         \
        if (rc_) return rc_;      \
    } while (0)

// A host-staging lane: a private stream, a device workspace and a pinned
// mirror of it.  The context keeps N_STAGERS of them, so host calls from
// several threads (e.g. one reader thread per interface) run concurrently
// instead of queueing on one lock; a call takes a free lane or waits for one.
struct Stager {
    std::mutex mu;
    hipStream_t stream = nullptr;
    uint8_t *d_work = nullptr;     // host-path workspace
    uint64_t work_cap = 0;
    // Pinned mirror of the workspace for token host calls up to STAGE_MAX
    // bytes: the caller's arrays are gathered here and cross PCIe as one copy
    // each way.  A pageable copy pays a driver staging round trip per array
    // (6 of them per encrypt), which dominates a one-packet Token.encrypt.
    uint8_t *h_stage = nullptr;
    uint8_t *h_stage_dev = nullptr;    // its device-side address (GPU stores, launch_store_host)
    uint64_t stage_cap = 0;
    bool stage_busy = false;       // a copy from h_stage may still be queued on `stream`
};
// 8 lanes (round 6): one Token call per packet from 16 threads, 44 600 ->
// 73 000 calls/s against 4 lanes (two runs each, profiles/r06_percall_lanes.txt;
// one thread unchanged at 19 000); streams beyond the box's four hardware
// queues still overlap the host-side waits of concurrent calls.  Pinned
// staging grows on demand, at most 8 MiB per lane.
static constexpr int N_STAGERS = 8;
static constexpr uint64_t STAGE_MAX = 8ull << 20;

// Chunk counters for the token kernels' dynamic packet loop (ragged uniform
// batches): one 64-B slot per launch.  A slot is handed out again only after
// the stream of its next user waits on the event recorded after its previous
// launch, so a counter is never zeroed or advanced while an earlier launch
// (on any stream) may still read it.  No lock is held across the launch:
// each slot has its own busy flag, taken by compare-and-swap at acquire() and
// dropped at release(), so threads launching on different streams only ever
// contend for one atomic increment (the round-robin cursor).  A thread that
// finds every slot held falls back to the static stride (correct, less
// balanced).
struct QueueRing final : SpareQueue {
    static constexpr uint32_t SLOTS = 256;
    uint32_t *d = nullptr;
    hipEvent_t ev[SLOTS] = {};
    bool recorded[SLOTS] = {};                 // read and written by the slot's holder only
    std::atomic<uint32_t> next{0};
    std::atomic<uint32_t> busy[SLOTS] = {};
    uint32_t *acquire(hipStream_t s, uint32_t *slot) override;
    void release(hipStream_t s, uint32_t slot) override;
};

struct rt_ctx {
    int device = 0;
    int n_cu = 0;
    // Reclaim stream: a destroyed key set's records are freed here, after
    // the events of their last launches (no host or device-wide sync).
    hipStream_t stream = nullptr;
    uint8_t *d_sbox = nullptr;     // 512 B: S-box || inverse S-box
    // Stream-ordered pool for key records: a per-packet key set per batch
    // (Identity.py:837-846) reuses the memory of the previous one without a
    // hipMalloc/hipFree (both synchronise the device) on the host timeline.
    hipMemPool_t pool = nullptr;
    Stager stagers[N_STAGERS];
    std::atomic<uint32_t> stager_rr{0};
    QueueRing queues;
    // rt_clock_stamps: the launch-clock words the token kernels add to, or null
    std::atomic<unsigned long long *> clk{nullptr};
    // Link tables (capi_link.hip): LINK_REPORTS mapped host words into which a
    // table's rebuild writes ticket << 32 | live entries.  They live as long as
    // the context, so a rebuild still in flight when its table is destroyed
    // writes into memory that exists; a table believes a word only when it
    // carries the ticket of that table's latest rebuild.
    static constexpr uint32_t LINK_REPORTS = 1024;
    std::mutex link_mu;
    uint64_t *h_link_report = nullptr, *d_link_report = nullptr;
    uint32_t link_next = 0;
    std::atomic<uint32_t> link_ticket{0};
};

struct rt_keyset {
    rt_ctx *ctx = nullptr;
    uint32_t key_len = 0, n_keys = 0;
    int nr = 0;
    uint32_t *d_rec = nullptr;
    hipStream_t home = nullptr;    // the stream the records were built on
    hipEvent_t ready = nullptr;    // recorded on `home` after the key setup
    // The last launch on each stream that read the records: destroy orders
    // the free after all of them.
    std::mutex mu;
    std::vector<std::pair<hipStream_t, hipEvent_t>> uses;
};

// Device-API streams: the caller's hipStream_t; NULL is HIP's null stream
// (torch's default stream), never the context's private staging stream.
inline hipStream_t as_stream(void *stream) { return (hipStream_t)stream; }

int check_keyset(const rt_keyset *k);
int check_key_len(uint32_t key_len);        // 32 or 64, else the reference's message (Token.py:72)
// Work enqueued on `s` from here on sees the key set's records.
hipError_t after_setup(const rt_keyset *k, hipStream_t s);
// The launch just enqueued on `s` reads the records.
hipError_t note_use(rt_keyset *k, hipStream_t s);

// A launch that reads k's records, on the caller's stream: ordered after the
// key setup, and recorded so that rt_keyset_destroy frees the records after
// it.  The caller has passed check_keyset(k) and its own argument checks.
template <class Launch>
int launch_with_keys(const rt_keyset *k, void *stream, const char *what, Launch launch) {
    hipStream_t s = as_stream(stream);
    RT_HIP(hipSetDevice(k->ctx->device), "hipSetDevice");
    RT_HIP(after_setup(k, s), "wait for key setup");
    RT_HIP(launch(s), what);
    RT_HIP(note_use(const_cast<rt_keyset *>(k), s), "record key set use");
    return RT_OK;
}

// A key set whose records are allocated and built on stream s.  `build`
// enqueues the kernel(s) that write k->d_rec.
hipError_t rec_alloc(rt_ctx *c, uint64_t bytes, uint32_t **p, hipStream_t s);
template <class Build>
rt_keyset *keyset_on(rt_ctx *c, uint32_t key_len, uint32_t n_keys, hipStream_t s, Build build) {
    rt_keyset *k = new rt_keyset();
    k->ctx = c;
    k->key_len = key_len;
    k->n_keys = n_keys;
    k->nr = key_len == 64 ? 14 : 10;
    k->home = s;
    hipError_t e = hipEventCreateWithFlags(&k->ready, hipEventDisableTiming);
    if (e == hipSuccess) e = rec_alloc(c, (uint64_t)n_keys * REC_WORDS * 4, &k->d_rec, s);
    if (e != hipSuccess) {
        fail(RT_E_NOMEM, std::string("key table allocation failed: ") + hipGetErrorString(e));
        if (k->ready) hipEventDestroy(k->ready);
        delete k;
        return nullptr;
    }
    if ((e = build(k)) != hipSuccess || (e = hipEventRecord(k->ready, s)) != hipSuccess) {
        hip_fail(e, "key setup launch");
        hipStreamSynchronize(s);
        hipFreeAsync(k->d_rec, s);
        hipEventDestroy(k->ready);
        delete k;
        return nullptr;
    }
    return k;
}

// Device -> host copy on stream s: GPU stores when dst is pinned and src is
// memory of `device`, hipMemcpyAsync otherwise (capi_runtime.hip).
bool query(hipPointerAttribute_t *at, const void *p);
hipError_t copy_d2h(void *dst, const void *src, uint64_t bytes, hipStream_t s, int device);

// The frame of one host-pointer call.  It holds a staging lane (a free one,
// or the caller's round-robin one once it is free) from construction to
// destruction, and the call states each region of the lane's workspace once:
// add() reserves it, open() readies the lane, put() and send() fill it, the
// call launches on stream() with dev<T>() pointers, get() and finish() bring
// the outputs back and synchronise.
//
// MIRROR (the token calls and rt_keyset_create): up to STAGE_MAX bytes the
// inputs are gathered in the lane's pinned mirror and cross PCIe as one copy,
// and the outputs come back by one store kernel over the range the get()s
// span; above that, or when the pinned allocation fails, each array is copied
// from and to the caller's memory.  PER_ARRAY: always the latter.
// open(true), for one-packet calls: when the mirror is there the kernel works
// on it in place (dev<T>() resolves to its device address) and nothing is
// copied; see host_direct in capi_token.hip.
//
// A call that returns before finish() with work queued leaves through the
// destructor, which synchronises the lane's stream first: neither the caller's
// arrays nor the lane's buffers are in flight when the next call takes the lane.
class HostCall {
public:
    enum Transport { PER_ARRAY, MIRROR };
    HostCall(rt_ctx *c, Transport t);
    ~HostCall();
    HostCall(const HostCall &) = delete;
    HostCall &operator=(const HostCall &) = delete;

    // Reserves max(bytes, 1) bytes (a possibly empty region still has an
    // address): its offset, 16-byte aligned.
    uint64_t add(uint64_t bytes) {
        const uint64_t o = end_;
        end_ = (o + std::max<uint64_t>(bytes, 1) + 15) & ~15ull;
        return o;
    }
    uint64_t total() const { return end_; }
    int open(bool one_packet = false);

    // Inputs.  A failed copy is remembered and reported by send().
    void put(uint64_t off, const void *src, uint64_t bytes, const char *what);
    void put_rows(uint64_t off, const void *src, uint64_t src_pitch, uint64_t row, uint64_t rows, const char *what);
    int send(uint64_t upto = 0);

    hipStream_t stream() const { return g_->stream; }
    bool mirrored() const { return h_ != nullptr; }
    template <class T>
    T *dev(uint64_t off) const {
        return (T *)((direct_ ? g_->h_stage_dev : g_->d_work) + off);
    }

    // Outputs, copied to the caller by finish().
    void get(void *dst, uint64_t off, uint64_t bytes, const char *what) {
        if (bytes) outs_[n_outs_++] = Out{dst, bytes, off, bytes, 1, false, what};
    }
    void get_rows(void *dst, uint64_t dst_pitch, uint64_t off, uint64_t row, uint64_t rows, const char *what) {
        if (row && rows) outs_[n_outs_++] = Out{dst, dst_pitch, off, row, rows, true, what};
    }
    int finish();
    // rt_keyset_create: return with the mirror's upload and the key setup
    // queued; the lane's next user waits for them before it touches the mirror.
    void leave_queued() { open_ = false; }

private:
    struct Out {
        void *dst;
        uint64_t dst_pitch, off, row, rows;
        bool strided;              // a hipMemcpy2DAsync when copied from the workspace
        const char *what;
    };
    rt_ctx *c_;
    Stager *g_ = nullptr;
    const Transport transport_;
    uint64_t end_ = 0;
    uint8_t *h_ = nullptr;         // the pinned mirror, when this call goes through it
    bool direct_ = false;          // the kernel reads and writes the mirror itself
    bool open_ = false;            // work may be queued on the lane's stream
    hipError_t put_err_ = hipSuccess;
    const char *put_what_ = nullptr;
    Out outs_[3];
    int n_outs_ = 0;
};

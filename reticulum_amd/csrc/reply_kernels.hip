// reply_kernels.hip — the send side of a read: what the stages of the inbound
// path leave to be transmitted (the LRPROOFs of rt_link_accept, the LINK PROOFs
// of rt_link_prove, the PROOFs of rt_destination_deliver), gathered from their
// sparse per-frame rows into one dense batch that rt_ifac_sign, rt_ifac_mask
// and rt_hdlc_frame_counted turn into the byte stream for the socket.  The
// reference sends each of them on the interface its frame came in on, in the
// order of its loop over the frames (Packet.prove / Link.prove with the
// receiving interface attached, Transport.py:1069-1104, 1199-1356), so one read
// has one reply stream.  DESIGN.md §4.3k.
//
// A source is a matrix of rows with a length per frame; 0 means nothing for
// that frame.  The replies are ordered by frame, then by source.
//   k_reply_count   one lane per frame, RG_BLOCK frames per workgroup: the
//       workgroup's replies into part[b].
//   k_scan_parts    (wire_kernels.hip) places the workgroups.
//   k_reply_write   the same lanes rank their frame's replies with
//       block_exclusive_scan and list them in LDS; then eight lanes move a row,
//       one 16-byte unit each, so a wave stores eight whole 128-byte lines per
//       instruction; also the per-reply columns, the sentinels past the replies
//       and the counts.
//   k_reply_hashes  one lane per gathered row: its packet hash, for the hash
//       list to remember what was sent (Transport.py:1343-1345).
// No kernel waits for another workgroup.
#include "wire_device.h"
#include "token_launch.h"
#include "reply_host.h"

namespace rnstok {

namespace {

static_assert(RG_BLOCK == SCAN_BLOCK, "k_scan_parts places workgroups of SCAN_BLOCK items");

// the length source s has for frame k: 0 for nothing
template <uint32_t S>
__device__ __forceinline__ uint32_t reply_len_of(const ReplyGatherArgs &a, uint64_t k) {
    if (S >= a.n_sources || k >= a.n) return 0u;
    const int32_t L = a.len[S][k];
    return reply_len_ok(L, a.width[S]) ? (uint32_t)L : 0u;
}

__device__ __forceinline__ void frame_lens(const ReplyGatherArgs &a, uint64_t k, uint32_t L[RG_MAX_SOURCES]) {
    L[0] = reply_len_of<0>(a, k);
    L[1] = reply_len_of<1>(a, k);
    L[2] = reply_len_of<2>(a, k);
    L[3] = reply_len_of<3>(a, k);
}

__global__ __launch_bounds__(RG_BLOCK) void k_reply_count(const ReplyGatherArgs a) {
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * RG_BLOCK + threadIdx.x;
    uint32_t L[RG_MAX_SOURCES];
    frame_lens(a, k, L);
    uint32_t c = 0;                  // the wave's replies
#pragma unroll
    for (uint32_t s = 0; s < RG_MAX_SOURCES; ++s) c += (uint32_t)__popcll(__ballot(L[s] != 0u));
    if ((threadIdx.x & 63u) == 0u && c) atomicAdd(&total, c);
    __syncthreads();
    if (threadIdx.x == 0) a.part[blockIdx.x] = total;
}

// an entry of the workgroup's list: the frame's lane, the source, the length (1..128)
__device__ __forceinline__ uint32_t entry_of(uint32_t t, uint32_t s, uint32_t L) { return t | (s << 16) | (L << 24); }

__global__ __launch_bounds__(RG_BLOCK) void k_reply_write(const ReplyGatherArgs a) {
    __shared__ uint32_t entry[RG_BLOCK * RG_MAX_SOURCES];
    const uint32_t t = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * RG_BLOCK, k = first + t;
    const uint32_t nb = reply_blocks(a.n);
    const uint64_t found = a.part[nb], written = reply_written(found, a.cap);
    if (blockIdx.x < nb) {                              // a workgroup with frames (the same for all its lanes)
        uint32_t L[RG_MAX_SOURCES];
        frame_lens(a, k, L);
        const uint32_t c = (L[0] != 0u) + (L[1] != 0u) + (L[2] != 0u) + (L[3] != 0u);
        uint64_t tot64;
        uint32_t at = (uint32_t)block_exclusive_scan(c, &tot64);
        const uint32_t tot = (uint32_t)tot64;
#pragma unroll
        for (uint32_t s = 0; s < RG_MAX_SOURCES; ++s)
            if (L[s]) entry[at++] = entry_of(t, s, L[s]);
        __syncthreads();
        const uint64_t base = a.part[blockIdx.x];       // the replies of the workgroups before this one
        // the columns, one reply per lane
        for (uint32_t li = t; li < tot && base + li < a.cap; li += RG_BLOCK) {
            const uint32_t e = entry[li];
            const uint64_t r = base + li;
            a.reply_len[r] = (int32_t)(e >> 24);
            a.reply_frame[r] = (int32_t)(first + (e & 0xFFFFu));
            a.reply_source[r] = (uint8_t)((e >> 16) & 0xFFu);
        }
        // the rows, eight lanes each: unit q of the row, zeros past the reply's
        // end, so every row is written as one whole line
        const uint32_t q = t & (RG_LANES_PER_ROW - 1u);
        for (uint32_t li = t / RG_LANES_PER_ROW; li < tot && base + li < a.cap; li += RG_ROWS_PER_PASS) {
            const uint32_t e = entry[li], s = (e >> 16) & 0xFFu, len = e >> 24;
            const uint8_t *rows = a.rows[0];
            uint64_t stride = a.stride[0];
#pragma unroll
            for (uint32_t j = 1; j < RG_MAX_SOURCES; ++j)
                if (s == j) {
                    rows = a.rows[j];
                    stride = a.stride[j];
                }
            const uint8_t *src = rows + (first + (e & 0xFFFFu)) * stride;
            const u32x4 v = 16u * q < len ? ld16_upto(src, 16u * q, len) : u32x4{0u, 0u, 0u, 0u};
            st16(a.out + (base + li) * RG_ROW + 16u * q, v);
        }
    }
    if (k < a.cap && k >= written) {                    // past the replies: nothing to send
        a.reply_len[k] = 0;
        a.reply_frame[k] = -1;
        a.reply_source[k] = 0xFFu;
    }
    if (k == 0) {
        a.reply_counts[0] = (int64_t)written;
        a.reply_counts[1] = (int64_t)found;
    }
}

__global__ __launch_bounds__(256) void k_reply_hashes(const uint8_t *rows, uint64_t stride, const int32_t *len,
                                                      const int64_t *counts, uint32_t cap, uint8_t *hashes,
                                                      uint8_t *mask) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cap) return;
    const int64_t c = counts[0];
    const uint8_t *raw = rows + (uint64_t)j * stride;
    bool ok = (int64_t)j < c && reply_len_ok(len[j], RG_ROW);
    // a packet has its context byte (Packet.py:242-268): 19 bytes, or 35 with a transport id
    if (ok) ok = (uint32_t)len[j] > (((raw[0] >> 6) & 1u) ? 34u : 18u);
    mask[j] = ok ? 1 : 0;
    if (!ok) return;
    uint32_t d[8];
    packet_hash_words(raw, (uint32_t)len[j], d);
    st16(hashes + 32ull * j, u32x4{bswap(d[0]), bswap(d[1]), bswap(d[2]), bswap(d[3])});
    st16(hashes + 32ull * j + 16, u32x4{bswap(d[4]), bswap(d[5]), bswap(d[6]), bswap(d[7])});
}

}  // namespace

hipError_t launch_reply_gather(const ReplyGatherArgs &a, hipStream_t s) {
    const uint32_t nb = reply_count_grid(a.n);
    if (nb) hipLaunchKernelGGL(k_reply_count, dim3(nb), dim3(RG_BLOCK), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = launch_scan_parts(a.part, nb, s)) != hipSuccess) return e;        // with nb = 0: part[0] = 0
    hipLaunchKernelGGL(k_reply_write, dim3(reply_write_grid(a.n, a.cap)), dim3(RG_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_reply_hashes(const uint8_t *rows, uint64_t stride, const int32_t *len, const int64_t *counts,
                               uint32_t cap, uint8_t *hashes, uint8_t *mask, hipStream_t s) {
    if (cap == 0) return hipSuccess;
    hipLaunchKernelGGL(k_reply_hashes, dim3((cap + 255) / 256), dim3(256), 0, s, rows, stride, len, counts, cap,
                       hashes, mask);
    return hipGetLastError();
}

}  // namespace rnstok

// reply_host.h — the host's planning for gathering the replies of a read
// (reply_kernels.hip): the workspace of a call over n frames and S sources, the
// grids of its kernels, and the arithmetic of the counts.  Plain C++ with no
// HIP in it, for the kernels and the host alike, so that tests/reply_host/ can
// build it alone under the sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RG_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define RG_FN inline __attribute__((always_inline))
#endif

namespace rnstok {

constexpr uint32_t RG_BLOCK = 1024;            // frames per workgroup: SCAN_BLOCK, what k_scan_parts places
constexpr uint32_t RG_MAX_SOURCES = 4;
constexpr uint32_t RG_ROW = 128;               // bytes of a gathered row, and the longest reply
constexpr uint32_t RG_LANES_PER_ROW = RG_ROW / 16;               // one 16-byte unit per lane
constexpr uint32_t RG_ROWS_PER_PASS = RG_BLOCK / RG_LANES_PER_ROW;
constexpr uint32_t RG_MAX_FRAMES = 0x7FFFFFFFu;                  // reply_frame is an int32

RG_FN bool reply_sources_ok(uint32_t S) { return S >= 1 && S <= RG_MAX_SOURCES; }

// workgroups that cover n items, one per thread (n up to 2^32 - 1: at most 2^22)
RG_FN uint32_t reply_blocks(uint64_t n) { return (uint32_t)((n + RG_BLOCK - 1) / RG_BLOCK); }

// The count kernel has one workgroup per RG_BLOCK frames; the write kernel also
// clears the entries past the replies, so its grid covers the frames and the
// capacity, whichever are more, and is never empty (thread 0 writes the counts).
RG_FN uint32_t reply_count_grid(uint32_t n) { return reply_blocks(n); }
RG_FN uint32_t reply_write_grid(uint32_t n, uint32_t cap) {
    const uint32_t g = reply_blocks(n > cap ? n : cap);
    return g ? g : 1u;
}

// The workspace: one 64-bit word per workgroup of frames and one for their
// sum, rounded up to 16 bytes.  The sources do not change it; a bad S gives 0.
RG_FN uint64_t reply_gather_workspace_bytes(uint32_t n, uint32_t S) {
    if (!reply_sources_ok(S)) return 0;
    return (8ull * ((uint64_t)reply_blocks(n) + 1) + 15) & ~15ull;
}

// A length the gather takes: 1 .. min(RG_ROW, the source's row width).
RG_FN bool reply_len_ok(int32_t len, uint32_t width) {
    return len >= 1 && (uint32_t)len <= (width < RG_ROW ? width : RG_ROW);
}

// reply_counts[0] from the replies found and the capacity.
RG_FN uint64_t reply_written(uint64_t found, uint32_t cap) { return found < cap ? found : cap; }

}  // namespace rnstok

// The conventions of the device logs a captured step appends to (evf_eval_log.hip, evf_train_log.hip, evf_activity.hip), defined
// ONCE here:
//
//   the row    ONE int64 word in DEVICE memory, read by the kernel, names the row a launch fills; a row outside 0 .. nrows - 1 is
//              a defined no-op: nothing is stored (evf_log_row).  The host answers EVF_EINVAL, before any launch, for a
//              destination that cannot hold the row (evf_log_dest_ok).
//   the walk   a source is only 4-byte aligned: a scalar peel up to the first 16-byte boundary, 16-byte trips, at most three tail
//              elements (evf_walk16).
//   the count  exact integer counts -- set bits or nonzero floats (act_one) --, reduced by a wave butterfly and the four waves of
//              a block added in index order (evf_block_count): the same bits from call to call.
//
// Plain launches on one stream, no atomics, no ticket; nothing is allocated or copied, so every call can be captured.
// Header only, nothing but inline definitions: a log source also compiles on its own.
#pragma once
#include "evf_common.h"

// The row `row[0] * mul + add`, formed in 128 bits (any row word times any multiplier is defined), or -1 when it lies outside
// 0 .. nrows - 1.  A uniform load: every thread of every block reads the one word.
__device__ __forceinline__ long long evf_log_row(const long long* __restrict__ row, long long mul, long long add, long long nrows) {
  const __int128 r = (__int128)row[0] * mul + add;
  return (r < 0 || r >= nrows) ? -1 : (long long)r;
}

// Host: `need` floats at `offset` fit a row of `row_floats` floats of a log of `nrows` rows, the log is 4-byte and the row word
// 8-byte aligned.  (A launcher that lays its row out itself leaves the last three arguments alone.)
static inline bool evf_log_dest_ok(const void* row, int64_t nrows, const void* log, int64_t row_floats = 1, int64_t offset = 0,
                                   int64_t need = 0) {
  return row && log && nrows >= 1 && row_floats >= 1 && offset >= 0 && need >= 0 && offset + need <= row_floats &&
         !((uintptr_t)log & 3u) && !((uintptr_t)row & 7u);
}

// f(g[i]) for the elements i in [0, len) behind g (4-byte aligned) that fall to this thread: the 16-byte groups first,
// first + stride, ... behind the peel, and -- `ends`: uniform over the block -- thread t element t of the peel and of the tail.
// In the order peel, trips, tail.  UNROLL > 0: `#pragma unroll UNROLL` on the trips.
template <int UNROLL = 0, typename T, typename I, typename F>
__device__ __forceinline__ void evf_walk16(const T* __restrict__ g, I len, I first, I stride, bool ends, F f) {
  typedef HIP_vector_type<T, 4> V4;  // (float4, uint4)
  static_assert(sizeof(T) == 4, "evf_walk16: 4-byte elements");
  I head = (I)((4u - (unsigned)(((uintptr_t)g >> 2) & 3u)) & 3u);
  head = head < len ? head : len;
  const I n4 = (len - head) >> 2, t0 = head + 4 * n4;
  const V4* g4 = (const V4*)(g + head);
  auto trip = [&](I i) {
    const V4 q = g4[i];
    f(q.x), f(q.y), f(q.z), f(q.w);
  };
  if (ends && (I)threadIdx.x < head) f(g[threadIdx.x]);
  if constexpr (UNROLL > 0) {
#pragma unroll UNROLL
    for (I i = first; i < n4; i += stride) trip(i);
  } else {
    for (I i = first; i < n4; i += stride) trip(i);
  }
  if (ends && t0 + (I)threadIdx.x < len) f(g[t0 + threadIdx.x]);  // (at most three)
}

// What one 4-byte word adds to a count.  WORDS: its set bits; else torch.ne(0) of a float32 on the bits -- -0.0 is zero, NaN,
// +-inf and every denormal are not, whatever the denormal mode.
template <bool WORDS>
__device__ __forceinline__ unsigned act_one(unsigned w) {
  return WORDS ? (unsigned)__popc(w) : ((w & 0x7fffffffu) != 0u ? 1u : 0u);
}

// Exact count of a block of 256 threads: the wave butterfly, then the four waves added in index order; valid in thread 0.
__device__ __forceinline__ unsigned evf_block_count(unsigned cnt, unsigned* red /* 4 words of LDS */) {
  cnt = evf_wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  return threadIdx.x == 0 ? ((red[0] + red[1]) + red[2]) + red[3] : 0u;
}

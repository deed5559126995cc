// Spike-activity log of an evaluation pass (activity.ActivityLog): the reference's `model(..., log=True)` -- per layer the fraction
// of nonzero outputs -- as EXACT integer counts, per source and per sample, appended to a device log at the row the host named
// (the device-log conventions, evf_log.h).
//
//   evf_activity_at   up to 16 sources [B][n_k] in ONE launch: float32 elements with x != 0 (EVF_ACT_FLOAT) or set bits of int32
//                     words (EVF_ACT_WORDS) -> log[row][k][b][part], uint32.
//
// One plain launch, no atomics, no ticket, no workspace: block (part, k, b) counts its contiguous share, reduces it in the block and
// stores ONE word; the host adds the parts in int64.  Integer sums: the same bits from call to call.  Nothing is allocated or
// copied, so the call can be captured.  A row outside 0 .. nrows - 1 leaves the log untouched.
#include "evf_log.h"

#define ACT_THREADS 256
#define ACT_MAX_SRC 16
#define ACT_MAX_N ((1LL << 27) - 1)  // 32 bits a word: a block's count stays below 2^32 even with ONE part
// Elements per block before a source is cut into a further part, and the most parts.
// The split was chosen by timing the call inside a replayed graph (16 calls a graph) at the two evaluation shapes, B = 1 and nine
// sources each (tools/eval_activity_rate.py, profiles/eval_activity_rate.json; MI355X, microseconds per call):
//   elements a block   180 x 240 (parts, us)   256 x 256 (parts, us)
//   one part                  1   6.09                1   7.56
//   65536                     2   4.46                2   5.14
//   32768                     3   4.10                4   4.00
//   16384                     6   3.72                8   3.47
//   8192                     11   3.75               16   3.16
//   4096                     22   3.37               32   3.29
//   2048                     43   3.31               64   3.38
//   1024                     85   3.37              128   3.81
// One block per (source, sample) leaves nine blocks on 256 CUs and costs twice the time; from 16384 elements a block down the
// call sits on the floor of a launch inside a graph (3.1 to 3.8 us, differences of the size of the run-to-run spread), and more
// parts only make the row longer.  8192 it is: 16 float4 trips a thread at most, 11 and 16 words per (source, sample) to read.
#ifndef ACT_CHUNK
#define ACT_CHUNK 8192
#endif
#ifndef ACT_MAX_PARTS
#define ACT_MAX_PARTS 64
#endif

struct ActSrc {
  const unsigned* src[ACT_MAX_SRC];
  int n[ACT_MAX_SRC];
  unsigned words;  // bit k: source k is EVF_ACT_WORDS
};

// Elements [0, len) behind g (4-byte aligned), counted by the 256 threads of a block (evf_walk16; four trips unrolled: the times
// in the table above).
template <bool WORDS>
__device__ __forceinline__ unsigned act_count(const unsigned* __restrict__ g, int len) {
  unsigned cnt = 0;
  evf_walk16<4>(g, len, (int)threadIdx.x, ACT_THREADS, true, [&](unsigned w) { cnt += act_one<WORDS>(w); });
  return cnt;
}

// Block (p, k, b): elements [p * share, min((p + 1) * share, n_k)) of sample b of source k, share = ceil(n_k / parts) rounded up
// to whole 16-byte groups.  A block whose share is empty stores 0: every word of the row is written.
__global__ void __launch_bounds__(ACT_THREADS) k_activity_at(ActSrc as, const long long* __restrict__ row, long long row_mul,
                                                             long long row_add, long long nrows, unsigned* __restrict__ log) {
  __shared__ unsigned red[ACT_THREADS / 64];
  const long long r = evf_log_row(row, row_mul, row_add, nrows);
  if (r < 0) return;
  const int parts = gridDim.x, p = blockIdx.x, k = blockIdx.y, b = blockIdx.z;
  const int n = as.n[k];
  const int share = (((n + parts - 1) / parts) + 3) & ~3;
  const long long a = (long long)p * share;
  unsigned cnt = 0;
  if (a < n) {
    const int len = (int)(a + share < n ? share : n - a);
    const unsigned* g = as.src[k] + (long long)b * n + a;
    cnt = ((as.words >> k) & 1u) ? act_count<true>(g, len) : act_count<false>(g, len);
  }
  cnt = evf_block_count(cnt, red);
  if (threadIdx.x == 0) log[(((r * gridDim.y + k) * gridDim.z + b) * parts) + p] = cnt;
}

extern "C" int evf_activity_parts(int64_t n_max) {
  if (n_max < 1 || n_max > ACT_MAX_N) return EVF_EINVAL;
  const int64_t parts = (n_max + ACT_CHUNK - 1) / ACT_CHUNK;
  return (int)(parts < ACT_MAX_PARTS ? parts : ACT_MAX_PARTS);
}

extern "C" int evf_activity_at(const void* const* src, const int* kind, const int64_t* n, int nsrc, int B, const int64_t* row,
                               int64_t row_mul, int64_t row_add, int64_t nrows, uint32_t* log, void* stream) {
  if (!src || !kind || !n || !evf_log_dest_ok(row, nrows, log)) return EVF_EINVAL;  // (the row is [nsrc][B][parts]: sized here)
  if (nsrc < 1 || nsrc > ACT_MAX_SRC || B < 1 || B > 65535 || row_mul < 0 || row_add < 0) return EVF_EINVAL;
  ActSrc as;
  as.words = 0;
  int64_t n_max = 1;
  for (int k = 0; k < ACT_MAX_SRC; ++k) {
    as.src[k] = nullptr;
    as.n[k] = 0;
    if (k >= nsrc) continue;
    if (!src[k] || ((uintptr_t)src[k] & 3u)) return EVF_EINVAL;
    if (kind[k] != EVF_ACT_FLOAT && kind[k] != EVF_ACT_WORDS) return EVF_EINVAL;
    if (n[k] < 1 || n[k] > ACT_MAX_N) return EVF_EINVAL;
    as.src[k] = (const unsigned*)src[k];
    as.n[k] = (int)n[k];
    if (kind[k] == EVF_ACT_WORDS) as.words |= 1u << k;
    n_max = n[k] > n_max ? n[k] : n_max;
  }
  const int parts = evf_activity_parts(n_max);
  hipLaunchKernelGGL(k_activity_at, dim3(parts, nsrc, B), dim3(ACT_THREADS), 0, EVF_STREAM(stream), as, (const long long*)row,
                     (long long)row_mul, (long long)row_add, (long long)nrows, (unsigned*)log);
  return evf_status();
}

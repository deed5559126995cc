// Result log of a replayed evaluation step (evaluate.ResidentEvalStep): a captured graph cannot hand its metric values to the
// host without a read per step, so it appends them to a preallocated device log instead, at the row the host named in the
// step's job table.
//
//   evf_store_segments_at  log[row[0] * row_floats + offset[k] + i] = src[k][i], up to 32 segments in one launch.
//
// A plain streaming copy: a row is K * (B + 1) + P floats (a few dozen), every segment one to B of them.
#include "evf_common.h"

// --------------------------------------------------------------------------
// evf_store_segments_at
// --------------------------------------------------------------------------
// Block y = segment, a grid-stride loop of dword loads and stores over it (the destinations are only 4-byte aligned: the row
// pitch and the offsets are arbitrary).  The row word is read once per block; a row outside 0 .. nrows - 1 returns before any
// store.  offset[k] + n[k] <= row_floats is checked on the host, so an accepted row never writes outside the log.
#define STORE_THREADS 256
#define STORE_MAX_BLOCKS 64  // per segment
struct StoreSegs {
  const float* src[32];
  int offset[32];
  int n[32];
};
__global__ void __launch_bounds__(STORE_THREADS) k_store_segments_at(const long long* __restrict__ row, long long nrows,
                                                                      float* __restrict__ log, long long row_floats, StoreSegs sg) {
  __shared__ long long r;
  if (threadIdx.x == 0) r = row[0];  // one load per block
  __syncthreads();
  if (r < 0 || r >= nrows) return;
  const int k = blockIdx.y;
  const float* s = sg.src[k];
  float* d = log + r * row_floats + sg.offset[k];
  const int n = sg.n[k];
  for (int i = blockIdx.x * STORE_THREADS + threadIdx.x; i < n; i += gridDim.x * STORE_THREADS) d[i] = s[i];
}

extern "C" int evf_store_segments_at(const int64_t* row, int64_t nrows, float* log, int64_t row_floats, const void* const* src,
                                     const int* offset, const int* n, int nseg, void* stream) {
  if (!row || !log || !src || !offset || !n || nseg < 1 || nseg > 32) return EVF_EINVAL;
  StoreSegs sg;
  int most = 0;
  for (int k = 0; k < 32; ++k) {
    sg.src[k] = nullptr;
    sg.offset[k] = 0;
    sg.n[k] = 0;
    if (k >= nseg) continue;
    if (!src[k] || ((uintptr_t)src[k] & 3u) || n[k] < 0 || offset[k] < 0 || (int64_t)offset[k] + (int64_t)n[k] > row_floats)
      return EVF_EINVAL;
    sg.src[k] = (const float*)src[k];
    sg.offset[k] = offset[k];
    sg.n[k] = n[k];
    if (n[k] > most) most = n[k];
  }
  int blocks = evf_cdiv(most, STORE_THREADS);
  blocks = blocks < 1 ? 1 : (blocks > STORE_MAX_BLOCKS ? STORE_MAX_BLOCKS : blocks);
  hipLaunchKernelGGL(k_store_segments_at, dim3(blocks, nseg), dim3(STORE_THREADS), 0, EVF_STREAM(stream),
                     (const long long*)row, (long long)nrows, log, (long long)row_floats, sg);
  return evf_status();
}

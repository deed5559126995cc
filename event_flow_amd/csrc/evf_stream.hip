// Streaming inference (stream.py): events that arrive in pushes live in a device RING of R slots per column -- the arena's
// layout, xs, ys uint16, ts float64, ps uint8 -- that is appended to while windows are cut out of it.
//
//   evf_ring_append  one staged chunk of n events (one contiguous buffer ts | xs | ys | ps) scattered to slots (head + i) mod R.
//   evf_ring_cut     evf_seq_cut on the ring: job j takes the stream's events first[j] .. first[j] + N - 1 (absolute indices) from
//                    slots index mod R, as the same 16-byte rows (evf_seq_row_ring, evf_seq_row.h).
//
// Both are plain streaming kernels of a few tens of KB a call (a window of 20000 events is 260 KB of columns in, 320 KB of rows
// out): plain vector loads and stores, no atomics, no LDS.  Head, first and appended are words in DEVICE memory, read by the
// kernels, so both launches can sit in a captured graph.
#include "evf_seq_row.h"

// --------------------------------------------------------------------------
// evf_ring_append
// --------------------------------------------------------------------------
// Thread i copies event i of the chunk.  The chunk's columns start at byte 0 (ts), 8 n (xs), 10 n (ys), 12 n (ps) of a buffer that is
// 8-byte aligned, so every column is naturally aligned.  n <= R (the host's guard): no slot is written twice by one launch.  A
// negative head word is the kernel's own guard: nothing is written.
__global__ void k_ring_append(const unsigned char* __restrict__ chunk, int n, const long long* __restrict__ head,
                              uint16_t* __restrict__ xs, uint16_t* __restrict__ ys, double* __restrict__ ts,
                              uint8_t* __restrict__ ps, long R) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long hd = (long)*head;
  if (hd < 0) return;
  long at = hd % R + i;
  if (at >= R) at -= R;
  const double* cts = (const double*)chunk;
  const uint16_t* cxs = (const uint16_t*)(chunk + 8l * n);
  const uint16_t* cys = (const uint16_t*)(chunk + 10l * n);
  const uint8_t* cps = chunk + 12l * n;
  ts[at] = cts[i];
  xs[at] = cxs[i];
  ys[at] = cys[i];
  ps[at] = cps[i];
}

extern "C" int evf_ring_append(const void* chunk, int n, const int64_t* head, uint16_t* xs, uint16_t* ys, double* ts, uint8_t* ps,
                               int64_t R, void* stream) {
  if (!chunk || !head || !xs || !ys || !ts || !ps || n < 0 || R < 1 || (int64_t)n > R || ((uintptr_t)chunk & 7u) ||
      ((uintptr_t)head & 7u) || ((uintptr_t)ts & 7u) || ((uintptr_t)xs & 1u) || ((uintptr_t)ys & 1u))
    return EVF_EINVAL;
  if (n == 0) return EVF_OK;
  hipLaunchKernelGGL(k_ring_append, dim3(evf_cdiv(n, 256)), dim3(256), 0, EVF_STREAM(stream), (const unsigned char*)chunk, n,
                     (const long long*)head, xs, ys, ts, ps, (long)R);
  return evf_status();
}

// --------------------------------------------------------------------------
// evf_ring_cut
// --------------------------------------------------------------------------
// Job j = b * P + p reads the stream's events first[j] .. first[j] + N - 1.  The ring holds events [appended - R, appended): a job
// whose range is not inside it -- partly overwritten, partly unwritten, or N > R -- writes padding rows (p = 0) and dt = 0, like
// k_seq_cut for a range outside the arena (the table comes from the host; this is the kernel's own guard).
__global__ void k_ring_cut(const uint16_t* __restrict__ xs, const uint16_t* __restrict__ ys, const double* __restrict__ ts,
                           const uint8_t* __restrict__ ps, long R, const long long* __restrict__ first,
                           const long long* __restrict__ appended, const int* __restrict__ flags, int B, int P, int N, int H, int W,
                           float4* __restrict__ ev, double* __restrict__ dt_input) {
  const int j = blockIdx.y;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const long f = (long)first[j], a = (long)*appended;
  const int b = j / P, p = j - b * P;
  const bool live = (long)N <= R && f >= 0 && a >= 0 && f >= a - R && f <= a - N;
  evf_seq_row_ring(xs, ys, ts, ps, live, live ? f % R : 0, R, N, n, flags + j, H, W, ev + (long)j * N + n, dt_input + (long)p * B + b);
}

extern "C" int evf_ring_cut(const uint16_t* xs, const uint16_t* ys, const double* ts, const uint8_t* ps, int64_t R,
                            const int64_t* first, const int64_t* appended, const int* flags, int B, int P, int N, int H, int W,
                            float* ev, double* dt_input, void* stream) {
  if (!xs || !ys || !ts || !ps || !first || !appended || !flags || !ev || !dt_input || R < 1 || B <= 0 || P <= 0 || N <= 0 || H <= 0 ||
      W <= 0 || (long)B * P > 65535 || ((uintptr_t)first & 7u) || ((uintptr_t)appended & 7u) || ((uintptr_t)ev & 15u))
    return EVF_EINVAL;
  hipLaunchKernelGGL(k_ring_cut, dim3(evf_cdiv(N, 256), B * P), dim3(256), 0, EVF_STREAM(stream), xs, ys, ts, ps, (long)R,
                     (const long long*)first, (const long long*)appended, flags, B, P, N, H, W, (float4*)ev, dt_input);
  return evf_status();
}

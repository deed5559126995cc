// Streaming inference (stream.py): events that arrive in pushes live in a device RING of R slots per column -- the arena's
// layout, xs, ys uint16, ts float64, ps uint8 -- that is appended to while windows are cut out of it.
//
//   evf_ring_append  one staged chunk of n events (one contiguous buffer ts | xs | ys | ps) scattered to slots (head + i) mod R.
//   evf_ring_cut     evf_seq_cut on the ring: job j takes the stream's events first[j] .. first[j] + N - 1 (absolute indices) from
//                    slots index mod R, as the same 16-byte rows (evf_seq_row_ring, evf_seq_row.h).
//   evf_rings_append      evf_ring_append for the B rings of a rig (rig_stream.py) in ONE launch: the columns are [B][R], one staged
//                         buffer holds B head words, B + 1 offsets and the chunk of all cameras in camera order.
//   evf_rings_cut_ragged  evf_seq_cut_ragged on the B rings: job b takes count[b] events of ring b from stream index first[b] on.
//
// All are plain streaming kernels of a few tens of KB a call (a window of 20000 events is 260 KB of columns in, 320 KB of rows
// out): plain vector loads and stores, no atomics, no LDS.  Head, offsets, first, appended and count are words in DEVICE memory,
// read by the kernels, so every launch can sit in a captured graph.
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

// --------------------------------------------------------------------------
// evf_rings_append
// --------------------------------------------------------------------------
#define RIGS_MAX 16  // cameras of a rig: the offset walk of a thread is at most RIGS_MAX + 1 words

// The staged buffer: head int64 [B] | off int64 [B + 1] | the chunk ts | xs | ys | ps of n = off[B] events, camera b's at
// [off[b], off[b + 1]).  Thread i walks the offsets (the same B + 1 words for every thread: they stay in the cache), finds its camera
// and writes slot (head[b] + i - off[b]) mod R of ring b.  The kernel's own guards: a table that does not ascend from 0 to n, or
// gives a camera more than R events, writes nothing at all (every thread sees the same table); a negative head word writes nothing
// for that camera.  i - off[b] < R: no slot is written twice by one launch, and b < B, slot < R: nothing leaves the columns.
__global__ void k_rings_append(const long long* __restrict__ head, const long long* __restrict__ off,
                               const unsigned char* __restrict__ chunk, int B, int n, uint16_t* __restrict__ xs,
                               uint16_t* __restrict__ ys, double* __restrict__ ts, uint8_t* __restrict__ ps, long R) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool ok = off[0] == 0 && off[B] == (long long)n;
  int cam = 0;
  for (int b = 0; b < B; ++b) {
    const long long lo = off[b], hi = off[b + 1];
    ok = ok && lo <= hi && hi - lo <= (long long)R;
    if ((long long)i >= lo) cam = b;  // (ascending: the last camera whose range starts at or before i; empty ones end at lo)
  }
  if (!ok) return;
  // (with an ascending table off[cam] <= i, and i < off[cam + 1]: a later camera would have started at or before i otherwise)
  const long long hd = head[cam];
  if (hd < 0) return;
  long at = (long)(hd % R) + (long)((long long)i - off[cam]);
  if (at >= R) at -= R;
  at += (long)cam * R;
  const double* cts = (const double*)chunk;
  const uint16_t* cxs = (const uint16_t*)(chunk + 8l * n);
  const uint16_t* cys = (const uint16_t*)(chunk + 10l * n);
  const uint8_t* cps = chunk + 12l * n;
  ts[at] = cts[i];
  xs[at] = cxs[i];
  ys[at] = cys[i];
  ps[at] = cps[i];
}

extern "C" int evf_rings_append(const void* staged, int B, int n, int most, uint16_t* xs, uint16_t* ys, double* ts, uint8_t* ps,
                                int64_t R, void* stream) {
  if (!staged || !xs || !ys || !ts || !ps || B < 1 || B > RIGS_MAX || n < 0 || most < 0 || most > n || R < 1 || (int64_t)most > R ||
      (int64_t)n > (int64_t)B * most || ((uintptr_t)staged & 7u) || ((uintptr_t)ts & 7u) || ((uintptr_t)xs & 1u) ||
      ((uintptr_t)ys & 1u))
    return EVF_EINVAL;
  if (n == 0) return EVF_OK;
  const long long* head = (const long long*)staged;
  hipLaunchKernelGGL(k_rings_append, dim3(evf_cdiv(n, 256)), dim3(256), 0, EVF_STREAM(stream), head, head + B,
                     (const unsigned char*)(head + 2 * B + 1), B, n, xs, ys, ts, ps, (long)R);
  return evf_status();
}

// --------------------------------------------------------------------------
// evf_rings_cut_ragged
// --------------------------------------------------------------------------
// Job b reads the events first[b] .. first[b] + count[b] - 1 of camera b's stream from ring b (columns + b R) into rows 0 ..
// count[b] - 1 of its Npad rows; the rows behind are zero.  Ring b holds its camera's events [appended[b] - R, appended[b]): a job
// with no events, more than Npad or R of them, or a range that is not inside the ring is all padding with dt = 0, like
// k_seq_cut_ragged for a range outside the arena, and reads nothing.
__global__ void k_rings_cut_ragged(const uint16_t* __restrict__ xs, const uint16_t* __restrict__ ys, const double* __restrict__ ts,
                                   const uint8_t* __restrict__ ps, long R, const long long* __restrict__ first,
                                   const long long* __restrict__ appended, const int* __restrict__ count,
                                   const int* __restrict__ flags, int Npad, int H, int W, float4* __restrict__ ev,
                                   double* __restrict__ dt_input) {
  const int b = blockIdx.y;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= Npad) return;
  const long f = (long)first[b], a = (long)appended[b], c = (long)count[b];
  const bool ok = c > 0 && c <= (long)Npad && c <= R && f >= 0 && a >= 0 && f >= a - R && f <= a - c;
  const long at = (long)b * R;
  // (n == 0 < c in a valid job with events: only an empty or refused job writes dt = 0)
  evf_seq_row_ring(xs + at, ys + at, ts + at, ps + at, ok && n < c, ok ? f % R : 0, R, c, n, flags + b, H, W, ev + (long)b * Npad + n,
                   dt_input + b);
}

extern "C" int evf_rings_cut_ragged(const uint16_t* xs, const uint16_t* ys, const double* ts, const uint8_t* ps, int64_t R,
                                    const int64_t* first, const int64_t* appended, const int* count, const int* flags, int B,
                                    int Npad, int H, int W, float* ev, double* dt_input, void* stream) {
  if (!xs || !ys || !ts || !ps || !first || !appended || !count || !flags || !ev || !dt_input || R < 1 || B < 1 || B > RIGS_MAX ||
      Npad <= 0 || H <= 0 || W <= 0 || ((uintptr_t)first & 7u) || ((uintptr_t)appended & 7u) || ((uintptr_t)count & 3u) ||
      ((uintptr_t)flags & 3u) || ((uintptr_t)ts & 7u) || ((uintptr_t)xs & 1u) || ((uintptr_t)ys & 1u) || ((uintptr_t)ev & 15u) ||
      ((uintptr_t)dt_input & 7u))
    return EVF_EINVAL;
  hipLaunchKernelGGL(k_rings_cut_ragged, dim3(evf_cdiv(Npad, 256), B), dim3(256), 0, EVF_STREAM(stream), xs, ys, ts, ps, (long)R,
                     (const long long*)first, (const long long*)appended, count, flags, Npad, H, W, (float4*)ev, dt_input);
  return evf_status();
}

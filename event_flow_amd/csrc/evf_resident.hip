// Device-resident event sequences (dataloader/resident.py): the loader's host work of dataloader/h5.py:240-311 and
// dataloader/base.py:60-116 as two kernels.
//
//   evf_seq_cut     input windows cut out of the sequence columns that were uploaded once, formatted and flipped like
//                   event_formatting / augment_events, one 16-byte row (t, y, x, p) per event.
//   evf_hot_pixels  create_hot_mask + get_hot_event_mask: the persistent per-slot statistics and the mask of every pass.
//   evf_zero_segments_if  the recurrent state's reset as a node of a replayed step: zero-fill under a device flag.
//
// All are plain streaming kernels: a c3 window is 80 jobs x 1000 events (1 MB of rows) and 80 masks of 128 x 128 pixels.
// The row of an event is evf_seq_row (evf_seq_row.h), shared with evf_seq_cut_ragged.
#include "evf_seq_row.h"

// --------------------------------------------------------------------------
// evf_seq_cut
// --------------------------------------------------------------------------
// Job j = b * P + p reads events first[j] .. first[j] + N - 1 of the arena.  A job whose range leaves the arena writes padding
// rows (p = 0) and dt = 0 instead of reading out of bounds (the table comes from the host; this is the kernel's own guard).
__global__ void k_seq_cut(const uint16_t* __restrict__ xs, const uint16_t* __restrict__ ys, const double* __restrict__ ts,
                          const uint8_t* __restrict__ ps, long total, const long long* __restrict__ first,
                          const int* __restrict__ flags, int B, int P, int N, int H, int W, float4* __restrict__ ev,
                          double* __restrict__ dt_input) {
  const int j = blockIdx.y;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const long f = (long)first[j];
  const int b = j / P, p = j - b * P;
  evf_seq_row(xs, ys, ts, ps, f >= 0 && f <= total - N, f, N, n, flags + j, H, W, ev + (long)j * N + n, dt_input + (long)p * B + b);
}

extern "C" int evf_seq_cut(const uint16_t* xs, const uint16_t* ys, const double* ts, const uint8_t* ps, int64_t total,
                           const int64_t* first, const int* flags, int B, int P, int N, int H, int W, float* ev,
                           double* dt_input, void* stream) {
  if (!xs || !ys || !ts || !ps || !first || !flags || !ev || !dt_input || total < 0 || B <= 0 || P <= 0 || N <= 0 || H <= 0 ||
      W <= 0 || (long)B * P > 65535)
    return EVF_EINVAL;
  hipLaunchKernelGGL(k_seq_cut, dim3(evf_cdiv(N, 256), B * P), dim3(256), 0, EVF_STREAM(stream), xs, ys, ts, ps, (long)total,
                     (const long long*)first, flags, B, P, N, H, W, (float4*)ev, dt_input);
  return evf_status();
}

// --------------------------------------------------------------------------
// evf_hot_pixels
// --------------------------------------------------------------------------
#define HOT_THREADS 1024

// block-wide integer sum, the result in every thread (smem: >= 16 ints)
__device__ __forceinline__ int hot_block_sum(int v, int* smem) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) smem[wid] = v;
  __syncthreads();
  int r = 0;
  for (int w = 0; w < HOT_THREADS / 64; ++w) r += smem[w];
  __syncthreads();
  return r;
}

// Order key of a pixel for the selection: the bits of its rate when the rate exceeds max_rate, else 0.  Rates are
// non-negative floats, whose bit patterns order like their values; max_rate >= 0, so a selected pixel has a key > 0.
__device__ __forceinline__ uint32_t hot_key(int count, float fidx, float max_rate) {
  const float rate = (float)count / fidx;  // base.py:114: float32 tensor / int
  return rate > max_rate ? __float_as_uint(rate) : 0u;
}

// One block per slot walks the slot's P passes in order.  events [B][HW] int32 and obvs [B] are the persistent statistics
// (hot_events / hot_idx of base.py:34-39).  Masks: mask_bp [B][P][HW] and / or mask_pb [P][B][HW], 1 = keep.
__global__ void __launch_bounds__(HOT_THREADS)
k_hot_pixels(const float4* __restrict__ ev, const int* __restrict__ reset, int* __restrict__ events, int* __restrict__ obvs,
             float* __restrict__ mask_bp, float* __restrict__ mask_pb, int B, int P, int N, int H, int W, int max_px,
             int min_obvs, float max_rate) {
  extern __shared__ uint32_t lds[];
  const int HW = H * W, words = (HW + 31) / 32;
  uint32_t* bitmap = lds;               // [words]
  int* red = (int*)(lds + words);       // [16]
  int* scan = red + 16;                 // [HOT_THREADS]
  const int b = blockIdx.x, tid = threadIdx.x;
  int* cnt = events + (long)b * HW;
  int idx = obvs[b];
  for (int p = 0; p < P; ++p) {
    const bool rst = reset[b * P + p] != 0;
    if (rst) idx = 0;
    for (int w = tid; w < words; w += HOT_THREADS) bitmap[w] = 0u;
    __syncthreads();
    // pixels that received an event (base.py:108-111), coordinates truncated like .astype(int64)
    const float4* e = ev + ((long)b * P + p) * N;
    for (int n = tid; n < N; n += HOT_THREADS) {
      const float4 r = e[n];
      if (r.w == 0.f) continue;
      const long x = (long)r.z, y = (long)r.y;
      if (x < 0 || x >= W || y < 0 || y >= H) continue;
      const int q = (int)(y * W + x);
      atomicOr(&bitmap[q >> 5], 1u << (q & 31));
    }
    __syncthreads();
    idx += 1;
    const float fidx = (float)idx;
    const bool filter = idx > min_obvs && max_px > 0;
    // statistics (pixel q belongs to thread q % HOT_THREADS in every sweep of this kind) + number of pixels over the rate
    int over = 0;
    for (int q = tid; q < HW; q += HOT_THREADS) {
      const int c = (rst ? 0 : cnt[q]) + (int)((bitmap[q >> 5] >> (q & 31)) & 1u);
      cnt[q] = c;
      if (filter && hot_key(c, fidx, max_rate)) ++over;
    }
    over = hot_block_sum(over, red);  // (its barriers also end this pass's reads of the bitmap)
    float* m0 = mask_bp ? mask_bp + ((long)b * P + p) * HW : nullptr;
    float* m1 = mask_pb ? mask_pb + ((long)p * B + b) * HW : nullptr;
    if (!filter || over <= max_px) {  // all of them (or none): no order needed
      for (int q = tid; q < HW; q += HOT_THREADS) {
        const float m = (filter && hot_key(cnt[q], fidx, max_rate)) ? 0.f : 1.f;
        if (m0) m0[q] = m;
        if (m1) m1[q] = m;
      }
      continue;
    }
    // More candidates than max_px: torch.argmax takes the highest rate, the lowest flat index among equals, max_px times
    // (encodings.py:204-210).  K = the max_px-th largest key, by bisection on the key's bits: the largest K with
    // #(key >= K) >= max_px.
    uint32_t K = 0u;
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t trial = K | (1u << bit);
      int c = 0;
      for (int q = tid; q < HW; q += HOT_THREADS) c += hot_key(cnt[q], fidx, max_rate) >= trial ? 1 : 0;
      if (hot_block_sum(c, red) >= max_px) K = trial;
    }
    // every key > K is taken; of the keys == K the first `take` in index order.  Threads own contiguous chunks of pixels here
    // (the counts were written under the other mapping: the barriers of hot_block_sum above order those stores).
    const int chunk = (HW + HOT_THREADS - 1) / HOT_THREADS;
    const int q0 = min(tid * chunk, HW), q1 = min(q0 + chunk, HW);
    int above = 0, ties = 0;
    for (int q = q0; q < q1; ++q) {
      const uint32_t k = hot_key(cnt[q], fidx, max_rate);
      above += k > K ? 1 : 0;
      ties += k == K ? 1 : 0;
    }
    const int take = max_px - hot_block_sum(above, red);
    scan[tid] = ties;
    __syncthreads();
    for (int o = 1; o < HOT_THREADS; o <<= 1) {  // inclusive scan over the threads
      const int v = tid >= o ? scan[tid - o] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    int rank = scan[tid] - ties;  // ties in the chunks before this one
    __syncthreads();
    for (int q = q0; q < q1; ++q) {
      const uint32_t k = hot_key(cnt[q], fidx, max_rate);
      bool hot = k > K;
      if (k == K) hot = rank++ < take;
      const float m = hot ? 0.f : 1.f;
      if (m0) m0[q] = m;
      if (m1) m1[q] = m;
    }
    __syncthreads();  // the next pass writes the counts under the strided mapping again
  }
  if (tid == 0) obvs[b] = idx;
}

extern "C" int evf_hot_pixels(const float* ev, const int* reset, int* events, int* obvs, float* mask_bp, float* mask_pb, int B,
                              int P, int N, int H, int W, int max_px, int min_obvs, float max_rate, void* stream) {
  if (!ev || !reset || !events || !obvs || (!mask_bp && !mask_pb) || B <= 0 || P <= 0 || N < 0 || H <= 0 || W <= 0 ||
      !(max_rate >= 0.f) || (long)H * W > (1L << 18))  // (the bitmap of 2^18 pixels is 32 KiB of LDS)
    return EVF_EINVAL;
  const size_t lds = sizeof(uint32_t) * (((size_t)H * W + 31) / 32 + 16 + HOT_THREADS);
  hipLaunchKernelGGL(k_hot_pixels, dim3(B), dim3(HOT_THREADS), lds, EVF_STREAM(stream), (const float4*)ev, reset, events, obvs,
                     mask_bp, mask_pb, B, P, N, H, W, max_px, min_obvs, max_rate);
  return evf_status();
}

// --------------------------------------------------------------------------
// evf_zero_segments_if
// --------------------------------------------------------------------------
// Up to 32 segments (4-byte aligned, a multiple of 4 bytes long) set to zero bytes when *flag != 0 (flag NULL: always); block y =
// segment, a grid-stride loop of 16-byte stores over the segment's 16-byte aligned middle, dword stores for the up to three words
// before and after it.  A block whose flag reads 0 returns before any store: the clear case is one empty launch.
#define ZERO_THREADS 256
#define ZERO_MAX_BLOCKS 512  // per segment: one sweep of the grid covers 2 MiB of it
struct ZeroSegs {
  uint32_t* dst[32];
  long long bytes[32];
};
__global__ void __launch_bounds__(ZERO_THREADS) k_zero_segments_if(const int* __restrict__ flag, ZeroSegs sg) {
  __shared__ int go;
  if (threadIdx.x == 0) go = flag ? *flag : 1;  // one load per block
  __syncthreads();
  if (go == 0) return;
  const int k = blockIdx.y;
  uint32_t* p = sg.dst[k];
  const long words = sg.bytes[k] >> 2;
  long head = (long)(((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u) >> 2);  // words in front of the first 16-byte boundary
  if (head > words) head = words;
  const long nvec = (words - head) >> 2;
  const long tail0 = head + 4 * nvec;  // first word behind the last whole vector
  uint4* v = (uint4*)(p + head);
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  for (long i = (long)blockIdx.x * ZERO_THREADS + threadIdx.x; i < nvec; i += (long)gridDim.x * ZERO_THREADS) v[i] = z;
  if (blockIdx.x == 0) {
    if ((long)threadIdx.x < head) p[threadIdx.x] = 0u;
    if (tail0 + (long)threadIdx.x < words) p[tail0 + threadIdx.x] = 0u;  // (at most three words)
  }
}

extern "C" int evf_zero_segments_if(const int* flag, void* const* dst, const int64_t* bytes, int nseg, void* stream) {
  if (!dst || !bytes || nseg < 1 || nseg > 32) return EVF_EINVAL;
  ZeroSegs sg;
  long long most = 0;
  for (int k = 0; k < 32; ++k) {
    sg.dst[k] = nullptr;
    sg.bytes[k] = 0;
    if (k >= nseg) continue;
    if (!dst[k] || ((uintptr_t)dst[k] & 3u) || bytes[k] < 0 || (bytes[k] & 3)) return EVF_EINVAL;
    sg.dst[k] = (uint32_t*)dst[k];
    sg.bytes[k] = (long long)bytes[k];
    if (sg.bytes[k] > most) most = sg.bytes[k];
  }
  int blocks = evf_cdiv((long)most, (long)ZERO_THREADS * 16);
  blocks = blocks < 1 ? 1 : (blocks > ZERO_MAX_BLOCKS ? ZERO_MAX_BLOCKS : blocks);
  hipLaunchKernelGGL(k_zero_segments_if, dim3(blocks, nseg), dim3(ZERO_THREADS), 0, EVF_STREAM(stream), flag, sg);
  return evf_status();
}

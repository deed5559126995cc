// Device-resident evaluation (dataloader/resident_eval.py): the input modes `time`, `frames`, `gtflow_dt1` and `gtflow_dt4` of
// dataloader/h5.py:136-311 on sequences that were uploaded once.
//
//   evf_ts_search        binary_search_array (dataloader/encodings.py) for a batch of timestamps: every window boundary of every
//                        file in ONE launch at upload time.
//   evf_seq_cut_ragged   evf_seq_cut with an event count per job: rows behind a job's count are padding (all zero).
//   evf_gather_flowmaps  augment_flowmap of resident ground-truth maps picked by index.
//   evf_gather_frames    augment_frames of two resident APS frames per slot.
//
// All are streaming kernels, one thread per query / event / 16 bytes of output.  The row of an event is evf_seq_row
// (evf_seq_row.h), shared with evf_seq_cut.
#include "evf_seq_row.h"

#define RE_THREADS 256

// --------------------------------------------------------------------------
// evf_ts_search
// --------------------------------------------------------------------------
// The bisection of binary_search_array step for step: mid = lo + (hi - lo) / 2, the first equal element met is the answer
// (with duplicates that is not the leftmost one), else the final lo.  A segment that leaves the column answers -1.
__global__ void __launch_bounds__(RE_THREADS)
k_ts_search(const double* __restrict__ ts, long total, const long long* __restrict__ seg_begin, const long long* __restrict__ seg_len,
            const double* __restrict__ query, long Q, long long* __restrict__ out) {
  const long q = (long)blockIdx.x * RE_THREADS + threadIdx.x;
  if (q >= Q) return;
  const long b = (long)seg_begin[q], n = (long)seg_len[q];
  if (b < 0 || n < 0 || b > total - n) {
    out[q] = -1;
    return;
  }
  const double x = query[q];
  const double* a = ts + b;
  long lo = 0, hi = n - 1;
  while (lo <= hi) {
    const long mid = lo + (hi - lo) / 2;
    const double v = a[mid];
    if (v == x) {
      lo = mid;
      break;
    }
    if (x < v)
      hi = mid - 1;
    else
      lo = mid + 1;
  }
  out[q] = lo;
}

extern "C" int evf_ts_search(const double* ts, int64_t total, const int64_t* seg_begin, const int64_t* seg_len, const double* query,
                             int64_t Q, int64_t* out, void* stream) {
  if (!ts || !seg_begin || !seg_len || !query || !out || total <= 0 || Q <= 0 || Q > (int64_t)RE_THREADS * 2147483647LL)
    return EVF_EINVAL;
  hipLaunchKernelGGL(k_ts_search, dim3(evf_cdiv((long)Q, RE_THREADS)), dim3(RE_THREADS), 0, EVF_STREAM(stream), ts, (long)total,
                     (const long long*)seg_begin, (const long long*)seg_len, query, (long)Q, (long long*)out);
  return evf_status();
}

// --------------------------------------------------------------------------
// evf_seq_cut_ragged
// --------------------------------------------------------------------------
// Job j reads events first[j] .. first[j] + count[j] - 1 of the arena into rows 0 .. count[j] - 1 of its Npad rows; the rows
// behind are zero.  A job with a negative first or count, a count above Npad or a range that leaves the arena is all padding
// with dt = 0: nothing is read out of bounds.
__global__ void __launch_bounds__(RE_THREADS)
k_seq_cut_ragged(const uint16_t* __restrict__ xs, const uint16_t* __restrict__ ys, const double* __restrict__ ts,
                 const uint8_t* __restrict__ ps, long total, const long long* __restrict__ first, const int* __restrict__ count,
                 const int* __restrict__ flags, int Npad, int H, int W, float4* __restrict__ ev, double* __restrict__ dt_input) {
  const int j = blockIdx.y;
  const int n = blockIdx.x * RE_THREADS + threadIdx.x;
  if (n >= Npad) return;
  const long f = (long)first[j];
  const long c = (long)count[j];
  const bool ok = c > 0 && c <= (long)Npad && f >= 0 && f <= total - c;
  // (n == 0 < c in a valid job with events: only an empty or refused job writes dt = 0)
  evf_seq_row(xs, ys, ts, ps, ok && n < c, f, c, n, flags + j, H, W, ev + (long)j * Npad + n, dt_input + j);
}

extern "C" int evf_seq_cut_ragged(const uint16_t* xs, const uint16_t* ys, const double* ts, const uint8_t* ps, int64_t total,
                                  const int64_t* first, const int* count, const int* flags, int J, int Npad, int H, int W, float* ev,
                                  double* dt_input, void* stream) {
  if (!xs || !ys || !ts || !ps || !first || !count || !flags || !ev || !dt_input || total <= 0 || J <= 0 || Npad <= 0 || H <= 0 ||
      W <= 0 || J > 65535)
    return EVF_EINVAL;
  hipLaunchKernelGGL(k_seq_cut_ragged, dim3(evf_cdiv(Npad, RE_THREADS), J), dim3(RE_THREADS), 0, EVF_STREAM(stream), xs, ys, ts, ps,
                     (long)total, (const long long*)first, count, flags, Npad, H, W, (float4*)ev, dt_input);
  return evf_status();
}

// --------------------------------------------------------------------------
// evf_gather_flowmaps / evf_gather_frames
// --------------------------------------------------------------------------
// One thread per VEC consecutive pixels of an output row; consecutive threads write consecutive addresses.  A reversed row
// reads the mirrored group and swaps its elements, so both directions move whole groups: VEC = 4 floats / 16 bytes when W
// is a multiple of it and the tensors are 16-byte aligned, else VEC = 1.  Flags: bit 0 reverses x, bit 1 reverses y.

template <int VEC>
__global__ void __launch_bounds__(RE_THREADS)
k_gather_flowmaps(const float* __restrict__ maps, int M, const int* __restrict__ idx, const int* __restrict__ flags, long groups,
                  int H, int W, float* __restrict__ out) {
  const long i = (long)blockIdx.x * RE_THREADS + threadIdx.x;
  if (i >= groups) return;
  const int Wg = W / VEC;
  const int xg = (int)(i % Wg);
  long r = i / Wg;
  const int y = (int)(r % H);
  r /= H;
  const int c = (int)(r & 1);
  const int b = (int)(r >> 1);
  const int m = idx[b], fl = flags[b];
  const int x0 = xg * VEC;
  const int sx = (fl & 1) ? W - VEC - x0 : x0;
  const int sy = (fl & 2) ? H - 1 - y : y;
  const bool neg = c == 0 ? (fl & 1) != 0 : (fl & 2) != 0;  // a flipped axis negates its own flow component
  const bool in = m >= 0 && m < M;
  const long src = in ? (((long)m * 2 + c) * H + sy) * W + sx : 0;
  const long dst = (((long)b * 2 + c) * H + y) * W + x0;
  if constexpr (VEC == 4) {
    float4 v = in ? *(const float4*)(maps + src) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (fl & 1) v = make_float4(v.w, v.z, v.y, v.x);
    if (neg) v = make_float4(-v.x, -v.y, -v.z, -v.w);
    *(float4*)(out + dst) = v;
  } else {
    const float v = in ? maps[src] : 0.f;
    out[dst] = neg ? -v : v;
  }
}

extern "C" int evf_gather_flowmaps(const float* maps, int M, const int* idx, const int* flags, int B, int H, int W, float* out,
                                   void* stream) {
  if (!maps || !idx || !flags || !out || M <= 0 || B <= 0 || H <= 0 || W <= 0) return EVF_EINVAL;
  const bool vec = (W % 4) == 0 && (((uintptr_t)maps | (uintptr_t)out) & 15u) == 0;
  const long rows = (long)B * 2 * H, per_row = vec ? W / 4 : W;
  if (rows > (long)RE_THREADS * 2147483647L / per_row) return EVF_EINVAL;  // (more blocks than a grid holds)
  const long groups = rows * per_row;
  const dim3 grid(evf_cdiv(groups, RE_THREADS));
  if (vec)
    hipLaunchKernelGGL(k_gather_flowmaps<4>, grid, dim3(RE_THREADS), 0, EVF_STREAM(stream), maps, M, idx, flags, groups, H, W, out);
  else
    hipLaunchKernelGGL(k_gather_flowmaps<1>, grid, dim3(RE_THREADS), 0, EVF_STREAM(stream), maps, M, idx, flags, groups, H, W, out);
  return evf_status();
}

// the four bytes of a word in reverse order
__device__ __forceinline__ uint32_t re_swap_bytes(uint32_t w) { return __builtin_bswap32(w); }

template <int VEC>
__global__ void __launch_bounds__(RE_THREADS)
k_gather_frames(const uint8_t* __restrict__ frames, int M, const int* __restrict__ curr, const int* __restrict__ next,
                const int* __restrict__ flags, long groups, int H, int W, uint8_t* __restrict__ out) {
  const long i = (long)blockIdx.x * RE_THREADS + threadIdx.x;
  if (i >= groups) return;
  const int Wg = W / VEC;
  const int xg = (int)(i % Wg);
  long r = i / Wg;
  const int y = (int)(r % H);
  r /= H;
  const int c = (int)(r & 1);
  const int b = (int)(r >> 1);
  const int m = c == 0 ? curr[b] : next[b], fl = flags[b];
  const int x0 = xg * VEC;
  const int sx = (fl & 1) ? W - VEC - x0 : x0;
  const int sy = (fl & 2) ? H - 1 - y : y;
  const bool in = m >= 0 && m < M;
  const long src = in ? ((long)m * H + sy) * W + sx : 0;
  const long dst = (((long)b * 2 + c) * H + y) * W + x0;
  if constexpr (VEC == 16) {
    uint4 v = in ? *(const uint4*)(frames + src) : make_uint4(0u, 0u, 0u, 0u);
    if (fl & 1) v = make_uint4(re_swap_bytes(v.w), re_swap_bytes(v.z), re_swap_bytes(v.y), re_swap_bytes(v.x));
    *(uint4*)(out + dst) = v;
  } else {
    out[dst] = in ? frames[src] : (uint8_t)0;
  }
}

extern "C" int evf_gather_frames(const uint8_t* frames, int M, const int* curr, const int* next, const int* flags, int B, int H,
                                 int W, uint8_t* out, void* stream) {
  if (!frames || !curr || !next || !flags || !out || M <= 0 || B <= 0 || H <= 0 || W <= 0) return EVF_EINVAL;
  const bool vec = (W % 16) == 0 && (((uintptr_t)frames | (uintptr_t)out) & 15u) == 0;
  const long rows = (long)B * 2 * H, per_row = vec ? W / 16 : W;
  if (rows > (long)RE_THREADS * 2147483647L / per_row) return EVF_EINVAL;  // (more blocks than a grid holds)
  const long groups = rows * per_row;
  const dim3 grid(evf_cdiv(groups, RE_THREADS));
  if (vec)
    hipLaunchKernelGGL(k_gather_frames<16>, grid, dim3(RE_THREADS), 0, EVF_STREAM(stream), frames, M, curr, next, flags, groups, H, W,
                       out);
  else
    hipLaunchKernelGGL(k_gather_frames<1>, grid, dim3(RE_THREADS), 0, EVF_STREAM(stream), frames, M, curr, next, flags, groups, H, W,
                       out);
  return evf_status();
}

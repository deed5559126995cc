// Training log of a (replayed) optimizer step (monitor.TrainMonitor): what the reference's vis.store_grads records per step --
// mean, min and max of |grad| per weight tensor after clipping -- and the spike rate of every layer of the fused FireNets, appended
// to a preallocated device log at the row the host named in the step's job table (the device-log conventions, evf_log.h).
//
//   evf_grad_stats_partial   BEFORE the optimizer step (which clears the gradient): per segment and chunk of GS_CHUNK elements
//                            (float64 sum |g|, min |g|, max |g|, NaN seen) -> ws[segment][chunk].
//   evf_grad_stats_store     AFTER the optimizer step: the chunks of a segment added in chunk order, scaled by the clip coefficient
//                            the step applied (from the squared norm it left in norm_ws[0]) ->
//                            log[row][offset ..] = [loss, norm, coef, (mean, min, max) per segment].
//   evf_spike_count          set bits of up to 32 int32 word tensors -> SC_PARTS integer partials per source in ws[slot0 + k].
//   evf_spike_rates_store    per layer the partials of its slots added in slot order (int64) -> log[row][offset + layer] = rate.
//
// Plain launches on one stream, no atomics, no ticket: every addition's order is fixed by the geometry, so two calls give the same
// bits; nothing is allocated or copied, so the calls can be captured.  A row word outside 0 .. nrows - 1 leaves the log untouched.
#include "evf_log.h"

#define GS_THREADS 256
#define GS_CHUNK 4096  // elements per block: 16 per thread
#define GS_WORDS 5     // a chunk's partials: the float64 sum as two words, min, max, NaN flag
#define GS_TILE 256    // chunks the store kernel stages per round

#define SC_THREADS 256
#define SC_PARTS 32  // blocks (and partials) per source
#define SC_MAX_SLOTS 256

// --------------------------------------------------------------------------
// evf_grad_stats_partial
// --------------------------------------------------------------------------
struct GsAcc {
  double s;
  float lo, hi, nan;
};
__device__ __forceinline__ void gs_take(float x, GsAcc& a) {
  const float m = fabsf(x);
  a.nan += (x != x) ? 1.f : 0.f;  // (fminf / fmaxf drop a NaN: it is flagged here and poisons the segment in the store kernel)
  a.s += (double)m;
  a.lo = fminf(a.lo, m);
  a.hi = fmaxf(a.hi, m);
}

// Block (c, k): elements [c * GS_CHUNK, min((c + 1) * GS_CHUNK, n_k)) of segment k.  The segment starts anywhere: evf_walk16.
// A block past its segment's end leaves at once (its ws entry is never read).  Every other block writes its entry: ws needs no
// clearing.
__global__ void __launch_bounds__(GS_THREADS) k_grad_stats_partial(const float* __restrict__ grad, const long long* __restrict__ seg_off,
                                                                   const long long* __restrict__ seg_n, long long max_n,
                                                                   float* __restrict__ ws) {
  __shared__ float red[16];
  __shared__ double dred[4];
  __shared__ float lred[4], hred[4];
  const int k = blockIdx.y;
  long long n = seg_n[k];
  n = n < 0 ? 0 : (n > max_n ? max_n : n);  // (the grid and ws are sized from max_n)
  const long long a = (long long)blockIdx.x * GS_CHUNK;
  if (a >= n) return;
  const long long b = a + GS_CHUNK < n ? a + GS_CHUNK : n;
  const float* g = grad + seg_off[k] + a;
  GsAcc acc = {0.0, INFINITY, 0.f, 0.f};
  evf_walk16(g, (int)(b - a), (int)threadIdx.x, GS_THREADS, true, [&](float x) { gs_take(x, acc); });
  // wave butterflies, then the four waves in index order
  const double ws_ = evf_wave_sum(acc.s);
  const float wlo = evf_wave_min(acc.lo), whi = evf_wave_max(acc.hi);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) dred[wid] = ws_, lred[wid] = wlo, hred[wid] = whi;
  const float nans = evf_block_sum(acc.nan, red);  // (its barriers publish dred / lred / hred as well)
  if (threadIdx.x != 0) return;
  const double S = ((dred[0] + dred[1]) + dred[2]) + dred[3];
  const float lo = fminf(fminf(lred[0], lred[1]), fminf(lred[2], lred[3]));
  const float hi = fmaxf(fmaxf(hred[0], hred[1]), fmaxf(hred[2], hred[3]));
  float* w = ws + ((long long)k * gridDim.x + blockIdx.x) * GS_WORDS;
  w[0] = __int_as_float(__double2loint(S));  // (ws is only 4-byte aligned: the double travels as two words)
  w[1] = __int_as_float(__double2hiint(S));
  w[2] = lo;
  w[3] = hi;
  w[4] = nans;
}

extern "C" int evf_grad_stats_chunk() { return GS_CHUNK; }

extern "C" int64_t evf_grad_stats_ws(int nseg, int64_t max_n) {
  if (nseg < 1 || max_n < 1 || max_n > (int64_t)65535 * GS_CHUNK || nseg > 65535) return EVF_EINVAL;
  return (int64_t)nseg * evf_cdiv(max_n, GS_CHUNK) * GS_WORDS;
}

extern "C" int evf_grad_stats_partial(const float* grad, const int64_t* seg_off, const int64_t* seg_n, int nseg, int64_t max_n,
                                      float* ws, int64_t ws_floats, void* stream) {
  if (!grad || !seg_off || !seg_n || !ws) return EVF_EINVAL;
  const int64_t need = evf_grad_stats_ws(nseg, max_n);
  if (need < 0 || ws_floats < need) return EVF_EINVAL;
  if (((uintptr_t)grad & 3u) || ((uintptr_t)ws & 3u) || ((uintptr_t)seg_off & 7u) || ((uintptr_t)seg_n & 7u)) return EVF_EINVAL;
  hipLaunchKernelGGL(k_grad_stats_partial, dim3(evf_cdiv(max_n, GS_CHUNK), nseg), dim3(GS_THREADS), 0, EVF_STREAM(stream), grad,
                     (const long long*)seg_off, (const long long*)seg_n, (long long)max_n, ws);
  return evf_status();
}

// --------------------------------------------------------------------------
// evf_grad_stats_store
// --------------------------------------------------------------------------
// Block k < nseg: segment k; block nseg: the row's head.  The chunks are staged GS_TILE at a time by the whole block and added by
// thread 0 in chunk order.  coef is k_clip_adam_fused's expression (evf_step_tail.hip) on the squared norm that step left behind,
// so the logged norm and coefficient are the applied ones bit for bit.
__global__ void __launch_bounds__(GS_TILE) k_grad_stats_store(const float* __restrict__ ws, const long long* __restrict__ seg_n,
                                                              int nseg, long long max_n, int chunks_ld,
                                                              const float* __restrict__ norm_ws, float max_norm,
                                                              const float* __restrict__ loss, const long long* __restrict__ row,
                                                              long long nrows, float* __restrict__ log, long long row_floats,
                                                              int offset) {
  __shared__ float st[GS_TILE][GS_WORDS];
  const long long r = evf_log_row(row, 1, 0, nrows);
  if (r < 0) return;
  const float total = norm_ws[0];
  float coef = 1.f;
  if (max_norm > 0.f) coef = fminf(1.f, max_norm / (sqrtf(total) + 1e-6f));
  float* d = log + r * row_floats + offset;
  const int k = blockIdx.x;
  if (k == nseg) {
    if (threadIdx.x == 0) {
      if (loss) d[0] = loss[0];
      d[1] = sqrtf(total);
      d[2] = coef;
    }
    return;
  }
  long long n = seg_n[k];
  n = n < 0 ? 0 : (n > max_n ? max_n : n);
  const int nchunks = (int)((n + GS_CHUNK - 1) / GS_CHUNK);
  const float* w = ws + (long long)k * chunks_ld * GS_WORDS;
  double S = 0.0;
  float lo = INFINITY, hi = 0.f, nans = 0.f;
  for (int c0 = 0; c0 < nchunks; c0 += GS_TILE) {
    const int c = c0 + threadIdx.x;
    if (c < nchunks)
#pragma unroll
      for (int j = 0; j < GS_WORDS; ++j) st[threadIdx.x][j] = w[(long long)c * GS_WORDS + j];
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = nchunks - c0 < GS_TILE ? nchunks - c0 : GS_TILE;
      for (int i = 0; i < m; ++i) {
        S += __hiloint2double(__float_as_int(st[i][1]), __float_as_int(st[i][0]));
        lo = fminf(lo, st[i][2]);
        hi = fmaxf(hi, st[i][3]);
        nans += st[i][4];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  float mean = (float)((double)coef * S / (double)n);
  float mn = lo * coef, mx = hi * coef;  // monotone under rounding: torch's (g * coef).abs().min() / .max()
  if (nans != 0.f) mean = mn = mx = __int_as_float(0x7fc00000);
  d[3 + 3 * k] = mean;
  d[4 + 3 * k] = mn;
  d[5 + 3 * k] = mx;
}

extern "C" int evf_grad_stats_store(const float* ws, int64_t ws_floats, const int64_t* seg_n, int nseg, int64_t max_n,
                                    const float* norm_ws, float max_norm, const float* loss, const int64_t* row, int64_t nrows,
                                    float* log, int64_t row_floats, int offset, void* stream) {
  if (!ws || !seg_n || !norm_ws) return EVF_EINVAL;  // (loss may be NULL: the field is left as it is)
  const int64_t need = evf_grad_stats_ws(nseg, max_n);
  if (need < 0 || ws_floats < need) return EVF_EINVAL;
  if (!evf_log_dest_ok(row, nrows, log, row_floats, offset, 3 + 3 * (int64_t)nseg)) return EVF_EINVAL;
  if (((uintptr_t)ws & 3u) || ((uintptr_t)norm_ws & 3u) || ((uintptr_t)loss & 3u) || ((uintptr_t)seg_n & 7u)) return EVF_EINVAL;
  hipLaunchKernelGGL(k_grad_stats_store, dim3(nseg + 1), dim3(GS_TILE), 0, EVF_STREAM(stream), ws, (const long long*)seg_n, nseg,
                     (long long)max_n, evf_cdiv(max_n, GS_CHUNK), norm_ws, max_norm, loss, (const long long*)row, (long long)nrows, log,
                     (long long)row_floats, offset);
  return evf_status();
}

// --------------------------------------------------------------------------
// evf_spike_count
// --------------------------------------------------------------------------
// Block (p, k): part p of source k, a grid-stride loop over the source's 16-byte groups (evf_walk16); block 0 of a source also
// takes the peel and the tail.  Every block stores its partial (0 when it had nothing): ws needs no clearing.  A partial is at most n_words * 32 / SC_PARTS + 7 * 32 < 2^32.
struct ScSrc {
  const unsigned* src[32];
};
__global__ void __launch_bounds__(SC_THREADS) k_spike_count(ScSrc sc, long long n_words, unsigned* __restrict__ ws, int slot0) {
  __shared__ unsigned red[SC_THREADS / 64];
  const int k = blockIdx.y;
  unsigned cnt = 0;
  evf_walk16(sc.src[k], n_words, (long long)blockIdx.x * SC_THREADS + threadIdx.x, (long long)SC_PARTS * SC_THREADS, blockIdx.x == 0,
             [&](unsigned w) { cnt += act_one<true>(w); });
  cnt = evf_block_count(cnt, red);
  if (threadIdx.x == 0) ws[(long long)(slot0 + k) * SC_PARTS + blockIdx.x] = cnt;
}

extern "C" int evf_spike_count_parts() { return SC_PARTS; }

extern "C" int evf_spike_count(const void* const* src, int nsrc, int64_t n_words, void* ws, int slot0, int ws_slots, void* stream) {
  if (!src || !ws || nsrc < 1 || nsrc > 32 || n_words < 1 || n_words > 2147483647LL) return EVF_EINVAL;
  if (slot0 < 0 || ws_slots < 1 || (int64_t)slot0 + nsrc > ws_slots || ((uintptr_t)ws & 3u)) return EVF_EINVAL;
  ScSrc sc;
  for (int k = 0; k < 32; ++k) {
    sc.src[k] = nullptr;
    if (k >= nsrc) continue;
    if (!src[k] || ((uintptr_t)src[k] & 3u)) return EVF_EINVAL;
    sc.src[k] = (const unsigned*)src[k];
  }
  hipLaunchKernelGGL(k_spike_count, dim3(SC_PARTS, nsrc), dim3(SC_THREADS), 0, EVF_STREAM(stream), sc, (long long)n_words, (unsigned*)ws,
                     slot0);
  return evf_status();
}

// --------------------------------------------------------------------------
// evf_spike_rates_store
// --------------------------------------------------------------------------
// One block, thread l = layer l: the partials of the layer's slots in slot order, parts in part order, as int64 -- an exact count --
// and rate = (float)((double)count / (double)total): one division and one rounding of exact operands.
struct ScLayers {
  unsigned char layer[SC_MAX_SLOTS];
};
__global__ void __launch_bounds__(SC_MAX_SLOTS) k_spike_rates_store(const unsigned* __restrict__ ws, ScLayers sl, int nslots, int nlayers,
                                                                    long long total, const long long* __restrict__ row,
                                                                    long long nrows, float* __restrict__ log, long long row_floats,
                                                                    int offset) {
  const long long r = evf_log_row(row, 1, 0, nrows);
  if (r < 0) return;
  const int l = threadIdx.x;
  if (l >= nlayers) return;
  long long cnt = 0;
  for (int s = 0; s < nslots; ++s) {
    if (sl.layer[s] != l) continue;
    for (int p = 0; p < SC_PARTS; ++p) cnt += (long long)ws[(long long)s * SC_PARTS + p];
  }
  log[r * row_floats + offset + l] = (float)((double)cnt / (double)total);
}

extern "C" int evf_spike_rates_store(const void* ws, int ws_slots, const int* slot_layer, int nslots, int nlayers,
                                     int64_t total_bits_per_layer, const int64_t* row, int64_t nrows, float* log, int64_t row_floats,
                                     int offset, void* stream) {
  if (!ws || !slot_layer || ((uintptr_t)ws & 3u)) return EVF_EINVAL;
  if (nslots < 1 || nslots > SC_MAX_SLOTS || nlayers < 1 || nlayers > SC_MAX_SLOTS || ws_slots < nslots) return EVF_EINVAL;
  if (total_bits_per_layer <= 0 || !evf_log_dest_ok(row, nrows, log, row_floats, offset, nlayers)) return EVF_EINVAL;
  ScLayers sl;
  for (int s = 0; s < SC_MAX_SLOTS; ++s) {
    sl.layer[s] = 0xff;
    if (s >= nslots) continue;
    if (slot_layer[s] < 0 || slot_layer[s] >= nlayers) return EVF_EINVAL;
    sl.layer[s] = (unsigned char)slot_layer[s];
  }
  hipLaunchKernelGGL(k_spike_rates_store, dim3(1), dim3(SC_MAX_SLOTS), 0, EVF_STREAM(stream), (const unsigned*)ws, sl, nslots, nlayers,
                     (long long)total_bits_per_layer, (const long long*)row, (long long)nrows, log, (long long)row_floats, offset);
  return evf_status();
}

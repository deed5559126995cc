// Result log of a replayed evaluation step (evaluate.ResidentEvalStep): a captured graph cannot hand its metric values to the
// host without a read per step, so it appends them to a preallocated device log instead, at the row the host named in the
// step's job table.
//
//   evf_store_segments_at  log[row[0] * row_floats + offset[k] + i] = src[k][i], up to 32 segments in one launch.
//   evf_aee_at             the AEE of one pass (evaluate.ResidentAEEStep) reduced and stored at log[row[0] * row_floats + offset ..].
//
// The first is a plain streaming copy: a row is K * (B + 1) + P floats (a few dozen), every segment one to B of them.
// The row word, the no-op outside 0 .. nrows - 1 and the host's destination guard are evf_log.h's.
#include "evf_log.h"

// --------------------------------------------------------------------------
// evf_store_segments_at
// --------------------------------------------------------------------------
// Block y = segment, a grid-stride loop of dword loads and stores over it (the destinations are only 4-byte aligned: the row
// pitch and the offsets are arbitrary).  A row outside 0 .. nrows - 1 returns before any store.  offset[k] + n[k] <= row_floats
// is checked on the host, so an accepted row never writes outside the log.
#define STORE_THREADS 256
#define STORE_MAX_BLOCKS 64  // per segment
struct StoreSegs {
  const float* src[32];
  int offset[32];
  int n[32];
};
__global__ void __launch_bounds__(STORE_THREADS) k_store_segments_at(const long long* __restrict__ row, long long nrows,
                                                                      float* __restrict__ log, long long row_floats, StoreSegs sg) {
  const long long r = evf_log_row(row, 1, 0, nrows);
  if (r < 0) return;
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

// --------------------------------------------------------------------------
// evf_aee_at
// --------------------------------------------------------------------------
// The AEE of ONE pass (loss/flow.py:594-628 on the pass' own flow, event mask and ground-truth map) written straight into a row
// of a device log, in two plain launches on one stream:
//
//   k_aee_stripes  grid (S, B): block (s, b) reduces pixels [s * AEE_STRIPE, min((s + 1) * AEE_STRIPE, HW)) of sample b to
//                  (sum err, n valid, n outliers) and stores the triple to ws[b][s] -- every triple is written, none is read.
//   k_aee_finish   one block: per sample the S partials added in stripe order, then one thread forms the per-sample values and
//                  the two batch means in sample order and stores the 2 (B + 1) floats of the row.
//
// No ticket, no atomics, no cooperative launch: the order of every addition is fixed by the geometry, so two calls give the same
// bits.  The per-pixel arithmetic is k_aee's (evf_events.hip), operation for operation; the ratio dt_gt / dt_input, which the
// eager path divides in torch (float32 tensors), is the same single IEEE division here, on the device values.
// A 256 x 256 sample is 32 stripes: 1.3 MB streamed by 32 blocks with 16-byte loads instead of by one with dword loads.
#define AEE_THREADS 256
#define AEE_STRIPE 2048  // pixels per block: a multiple of 4 * AEE_THREADS

__device__ __forceinline__ void aee_pixel(float f0, float f1, float gx, float gy, float m, float S, float r, float& se, float& nv,
                                          float& no) {
  const float fx = f0 * S * r, fy = f1 * S * r;  // loss/flow.py:597-598
  const bool valid = (m != 0.f) && !((gx == 0.f) && (gy == 0.f));  // :605-614
  const float err = valid ? sqrtf((fx - gx) * (fx - gx) + (fy - gy) * (fy - gy)) : 0.f;
  const float mag = valid ? sqrtf(fx * fx + fy * fy) : 0.f;
  se += err;
  nv += valid ? 1.f : 0.f;
  no += ((err > 3.0f) && (err > 0.05f * mag)) ? 1.f : 0.f;  // :625
}

template <bool VEC>
__global__ void __launch_bounds__(AEE_THREADS) k_aee_stripes(const float* __restrict__ flow, const float* __restrict__ gt,
                                                             const float* __restrict__ mask, const double* __restrict__ dt_gt,
                                                             const double* __restrict__ dt_input, int HW, float S,
                                                             float* __restrict__ ws) {
  __shared__ float red[16];
  const int s = blockIdx.x, b = blockIdx.y;
  const float* f = flow + (long)b * 2 * HW;
  const float* g = gt + (long)b * 2 * HW;
  const float* m = mask + (long)b * HW;
  const float r = (float)dt_gt[b] / (float)dt_input[b];  // no guard: inf / nan like the float32 torch division
  const int p0 = s * AEE_STRIPE;
  const int p1 = p0 + AEE_STRIPE < HW ? p0 + AEE_STRIPE : HW;
  float se = 0.f, nv = 0.f, no = 0.f;
  if (VEC) {  // HW is a multiple of 4 and so are p0 and p1: whole float4s, 16-byte aligned
    for (int p = p0 + 4 * (int)threadIdx.x; p < p1; p += 4 * AEE_THREADS) {
      const float4 a0 = *(const float4*)(f + p), a1 = *(const float4*)(f + HW + p);
      const float4 g0 = *(const float4*)(g + p), g1 = *(const float4*)(g + HW + p);
      const float4 mm = *(const float4*)(m + p);
      aee_pixel(a0.x, a1.x, g0.x, g1.x, mm.x, S, r, se, nv, no);
      aee_pixel(a0.y, a1.y, g0.y, g1.y, mm.y, S, r, se, nv, no);
      aee_pixel(a0.z, a1.z, g0.z, g1.z, mm.z, S, r, se, nv, no);
      aee_pixel(a0.w, a1.w, g0.w, g1.w, mm.w, S, r, se, nv, no);
    }
  } else {
    for (int p = p0 + (int)threadIdx.x; p < p1; p += AEE_THREADS) aee_pixel(f[p], f[HW + p], g[p], g[HW + p], m[p], S, r, se, nv, no);
  }
  se = evf_block_sum(se, red);
  nv = evf_block_sum(nv, red);
  no = evf_block_sum(no, red);
  if (threadIdx.x == 0) {
    float* w = ws + ((long)b * gridDim.x + s) * 3;
    w[0] = se;
    w[1] = nv;
    w[2] = no;
  }
}

// One block.  Thread t adds the stripes of samples t, t + AEE_THREADS, ... in stripe order and leaves the sample's sums in the
// sample's FIRST triple (its own, which it has read already); thread 0 then walks the samples in order.  The outlier count is
// summed over the whole batch before the division (the quirk AEE.forward keeps, loss/flow.py:626).  A row word outside
// 0 .. nrows - 1 returns before any store, the workspace included.
__global__ void __launch_bounds__(AEE_THREADS) k_aee_finish(float* __restrict__ ws, int B, int S, const long long* __restrict__ row,
                                                            long long nrows, float* __restrict__ log, long long row_floats,
                                                            int offset) {
  const long long r = evf_log_row(row, 1, 0, nrows);
  if (r < 0) return;
  for (int b = threadIdx.x; b < B; b += AEE_THREADS) {
    float* w = ws + (long)b * S * 3;
    float se = 0.f, nv = 0.f, no = 0.f;
    for (int s = 0; s < S; ++s) {
      se += w[3 * s];
      nv += w[3 * s + 1];
      no += w[3 * s + 2];
    }
    w[0] = se;
    w[1] = nv;
    w[2] = no;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float* d = log + r * row_floats + offset;
  float outliers = 0.f;
  for (int b = 0; b < B; ++b) outliers += ws[(long)b * S * 3 + 2];
  float sum_aee = 0.f, sum_pct = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* w = ws + (long)b * S * 3;
    const float aee = w[0] / (w[1] + 1e-9f), pct = outliers / (w[1] + 1e-9f);
    d[b] = aee;
    d[B + 1 + b] = pct;
    sum_aee += aee;
    sum_pct += pct;
  }
  d[B] = sum_aee / (float)B;
  d[2 * B + 1] = sum_pct / (float)B;
}

extern "C" int evf_aee_at_stripes(int H, int W) {
  if (H <= 0 || W <= 0 || (int64_t)H * W > 2147483647LL - AEE_STRIPE) return EVF_EINVAL;
  return evf_cdiv((long)H * W, AEE_STRIPE);
}

extern "C" int evf_aee_at(const float* flow, const float* gt, const float* mask, const double* dt_gt, const double* dt_input, int B,
                          int H, int W, float flow_scaling, const int64_t* row, int64_t nrows, float* log, int64_t row_floats,
                          int offset, float* ws, int64_t ws_floats, void* stream) {
  if (!flow || !gt || !mask || !dt_gt || !dt_input || !ws) return EVF_EINVAL;
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0) return EVF_EINVAL;
  if (!evf_log_dest_ok(row, nrows, log, row_floats, offset, 2 * ((int64_t)B + 1))) return EVF_EINVAL;
  const int S = evf_aee_at_stripes(H, W);
  if (S < 1 || S > 65535) return EVF_EINVAL;
  if (ws_floats < (int64_t)B * S * 3) return EVF_EINVAL;
  if (((uintptr_t)ws & 3u) || ((uintptr_t)flow & 3u) || ((uintptr_t)gt & 3u) || ((uintptr_t)mask & 3u) || ((uintptr_t)dt_gt & 7u) ||
      ((uintptr_t)dt_input & 7u))
    return EVF_EINVAL;
  const int HW = H * W;
  const bool vec = (W % 4 == 0) && !(((uintptr_t)flow | (uintptr_t)gt | (uintptr_t)mask) & 15u);
  if (vec)
    hipLaunchKernelGGL(k_aee_stripes<true>, dim3(S, B), dim3(AEE_THREADS), 0, EVF_STREAM(stream), flow, gt, mask, dt_gt, dt_input, HW,
                       flow_scaling, ws);
  else
    hipLaunchKernelGGL(k_aee_stripes<false>, dim3(S, B), dim3(AEE_THREADS), 0, EVF_STREAM(stream), flow, gt, mask, dt_gt, dt_input, HW,
                       flow_scaling, ws);
  int rc = evf_status();
  if (rc != EVF_OK) return rc;
  hipLaunchKernelGGL(k_aee_finish, dim3(1), dim3(AEE_THREADS), 0, EVF_STREAM(stream), ws, B, S, (const long long*)row,
                     (long long)nrows, log, (long long)row_floats, offset);
  return evf_status();
}

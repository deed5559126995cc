// What the 3x3 stride-1 bf16x3 convolution kernels share: k_conv3_b3t (evf_conv_b3tile.hip), k_conv3_b3i (evf_conv_b3img.hip),
// k_conv3_b3n (evf_conv_b3n.hip) and k_conv3_b3x (evf_conv_b3small.hip), chosen between by b3_launch (evf_conv_b3gen.hip).
//
// Operands.  Weights w = hi + mid + lo, three bf16 planes packed by evf_pack_conv2d_weight_b3 (evf_conv_b3gen.hip) as uint4
// [N tile 32][tap][64-channel group][16-channel chunk 4][term 3][lane 64].  Activations are split on the fly, exactly, into the same
// three planes (evf_split3_pair) and staged per 16-channel group as LDS planes of 48 B per halo pixel (16 channels x bf16 + 16 B
// pad: conflict-free b128 reads).  Products run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, the weights as the A operand:
// the tile comes out transposed, a lane owns one pixel and 4 x 4 consecutive channels per N tile.
//
// THE ARITHMETIC CONTRACT is b3_mma3 / b3_mma6 below -- the only places of the family where the order of the products is written.
// A block-uniform vote per channel group (B3Halo::commit: is some residual of the staged tile not zero?) picks between them; with
// mid = lo = 0 the six-term form adds exact zeros to the three-term one, so the vote never changes a result.  Per output element
// the channel groups are added in index order, split-K partial sums go to slabs that are added in index order (k_b3_reduce):
// every member of the family gives the same bits for the same product.
#pragma once
#include "evf_common.h"
#include "evf_split.h"

typedef float b3_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 b3_bf16x8 __attribute__((ext_vector_type(8)));
typedef float b3_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t b3_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void b3_lds_void;
typedef __attribute__((address_space(1))) const void b3_glb_void;

// Exact input (all residuals zero): w x = (lo + mid + hi) x, smallest terms first.
__device__ __forceinline__ void b3_mma3(b3_f32x16& acc, b3_bf16x8 wh, b3_bf16x8 wm, b3_bf16x8 wl, b3_bf16x8 x) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wm, x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, x, acc, 0, 0, 0);
}

// Real-valued input: the six terms of (hi + mid + lo)(xh + xm + xl) above 2^-24 of the leading one, smallest terms first.
__device__ __forceinline__ void b3_mma6(b3_f32x16& acc, b3_bf16x8 wh, b3_bf16x8 wm, b3_bf16x8 wl, b3_bf16x8 xh, b3_bf16x8 xm,
                                        b3_bf16x8 xl) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wm, xm, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, xh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wm, xh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xm, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xh, acc, 0, 0, 0);
}

// Four channels of one halo pixel -> the three planes (p: the pixel's 8 bytes in the hi plane; written if `store`).  Returns the mid
// halves: bf16 of the residuals, zero iff the residual is zero (-0 cannot arise from x - head(x)).
__device__ __forceinline__ uint32_t b3_split_store(b3_f32x4 v, char* p, int plane, bool store) {
  uint32_t h0, m0, l0, h1, m1, l1;
  evf_split3_pair(v.x, v.y, h0, m0, l0);
  evf_split3_pair(v.z, v.w, h1, m1, l1);
  if (store) {
    *(uint2*)(p) = make_uint2(h0, h1);
    *(uint2*)(p + plane) = make_uint2(m0, m1);
    *(uint2*)(p + 2 * plane) = make_uint2(l0, l1);
  }
  return m0 | m1;
}

// Staging of the halo of a ROWS x COLS output tile by THREADS threads, 16 channels (one group kc) at a time: global float4 ->
// registers (fetch, before the matrix phase) -> exact split -> three LDS planes (commit, behind it).
template <int ROWS, int COLS, int THREADS>
struct B3Halo {
  static constexpr int HR = ROWS + 2, HC = COLS + 2, PIX = HR * HC;
  static constexpr int PITCH = 48;            // bytes per halo pixel and plane
  static constexpr int PLANE = PIX * PITCH;   // bytes per plane
  static constexpr int TASKS = PIX * 4;       // float4 loads per group
  static constexpr int ITER = (TASKS + THREADS - 1) / THREADS;

  // img: the image of this block, (y0, x0): the tile's first output pixel, g: the kernel's geometry (H, W, K, lds).  Loads are
  // unconditional from clamped addresses.
  template <class Geo>
  static __device__ __forceinline__ void fetch(b3_f32x4 (&pa)[ITER], const float* img, int y0, int x0, const Geo& g, int kc, int tid) {
#pragma unroll
    for (int i = 0; i < ITER; ++i) {
      const int task = min(tid + THREADS * i, TASKS - 1), px = task >> 2, q = task & 3;
      const int hy = px / HC, hx = px - hy * HC;
      const int sy = min(max(y0 + hy - 1, 0), g.H - 1), sx = min(max(x0 + hx - 1, 0), g.W - 1);
      const int c = kc * 16 + 4 * q;
      pa[i] = *(const b3_f32x4*)(img + ((long)sy * g.W + sx) * g.lds + (c + 4 <= g.K ? c : 0));
    }
  }
  // returns "some residual is not zero" for this thread's elements (pixels outside the image and channels past K are zeros)
  template <class Geo>
  static __device__ __forceinline__ int commit(const b3_f32x4 (&pa)[ITER], char* s_a, int y0, int x0, const Geo& g, int kc, int tid) {
    uint32_t nz = 0u;
#pragma unroll
    for (int i = 0; i < ITER; ++i) {
      const int task = tid + THREADS * i, px = task >> 2, q = task & 3;
      const int hy = px / HC, hx = px - hy * HC;
      const int sy = y0 + hy - 1, sx = x0 + hx - 1;
      const bool ok = sy >= 0 && sy < g.H && sx >= 0 && sx < g.W && kc * 16 + 4 * q + 4 <= g.K;
      const b3_f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
      const b3_f32x4 v = ok ? pa[i] : zero4;
      nz |= b3_split_store(v, s_a + px * PITCH + q * 8, PLANE, task < TASKS);
    }
    return (nz & 0x7FFF7FFFu) != 0u;
  }
};

// split-K: split z of ksplit owns the channel groups [lo, hi) of KC (an empty split still writes its zeros).  The caller moves its
// output pointer to slab z.
__device__ __forceinline__ void b3_split_range(int KC, int ksplit, int z, int& lo, int& hi) {
  lo = 0, hi = KC;
  if (ksplit > 1) {
    const int per = (KC + ksplit - 1) / ksplit;
    lo = min(z * per, KC - 1), hi = min(lo + per, KC);
    if (z * per >= KC) hi = lo;
  }
}

#define B3_STAGE (4 * 3 * 64)  // uint4 per (N tile, tap, 64-channel group) of the packed weights: [chunk 4][term 3][lane 64]
// In the packed weights of one N tile (wt): lane `lane` of the fragment (tap, channel group kc of 16, term)
__device__ __forceinline__ const uint4* b3_wfrag(const uint4* wt, int tap, int G64, int kc, int term, int lane) {
  return wt + (((long)tap * G64 + (kc >> 2)) * 4 + (kc & 3)) * 192 + term * 64 + lane;
}

// Store of one N tile of one lane's pixel (orow): accumulator registers 4 q + e = channels n0 + 8 q + e (n0 = 32 tile + 4 kg);
// bias, accumulate, float4 where the row is aligned (vec) and the quad complete.
__device__ __forceinline__ void b3_store_tile(const b3_f32x16& acc, float* orow, int n0, int N, const float* bias, int accumulate,
                                              bool vec) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = n0 + 8 * q;
    if (n >= N) continue;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float x = acc[4 * q + e];
      if (bias && n + e < N) x += bias[n + e];
      if (accumulate && n + e < N) x += orow[n + e];
      v[e] = x;
    }
    if (vec && n + 4 <= N) {
      *(float4*)(orow + n) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n + e < N) orow[n + e] = v[e];
    }
  }
}

// Host side: the K splits of a plan.  blocks = blocks of the unsplit launch, KC = channel groups of 16.  At least `unsplit_at`
// blocks: no split; else enough splits for `target` blocks, at least four channel groups each, at most max_split (the slabs the
// caller's scratch holds).  force_split > 0 (EVF_CONV_SPLIT, evf_conv_split_select) overrides the shape's choice.
static inline int b3_plan_splits(long blocks, int KC, int max_split, int force_split, long unsplit_at, long target) {
  const int smax = max(1, min(max_split, KC / 4));
  int ks = blocks >= unsplit_at ? 1 : (int)min((long)smax, evf_cdiv(target, blocks));
  if (force_split > 0) ks = max(1, min(min(force_split, max(max_split, 1)), KC));
  return ks;
}

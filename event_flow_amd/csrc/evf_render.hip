// Stored visualisations colour-coded on the device (utils/visualization.py, Visualization(render="device")): every image of a
// pass -- count images, flow maps, frames, for every sample of the batch -- becomes one [H][W][3] uint8 tile of a frame sheet
// in ONE launch, so a stored pass costs one kernel and one copy instead of up to eight copies, three sorts per count image and
// the HSV arithmetic in numpy.
//
//   evf_render_sheet   out[b][k][H][W][3] = colour coding of image k of sample b, k < nimg <= 8.
//
// One block of 1024 threads per (sample, image).  No other block touches that image or its tile, so there is no grid-wide
// synchronisation, no ticket and no atomic on global memory; every pass of a block over its image (at most 2^18 pixels, 2 MB:
// L2 resident) is a strided loop.  All arithmetic that decides a colour is float64 in the order of the numpy code it mirrors,
// without FMA contraction, so the count images equal the host renderer byte for byte.
//
// EVF_RENDER_COUNTS needs the 1st and 99th percentile of both channels: the order statistics k and min(k + 1, n - 1) at both
// positions.  They are EXACT: a radix select on order-preserving 32-bit keys, most significant byte first, the two positions of
// a channel served by two 256-bin LDS histograms filled in the same pass over the data.  A thread adds a RUN of equal digits
// with one LDS atomic (count images are mostly zeros: without that every add of a pass would hit one bin).  The histograms
// are integer counts, so the order of the atomic adds does not show in the result.  After four passes the key of order
// statistic k is known together with its rank among its equals; the next order statistic is the same value if another equal
// follows, else the smallest key above it (one more pass, taken only then).  Every bin index is (key >> shift) & 255: bounded
// by construction, whatever the input bits (a NaN is just a key at one end of the order).
#include "evf_common.h"

#pragma clang fp contract(off)

#define RENDER_THREADS 1024
#define RENDER_WAVES (RENDER_THREADS / 64)
#define RENDER_MAX_IMG 8
#define RENDER_MAX_PIXELS (1 << 18)

struct RenderSrc {
  const void* src[RENDER_MAX_IMG];
  int kind[RENDER_MAX_IMG];
};

// float -> uint32 whose unsigned order is the float order (-0.0 just below +0.0), and back
__device__ __forceinline__ uint32_t render_key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float render_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

struct RenderSel {
  uint32_t hist[2][256];
  uint32_t wave_sum[8];
  uint32_t prefix[2];  // the selected key's bytes so far
  uint32_t rank[2];    // rank of the order statistic among the elements that share `prefix`
  uint32_t equal[2];   // number of elements in the bin chosen last
  uint32_t above[2];   // smallest key above the selected one
};

// Order statistics k[j] and min(k[j] + 1, n - 1), j = 0, 1, of x[0 .. n - 1]: v[2 j], v[2 j + 1], the same in every thread.
__device__ void render_select2(const float* __restrict__ x, int n, const uint32_t (&k)[2], RenderSel& s, float (&v)[4]) {
  const int tid = threadIdx.x;
  if (tid < 2) {
    s.prefix[tid] = 0u;
    s.rank[tid] = k[tid];
    s.equal[tid] = 0u;
    s.above[tid] = 0xffffffffu;
  }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const uint32_t mask = pass ? (0xffffffffu << (shift + 8)) : 0u;  // the bytes already decided
    if (tid < 512) (&s.hist[0][0])[tid] = 0u;
    __syncthreads();
    const uint32_t pre0 = s.prefix[0], pre1 = s.prefix[1], r0 = s.rank[0], r1 = s.rank[1];
    uint32_t run0 = 0u, run1 = 0u, dig0 = 0u, dig1 = 0u;
    for (int i = tid; i < n; i += RENDER_THREADS) {
      const uint32_t key = render_key(x[i]);
      const uint32_t d = (key >> shift) & 255u;
      if (((key ^ pre0) & mask) == 0u) {
        if (d != dig0 && run0) {
          atomicAdd(&s.hist[0][dig0], run0);
          run0 = 0u;
        }
        dig0 = d;
        ++run0;
      }
      if (((key ^ pre1) & mask) == 0u) {
        if (d != dig1 && run1) {
          atomicAdd(&s.hist[1][dig1], run1);
          run1 = 0u;
        }
        dig1 = d;
        ++run1;
      }
    }
    if (run0) atomicAdd(&s.hist[0][dig0], run0);
    if (run1) atomicAdd(&s.hist[1][dig1], run1);
    __syncthreads();
    // inclusive scan of both histograms by threads 0 .. 511 (waves 0-3: position 0, waves 4-7: position 1)
    uint32_t h = 0u, incl = 0u;
    if (tid < 512) {
      h = (&s.hist[0][0])[tid];
      incl = h;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if ((tid & 63) >= o) incl += up;
      }
      if ((tid & 63) == 63) s.wave_sum[tid >> 6] = incl;
    }
    __syncthreads();
    if (tid < 512) {
      const int j = tid >> 8, w = tid >> 6;
      for (int q = 4 * j; q < w; ++q) incl += s.wave_sum[q];
      const uint32_t excl = incl - h, r = j ? r1 : r0;
      if (h && excl <= r && r < incl) {  // exactly one bin per position
        s.prefix[j] = (j ? pre1 : pre0) | ((uint32_t)(tid & 255) << shift);
        s.rank[j] = r - excl;
        s.equal[j] = h;
      }
    }
    __syncthreads();
  }
  const uint32_t key0 = s.prefix[0], key1 = s.prefix[1];
  // the next order statistic: another equal, the last element itself, or the smallest key above
  const bool up0 = k[0] + 1u < (uint32_t)n && s.rank[0] + 1u >= s.equal[0];
  const bool up1 = k[1] + 1u < (uint32_t)n && s.rank[1] + 1u >= s.equal[1];
  if (up0 || up1) {  // (the same decision in every thread: LDS words behind a barrier)
    uint32_t m0 = 0xffffffffu, m1 = 0xffffffffu;
    for (int i = tid; i < n; i += RENDER_THREADS) {
      const uint32_t key = render_key(x[i]);
      if (key > key0 && key < m0) m0 = key;
      if (key > key1 && key < m1) m1 = key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t a = __shfl_xor(m0, o, 64), b = __shfl_xor(m1, o, 64);
      m0 = a < m0 ? a : m0;
      m1 = b < m1 ? b : m1;
    }
    if ((tid & 63) == 0) {
      atomicMin(&s.above[0], m0);
      atomicMin(&s.above[1], m1);
    }
    __syncthreads();
  }
  v[0] = render_unkey(key0);
  v[1] = up0 ? render_unkey(s.above[0]) : v[0];
  v[2] = render_unkey(key1);
  v[3] = up1 ? render_unkey(s.above[1]) : v[2];
  __syncthreads();  // (s is reused by the next channel)
}

// numpy's _lerp (lib/_function_base_impl.py) in float64: a + (b - a) g, and b - (b - a) (1 - g) from g = 0.5 on
__device__ __forceinline__ double render_lerp(double a, double b, double g) {
  const double d = b - a;
  return g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
}
__device__ __forceinline__ double render_clip01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }
// np.clip(np.rint(x), 0, 255).astype(uint8); a NaN gives 0
__device__ __forceinline__ uint8_t render_u8_rint(double x) {
  const double r = rint(x);
  return r >= 0.0 ? (r <= 255.0 ? (uint8_t)(int)r : (uint8_t)255) : (uint8_t)0;
}
// x.astype(uint8) of a value in [0, 255]: truncation; clipped outside, a NaN gives 0
__device__ __forceinline__ uint8_t render_u8_trunc(double x) { return x >= 0.0 ? (x <= 255.0 ? (uint8_t)(int)x : (uint8_t)255) : (uint8_t)0; }

// events_to_image(...) * 255 -> rint -> clip (utils/visualization.py), in PNG channel order
__device__ void render_counts(const float* __restrict__ x, int n, int scheme, int k_lo, double g_lo, int k_hi, double g_hi,
                              uint8_t* __restrict__ out, RenderSel& s) {
  const uint32_t k[2] = {(uint32_t)k_lo, (uint32_t)k_hi};
  double lo[2], hi[2];
  for (int c = 0; c < 2; ++c) {
    float v[4];
    render_select2(x + (long)c * n, n, k, s, v);
    lo[c] = render_lerp((double)v[0], (double)v[1], g_lo);
    hi[c] = render_lerp((double)v[2], (double)v[3], g_hi);
  }
  const double top = hi[0] > hi[1] ? hi[0] : hi[1];  // max(p99(pos), p99(neg))
  for (int i = threadIdx.x; i < n; i += RENDER_THREADS) {
    double c01[2];
    for (int c = 0; c < 2; ++c) {
      const double xv = (double)x[(long)c * n + i];
      c01[c] = render_clip01(lo[c] != top ? (xv - lo[c]) / (top - lo[c]) : xv);
    }
    uint8_t* o = out + 3 * (long)i;
    if (scheme == 1) {  // gray
      const uint8_t g = render_u8_rint((0.5 + 0.5 * c01[0] - 0.5 * c01[1]) * 255.0);
      o[0] = g;
      o[1] = g;
      o[2] = g;
    } else {  // green_red: R = negative, G = positive
      o[0] = render_u8_rint(c01[1] * 255.0);
      o[1] = render_u8_rint(c01[0] * 255.0);
      o[2] = 0;
    }
  }
}

// block-wide minimum and maximum of doubles, the same in every thread
__device__ void render_minmax(double& lo, double& hi, double* red /* 2 * RENDER_WAVES */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double a = __shfl_xor(lo, o, 64), b = __shfl_xor(hi, o, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[2 * w] = lo;
    red[2 * w + 1] = hi;
  }
  __syncthreads();
  lo = red[0];
  hi = red[1];
  for (int q = 1; q < RENDER_WAVES; ++q) {
    lo = red[2 * q] < lo ? red[2 * q] : lo;
    hi = red[2 * q + 1] > hi ? red[2 * q + 1] : hi;
  }
  __syncthreads();
}

// flow_to_image (utils/visualization.py) in float64 from the float32 components
__device__ void render_flow(const float* __restrict__ f, int n, uint8_t* __restrict__ out, double* red) {
  const double PI = 3.141592653589793;
  double lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < n; i += RENDER_THREADS) {
    const double m = hypot((double)f[i], (double)f[n + i]);
    lo = m < lo ? m : lo;
    hi = m > hi ? m : hi;
  }
  render_minmax(lo, hi, red);
  const double span = hi - lo;
  for (int i = threadIdx.x; i < n; i += RENDER_THREADS) {
    const double fx = (double)f[i], fy = (double)f[n + i];
    const double m = hypot(fx, fy);
    const double val = span != 0.0 ? (m - lo) / span : m - lo;
    const double hue = (atan2(fy, fx) + PI) / (2.0 * PI);
    // _hsv_to_rgb with s = 1
    const double h6 = hue * 6.0;
    const double fl = floor(h6);
    const double fr = h6 - fl;
    const double p = val * (1.0 - 1.0), q = val * (1.0 - 1.0 * fr), t = val * (1.0 - 1.0 * (1.0 - fr));
    const int sector = (fl >= 0.0 && fl < 12.0) ? (int)fl % 6 : 0;  // (a NaN hue: any colour, no index)
    double r, g, b;
    switch (sector) {
      case 0: r = val, g = t, b = p; break;
      case 1: r = q, g = val, b = p; break;
      case 2: r = p, g = val, b = t; break;
      case 3: r = p, g = q, b = val; break;
      case 4: r = t, g = p, b = val; break;
      default: r = val, g = p, b = q; break;
    }
    uint8_t* o = out + 3 * (long)i;
    o[0] = render_u8_trunc(255.0 * r);
    o[1] = render_u8_trunc(255.0 * g);
    o[2] = render_u8_trunc(255.0 * b);
  }
}

__global__ void __launch_bounds__(RENDER_THREADS) k_render_sheet(RenderSrc rs, int nimg, int n, int scheme, int k_lo, double g_lo,
                                                                  int k_hi, double g_hi, uint8_t* __restrict__ out) {
  __shared__ RenderSel sel;
  __shared__ double red[2 * RENDER_WAVES];
  const int img = blockIdx.x % nimg, b = blockIdx.x / nimg;
  uint8_t* o = out + (long)blockIdx.x * n * 3;  // tile (b, img) of [B][nimg][H][W][3]
  const int kind = rs.kind[img];
  if (kind == EVF_RENDER_COUNTS) {
    render_counts((const float*)rs.src[img] + (long)b * 2 * n, n, scheme, k_lo, g_lo, k_hi, g_hi, o, sel);
  } else if (kind == EVF_RENDER_FLOW) {
    render_flow((const float*)rs.src[img] + (long)b * 2 * n, n, o, red);
  } else {  // EVF_RENDER_FRAME: channel 1 of uint8 [B,2,H,W]
    const uint8_t* f = (const uint8_t*)rs.src[img] + ((long)b * 2 + 1) * n;
    for (int i = threadIdx.x; i < n; i += RENDER_THREADS) {
      const uint8_t g = f[i];
      o[3 * (long)i] = g;
      o[3 * (long)i + 1] = g;
      o[3 * (long)i + 2] = g;
    }
  }
}

extern "C" int evf_render_sheet(const void* const* src, const int* kind, int nimg, int B, int H, int W, int scheme, int k_lo,
                                double g_lo, int k_hi, double g_hi, uint8_t* out, void* stream) {
  if (!src || !kind || !out || nimg < 1 || nimg > RENDER_MAX_IMG) return EVF_EINVAL;
  if (B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > RENDER_MAX_PIXELS || (int64_t)B * nimg > 65535) return EVF_EINVAL;
  if (scheme != 0 && scheme != 1) return EVF_EINVAL;
  const int n = H * W;
  if (k_lo < 0 || k_lo > n - 1 || k_hi < 0 || k_hi > n - 1) return EVF_EINVAL;
  if (!(g_lo >= 0.0 && g_lo < 1.0) || !(g_hi >= 0.0 && g_hi < 1.0)) return EVF_EINVAL;  // (a NaN fails both comparisons)
  RenderSrc rs;
  for (int k = 0; k < RENDER_MAX_IMG; ++k) {
    rs.src[k] = nullptr;
    rs.kind[k] = EVF_RENDER_FRAME;
    if (k >= nimg) continue;
    if (!src[k]) return EVF_EINVAL;
    if (kind[k] != EVF_RENDER_COUNTS && kind[k] != EVF_RENDER_FLOW && kind[k] != EVF_RENDER_FRAME) return EVF_EINVAL;
    if (kind[k] != EVF_RENDER_FRAME && ((uintptr_t)src[k] & 3u)) return EVF_EINVAL;
    rs.src[k] = src[k];
    rs.kind[k] = kind[k];
  }
  hipLaunchKernelGGL(k_render_sheet, dim3(B * nimg), dim3(RENDER_THREADS), 0, EVF_STREAM(stream), rs, nimg, n, scheme, k_lo, g_lo, k_hi,
                     g_hi, out);
  return evf_status();
}

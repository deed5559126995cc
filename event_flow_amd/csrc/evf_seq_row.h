// One event of a cut window as its 16-byte row (t, y, x, p): event_formatting / augment_events of dataloader/base.py:60-100 for
// k_seq_cut (evf_resident.hip) and k_seq_cut_ragged (evf_resident_eval.hip).  Built with -ffp-contract=off; the float division
// is the correctly rounded one, so the normalised timestamps carry numpy's bits: keep the expression order.
#pragma once
#include "evf_common.h"

// Thread n of a job that reads events f .. f + c - 1 of the arena.  `live` false (the job is refused, or row n lies behind its
// events): a padding row, and from thread 0 dt = 0.  `*flag`: bit 0 flips x, bit 1 flips y, bit 2 the polarity.
__device__ __forceinline__ void evf_seq_row(const uint16_t* __restrict__ xs, const uint16_t* __restrict__ ys,
                                            const double* __restrict__ ts, const uint8_t* __restrict__ ps, bool live, long f, long c,
                                            int n, const int* __restrict__ flag, int H, int W, float4* __restrict__ row,
                                            double* __restrict__ dt) {
  if (!live) {
    *row = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n == 0) *dt = 0.0;
    return;
  }
  const int fl = *flag;
  const double d0 = ts[f], d1 = ts[f + c - 1];
  const float t0 = (float)d0, t1 = (float)d1;  // base.py:64: float32 first, then the normalisation in float32
  const float t = ((float)ts[f + n] - t0) / (t1 - t0);
  float x = (float)xs[f + n], y = (float)ys[f + n];
  float pol = (float)ps[f + n] * 2.0f - 1.0f;
  if (fl & 1) x = (float)(W - 1) - x;
  if (fl & 2) y = (float)(H - 1) - y;
  if (fl & 4) pol = -pol;
  *row = make_float4(t, y, x, pol);
  if (n == 0) *dt = d1 - d0;
}

// evf_seq_row for k_ring_cut (evf_stream.hip): the columns are a ring of R slots, and the job's events sit at slots h, h + 1, ..
// modulo R (h = f mod R in [0, R), c <= R).  The same expressions in the same order as above; only the three indices differ.
__device__ __forceinline__ void evf_seq_row_ring(const uint16_t* __restrict__ xs, const uint16_t* __restrict__ ys,
                                                 const double* __restrict__ ts, const uint8_t* __restrict__ ps, bool live, long h,
                                                 long R, long c, int n, const int* __restrict__ flag, int H, int W,
                                                 float4* __restrict__ row, double* __restrict__ dt) {
  if (!live) {
    *row = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n == 0) *dt = 0.0;
    return;
  }
  const long last = h + c - 1 >= R ? h + c - 1 - R : h + c - 1, at = h + n >= R ? h + n - R : h + n;
  const int fl = *flag;
  const double d0 = ts[h], d1 = ts[last];
  const float t0 = (float)d0, t1 = (float)d1;  // base.py:64: float32 first, then the normalisation in float32
  const float t = ((float)ts[at] - t0) / (t1 - t0);
  float x = (float)xs[at], y = (float)ys[at];
  float pol = (float)ps[at] * 2.0f - 1.0f;
  if (fl & 1) x = (float)(W - 1) - x;
  if (fl & 2) y = (float)(H - 1) - y;
  if (fl & 4) pol = -pol;
  *row = make_float4(t, y, x, pol);
  if (n == 0) *dt = d1 - d0;
}

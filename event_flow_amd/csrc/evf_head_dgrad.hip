// The head layer's backward of a window in the EPILOGUE of its input-gradient products: k_dgrad_head_win.
//
// The head cell (layer 0) receives dL/d(spikes) of pass t as the product W_ff(layer 1)^T . g_cur(layer 1, t).  On the recorded
// path that product ran inside a diagonal launch of k_dgrad_diag_dma and wrote 128 bytes per pixel, which k_head_bwd_win read
// back after the last diagonal.  Here the ten products of a window run in ONE persistent launch built from the loops of
// k_dgrad_diag_dma<FULL> (evf_dgrad_diag.hip), and a tile of dL/d(spikes) never leaves the block:
//
//   items    tile-major, the passes of a tile consecutive from the window's last to its first; a block owns whole tiles, so the
//            values a pixel carries from pass t + 1 to t (dL/dv and the potential loaded as v_prev, which is the next item's
//            v_out) stay in registers of the lane that owns the pixel -- what gvc / voc are in head_bwd_pass<.., NT > 0>;
//   weights  one set for the whole launch;
//   waves 0..3  matrix waves, one per SIMD: dg_matrix_phase3 (same terms, same accumulator order: g_z has the bits it had);
//               behind the second MFMA of item k the accumulators of item k - 1 go to the wave's staging tile, a few MFMAs
//               later an LDS word says so.  They issue no vector-memory instruction at all;
//   waves 4..7  loader waves: the LDS-DMA pieces of item k + 1, the element-wise operands of item k (v_prev, the spike word, the
//               input halo), and -- new -- the head cell's backward of item k - 1 on the staging tile of the matrix wave of
//               their SIMD, read row-wise (8 pixels x 128 bytes per instruction): the FAST expression of head_bwd_pass (arctan
//               surrogate, hard reset) element by element, the per-channel sums, and the head's weight gradient
//               dW[co][(ci, tap)] as VALU sums (4 pixels x 4 channels per lane; two lanes with adjacent pixels split the
//               columns by input channel: 20 packed accumulator pairs at Cin <= 2, 36 at Cin = 3).
//   hand-over   ONE staging tile per wave pair: written during item k (after barrier k - 1), read by the loader wave before
//               barrier k; "written" is the LDS word (the waves of a block are co-resident; no block waits for another).
//   sums        kept over all tiles and passes of the block, reduced once at the end into the block's row of the slab
//               [rows][32 * 9 * Cin] and of the per-block parameter rows.  The launch has fewer blocks than the slab has rows:
//               with accumulate = 0 a block also zeroes the rows blockIdx + j * gridDim it does not own.
// dL/dv leaving the window is bit-identical to k_dgrad_diag_dma + k_head_bwd_win; the sums differ in grouping only.
#include "evf_common.h"
#include "evf_dgrad_mma.h"
#include <stdlib.h>
#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void hw_lds_void;
typedef __attribute__((address_space(1))) const void hw_glb_void;

#define C32 32
#define HW_ROWS 4
#define HW_HW 34
#define HW_HP ((HW_ROWS + 2) * HW_HW)  // 204 halo pixels
#define HW_NFRAG 54
#define HW_SP 36                   // floats per pixel of the staging tile
#define HW_UPP 13                  // 16-pixel DMA units per plane
#define HW_PLANE (HW_UPP * 64)     // uint4 per plane
#define HW_BUF (3 * HW_PLANE)      // uint4 per halo buffer
#define HW_NU (3 * HW_UPP)         // DMA pieces per item
#define HW_NJ ((HW_NU + 3) / 4)    // pieces per loader wave
#define HW_XMAX (4 * HW_HP)        // floats per input-halo buffer (Cin <= 3, padded to an even channel count)
#define HW_LDS ((size_t)(HW_NFRAG * 64 + 2 * HW_BUF) * sizeof(uint4) + (size_t)4 * 32 * HW_SP * 4 + (size_t)2 * HW_XMAX * 4)  // + 16 static

__device__ uint4 hw_zero_page[16];  // 256 bytes of zeros: the DMA source of out-of-image halo pixels

// (the expressions of evf_network.hip, head_bwd_pass<FAST>: the library is built with -ffp-contract=off, the same bits here)
__device__ __forceinline__ float hw_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float hw_arctan_sg(float x, float width) { return __builtin_amdgcn_rcpf(1.0f + width * x * x); }

struct HwTile {
  int b, y0, x0, s;
};

template <int CIN>
__global__ __launch_bounds__(512) void k_dgrad_head_win(EvfHdwArgs A, unsigned plane_bytes, int ntx, int nty, unsigned ntiles) {
  // The two lanes that hold horizontally adjacent pixels of a channel group split the weight-gradient columns by INPUT CHANNEL (an
  // odd Cin is padded with a channel of zeros, so that the other lane's columns are a fixed distance away in the input halo):
  // CH channels = NH columns per lane, NH2 pairs of them (packed fp32 FMAs)
  constexpr int NCOL = 9 * CIN, CH = (CIN + 1) / 2, NH = 9 * CH, NH2 = (NH + 1) / 2, NX = CIN * HW_HP, NXL = (NX + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  uint4* s_w = (uint4*)smem_raw;                 // [54][64]
  uint4* s_a = s_w + HW_NFRAG * 64;              // [2][3][HW_UPP * 16 pixels][4], chunk c of pixel p in slot c ^ ((p >> 2) & 3)
  float* s_stage = (float*)(s_a + 2 * HW_BUF);   // [4 waves][32 pixels][HW_SP]
  float* s_x = s_stage + 4 * 32 * HW_SP;         // [2][HW_XMAX]: the input halo [ci][6 rows][34 columns] of a tile
  __shared__ int s_flag[4];                      // staging tiles matrix wave w has written so far
  float* s_part = (float*)s_a;                   // (after the last item) [4 loader waves][32][NCOL] weight-gradient partials ...
  float* s_red = s_part + 4 * C32 * NCOL;        // ... and [2][4][32] per-channel partials
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned flag_lds = (unsigned)(uintptr_t)&s_flag[wv & 3];  // (its LDS address: read and written by ds instructions below)
  const int i = lane & 31, kg = lane >> 5;
  const int H = A.H, W = A.W, np = A.np;
  const unsigned tlo = (unsigned)(((unsigned long long)blockIdx.x * ntiles) / gridDim.x);
  const unsigned thi = (unsigned)(((unsigned long long)(blockIdx.x + 1) * ntiles) / gridDim.x);
  const int nitem = (int)(thi - tlo) * np;
  const bool loader = wv >= 4;
  float* st = s_stage + (wv & 3) * (32 * HW_SP);
  if (nitem > 0 && !loader) {
    // ------------------------------------------------------------------------------------------------ matrix waves
    auto epi_write = [&](const f32x16& a) {  // lane (pixel i, K half kg): 4 x 16 bytes of its pixel's 128-byte line
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *(float4*)(st + i * HW_SP + 8 * q + 4 * kg) = make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
    };
    auto publish = [&](int n) {  // the tile's writes have left the wave's LDS queue, then the word (the LDS serves a wave in order)
      asm volatile("s_waitcnt lgkmcnt(0)\n\tds_write_b32 %0, %1" ::"v"(flag_lds), "v"(n) : "memory");
    };
    f32x16 acc_prev = {0};
    auto run_item = [&](int k, auto epi_tag) {
      constexpr bool EPI = decltype(epi_tag)::value;
      auto side = [&](int slot) {
        if (EPI) {
          if (slot == 1) epi_write(acc_prev);  // (barrier k - 1 is behind us: the loader wave has read the tile before it)
          if (slot == 9) publish(k);
        }
      };
      acc_prev = dg_matrix_phase3<true>(s_w, s_a + (k & 1) * HW_BUF, HW_PLANE, wv * HW_HW + i, lane, side);
      __syncthreads();
    };
    __syncthreads();  // weights and the planes of item 0 are in LDS
    run_item(0, std::false_type{});
    for (int k = 1; k < nitem; ++k) run_item(k, std::true_type{});
    epi_write(acc_prev);
    publish(nitem);
  } else if (nitem > 0) {
    // ------------------------------------------------------------------------------------------------ loader waves
    const int w = wv & 3, cg = lane & 7, pr = lane >> 3, ltid = tid - 256;
    // items in order: (tile, pass), the pass fastest; tiles x-fastest, then y, then the sample.  Scalar counters: the block walks
    // its items one by one (the float-reciprocal index arithmetic of k_dgrad_diag_dma costs vector registers here)
    auto item_first = [&](HwTile& t) {
      const unsigned tx = tlo % (unsigned)ntx, r = tlo / (unsigned)ntx, ty = r % (unsigned)nty, b = r / (unsigned)nty;
      t.s = 0, t.x0 = __builtin_amdgcn_readfirstlane((int)tx * 32);
      t.b = __builtin_amdgcn_readfirstlane((int)b), t.y0 = __builtin_amdgcn_readfirstlane((int)ty * HW_ROWS);
    };
    auto item_next = [&](const HwTile& c, HwTile& t) {  // (the caller does not step past the block's last item)
      t = c;
      if (++t.s == np) {
        t.s = 0;
        if ((t.x0 += 32) == W) {
          t.x0 = 0;
          if ((t.y0 += HW_ROWS) == H) t.y0 = 0, ++t.b;
        }
      }
    };
    // the DMA pieces of this wave (k_dgrad_diag_dma): piece q = w + 4 j covers plane q / 13, pixels 16 u .. 16 u + 15 (the per-lane
    // geometry is loop-invariant: the compiler keeps it in registers, as the tables there)
    const char* zero_page = (const char*)hw_zero_page + (lane & 3) * 16;
    auto dma_piece = [&](int j, const HwTile& t, const char* g, int buf, int ln) {  // ln = lane >> 2
      const int q = min(w + 4 * j, HW_NU - 1), pl = q / HW_UPP, u = q - pl * HW_UPP;  // (wave-uniform)
      const int p = 16 * u + ln, pc = min(p, HW_HP - 1);
      const int hr = (pc * 1928) >> 16, hc = pc - hr * HW_HW;  // = pc / 34 for pc < 204
      const int y = t.y0 - 1 + hr, x = t.x0 - 1 + hc;
      const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
      const unsigned off = ((unsigned)(t.b * H + y) * (unsigned)W + (unsigned)x) * 64u + (unsigned)pl * plane_bytes +
                           (unsigned)(((lane & 3) ^ ((p >> 2) & 3)) * 16);
      const unsigned long long m = in ? ~0ull : 0ull;
      const unsigned long long a = (((unsigned long long)g + off) & m) | ((unsigned long long)zero_page & ~m);
      const int dst = __builtin_amdgcn_readfirstlane(pl * HW_PLANE + u * 64);
      __builtin_amdgcn_global_load_lds((hw_glb_void*)a, (hw_lds_void*)(s_a + buf * HW_BUF + dst), 16, 0, 0);
    };
    // the input halo of a tile, [ci][6][34] floats: element lt + 256 n of it is this lane's (lt = w * 64 + lane)
    auto x_geo = [&](int n, int lt, int& hr, int& hc, int& rel) {
      const int j = min(lt + 256 * n, NX - 1), ci = (j * 1286) >> 18, rem = j - ci * HW_HP;  // = j / 204 for j < 816
      hr = (rem * 1928) >> 16, hc = rem - hr * HW_HW;                                       // = rem / 34 for rem < 204
      rel = (ci * H + hr - 1) * W + hc - 1;  // from the tile's first pixel in channel 0
    };
    struct Ops {  // element-wise operands of an item: the potential before the pass and the spike word, 4 pixels of this lane
      float4 vp[4];
      uint32_t zw[4];
    };
    // (`ln`: the lane number behind an empty asm, per step -- what depends on the lane is then worked out where it is used, a few
    //  instructions, and not hoisted out of the loop into registers that the sums need)
    auto elem = [&](const HwTile& t, int r, int ln) -> unsigned {  // float4 index of (pixel 8 r + pr of this wave's row, channel group cg)
      return ((unsigned)((t.b * H + t.y0 + w) * W + t.x0 + 8 * r + (ln >> 3))) * 8u + (unsigned)(ln & 7);
    };
    auto fetch_ops = [&](const HwTile& t, Ops& o, int ln) {  // (unconditional loads, valid addresses; NULL: zeros at use)
      const float4* pvp = A.v_prev[t.s] ? (const float4*)A.v_prev[t.s] : (const float4*)A.v_out0;
      const uint32_t* pzw = A.z_prev[t.s] ? A.z_prev[t.s] : (const uint32_t*)A.v_out0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned e = elem(t, r, ln);
        o.vp[r] = pvp[e];
        o.zw[r] = pzw[e >> 3];
      }
    };
    auto fetch_x = [&](const HwTile& t, float (&xv)[NXL], int ln) {
      const float* px = A.x_in[t.s];
      const int base = ((t.b * CIN) * H + t.y0) * W + t.x0;
#pragma unroll
      for (int n = 0; n < NXL; ++n) {
        int hr, hc, rel;
        x_geo(n, w * 64 + ln, hr, hc, rel);
        const int y = t.y0 - 1 + hr, x = t.x0 - 1 + hc;
        const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        xv[n] = px[in ? base + rel : 0];
      }
    };
    auto store_x = [&](const HwTile& t, const float (&xv)[NXL], int buf, int ln) {
#pragma unroll
      for (int n = 0; n < NXL; ++n) {
        int hr, hc, rel;
        x_geo(n, w * 64 + ln, hr, hc, rel);
        const int j = w * 64 + ln + 256 * n;
        const int y = t.y0 - 1 + hr, x = t.x0 - 1 + hc;
        const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        if (j < NX) s_x[buf * HW_XMAX + j] = in ? xv[n] : 0.f;
      }
    };
    float lam[4], th[4], inv_oml[4], sl[4], sth[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lam[k] = hw_sigmoid(A.leak[4 * cg + k]);
      th[k] = fmaxf(A.thresh[4 * cg + k], 0.01f);
      inv_oml[k] = 1.0f / (1.0f - lam[k]);
      sl[k] = sth[k] = 0.f;
    }
    const float width = A.width;
    // dW[4 cg + c][columns half * NH + 2 j, + 1], half = pr & 1, summed over this lane's pixels AND those of lane ^ 8 (the pixel
    // beside, same channels): that lane's dL/d(current) comes over by DPP, and it sums the other half of the columns for both.
    // (All columns for the own pixels only would be twice the accumulators: 72 / 108 registers, which do not fit.)
    f32x2 dw[4][NH2];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int j = 0; j < NH2; ++j) dw[c][j] = f32x2{0.f, 0.f};
    // offset of column jj of a lane's NH in the input halo [ci][6][34], from its first channel
    auto col_off = [](int jj) -> int { return (jj / 9) * HW_HP + ((jj % 9) / 3) * HW_HW + (jj % 3); };
    float4 gvc[4], voc[4];  // carried from item to item of a tile: dL/dv, the potential behind the pass (= v_prev of the item before)
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // the head cell's backward of item `kdone - 1` (tile t) on the staging tile of matrix wave w
    auto process = [&](const HwTile& t, const Ops& o, int kdone, int ln) {
      const int cg = ln & 7, pr = ln >> 3, half = pr & 1;
      const bool has_vp = A.v_prev[t.s] != nullptr, has_z = A.z_prev[t.s] != nullptr;
      const bool last = t.s == np - 1;
      float4* gvp = (float4*)A.g_v_prev;
      for (;;) {  // (almost always there already: the tile was written ~4 k cycles ago)
        int seen;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(seen) : "v"(flag_lds) : "memory");
        if (__builtin_amdgcn_readfirstlane(seen) >= kdone) break;
        __builtin_amdgcn_s_sleep(1);
      }
      const float* xs = s_x + ((kdone - 1) & 1) * HW_XMAX;
      float4 gzr[4];  // the tile row-wise: 8 pixels x 128 bytes per instruction (Cin <= 2: requested together, one LDS wait)
      if (CIN < 3) {
#pragma unroll
        for (int r = 0; r < 4; ++r) gzr[r] = *(const float4*)(st + (8 * r + pr) * HW_SP + 4 * cg);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = 8 * r + pr;
        const float4 gz4 = CIN < 3 ? gzr[r] : *(const float4*)(st + p * HW_SP + 4 * cg);
        const float4 vo4 = voc[r], gv4 = gvc[r], vp4 = has_vp ? o.vp[r] : zero4;
        const uint32_t zw = has_z ? (o.zw[r] >> (4 * cg)) : 0u;
        const float vo[4] = {vo4.x, vo4.y, vo4.z, vo4.w}, gz[4] = {gz4.x, gz4.y, gz4.z, gz4.w};
        const float gvo[4] = {gv4.x, gv4.y, gv4.z, gv4.w}, vp[4] = {vp4.x, vp4.y, vp4.z, vp4.w};
        float gc[4], gp[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // head_bwd_pass<FAST>: arctan surrogate, hard reset
#ifdef HW_PROBE_NOELEM  // (probe build: the weight gradient without the neuron's arithmetic)
          gc[k] = gz[k], gp[k] = gvo[k] + vp[k] + vo[k] + (float)(zw & 1u);
          continue;
#endif
          const float z = (float)((zw >> k) & 1u);
          const float sg = hw_arctan_sg(vo[k] - th[k], width);
          const float gsp = gz[k] * sg;
          const float gv = gvo[k] + gsp;
          gc[k] = gv * (1.0f - lam[k]);
          gp[k] = gv * lam[k] * (1.0f - z);
          const float cur = (vo[k] - (vp[k] * lam[k]) * (1.0f - z)) * inv_oml[k];
          const float dlam = vp[k] * (1.0f - z) - cur;
          sl[k] += gv * dlam;
          sth[k] -= gsp;
        }
        gvc[r] = make_float4(gp[0], gp[1], gp[2], gp[3]);
        voc[r] = o.vp[r];
#ifdef HW_PROBE_NODW  // (probe build: the neuron's arithmetic without the weight gradient)
        sl[0] += gc[0] + gc[1] + gc[2] + gc[3];
        continue;
#endif
        // weight gradient: this lane's half of the 9 Cin input taps, of its own pixel and of the pixel of lane ^ 8, from the halo in LDS
        float gcn[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)  // row_ror:8 -- lane ^ 8 within its row of 16
          gcn[c] = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, gc[c]), 0x128, 0xF, 0xF, true));
        const float* xp = xs + half * (CH * HW_HP) + w * HW_HW + p;
        const float* xn = xs + half * (CH * HW_HP) + w * HW_HW + (p ^ 1);
#pragma unroll
        for (int j = 0; j < NH2; ++j) {
          const bool two = 2 * j + 1 < NH;
          const int o0 = col_off(2 * j), o1 = two ? col_off(2 * j + 1) : 0;
          const f32x2 xa = {xp[o0], two ? xp[o1] : 0.f}, xb = {xn[o0], two ? xn[o1] : 0.f};
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            dw[c][j] = __builtin_elementwise_fma(f32x2{gc[c], gc[c]}, xa, dw[c][j]);
            dw[c][j] = __builtin_elementwise_fma(f32x2{gcn[c], gcn[c]}, xb, dw[c][j]);
          }
        }
        // one pixel at a time: with the four pixels' LDS reads at the top and their FMAs at the bottom the body needs 240 registers
        // (no branch in this loop: across one, the FMAs sink to the end whatever the scheduling barrier says.  The `continue`s of
        //  the HW_PROBE_* builds above are unconditional: such a build drops the rest of the body at compile time)
        __builtin_amdgcn_sched_barrier(0);
      }
      if (last && gvp) {  // (block-uniform) dL/dv leaving the window
#pragma unroll
        for (int r = 0; r < 4; ++r) gvp[elem(t, r, ln)] = gvc[r];
      }
    };
    auto load_carry = [&](const HwTile& t, int ln) {  // a tile's first item: the potential behind the window's last pass, dL/dv entering it
      const float4* pvo = (const float4*)A.v_out0;
      const float4* pgv = A.g_v_out0 ? (const float4*)A.g_v_out0 : pvo;
      const bool has_gv = A.g_v_out0 != nullptr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned e = elem(t, r, ln);
        voc[r] = pvo[e];
        const float4 g = pgv[e];
        gvc[r] = has_gv ? g : zero4;
      }
    };

    __builtin_amdgcn_s_setprio(3);
    if (lane == 0) s_flag[w] = 0;
    for (int j = NX + ltid; j < 2 * CH * HW_HP; j += 256) s_x[j] = s_x[HW_XMAX + j] = 0.f;  // (the padding channel of an odd Cin)
    for (int u = w; u < HW_NFRAG; u += 4)
      __builtin_amdgcn_global_load_lds((hw_glb_void*)((const uint4*)A.wt + u * 64 + lane), (hw_lds_void*)(s_w + u * 64), 16, 0, 0);
    HwTile cur, nxt, prv;
    item_first(cur);
    prv = nxt = cur;
#pragma unroll
    for (int j = 0; j < HW_NJ; ++j) dma_piece(j, cur, (const char*)A.g[cur.s], 0, lane >> 2);
    load_carry(cur, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // Step k: request the planes of item k + 1 (LDS-DMA), the operands and the input halo of item k (registers); run the head cell's
    // backward of item k - 1; wait for every request; input halo to LDS; barrier.  Nothing is in flight across a barrier.
    // (nitem + 1 steps, the last one without requests and without a barrier: ONE copy of the element-wise body.)
    // Cin = 3 (72 accumulators): a second set of operand registers does not fit -- the operands are requested behind the element-wise
    // body instead and waited for at once (zero spills in every instantiation; the step is longer by a load latency there).
    constexpr bool TWO_SETS = CIN < 3;
    Ops o_old, o_new;
    for (int k = 0; k <= nitem; ++k) {
      const bool more = k < nitem;  // (block-uniform)
      float xv[NXL];
      int ln = lane;
      asm volatile("" : "+v"(ln));
      const int lt = TWO_SETS ? lane : ln;  // (Cin <= 2: the geometry of the DMA pieces and of the input halo stays in registers)
      if (more) {
        if (k + 1 < nitem) item_next(cur, nxt);  // (past the end: the last item again -- its DMA is issued and never used)
        const char* gn = (const char*)A.g[nxt.s];
#pragma unroll
        for (int j = 0; j < HW_NJ; ++j) dma_piece(j, nxt, gn, (k + 1) & 1, lt >> 2);
        if (TWO_SETS) fetch_ops(cur, o_new, ln);
        fetch_x(cur, xv, lt);
      }
#ifndef HW_PROBE_IDLE  // (probe build: the loader team requests and waits only -- what does the element-wise body cost the launch?)
#ifdef HW_PROBE_PRIO0  // (probe build: the element-wise body BEHIND the matrix wave of the SIMD in the arbitration)
      __builtin_amdgcn_s_setprio(0);
#endif
      if (k > 0) process(prv, TWO_SETS ? o_old : o_new, k, ln);
#ifdef HW_PROBE_PRIO0
      __builtin_amdgcn_s_setprio(3);
#endif
#endif
      if (!more) break;
      if (!TWO_SETS) {
        asm volatile("" : "+v"(ln)::"memory");
        fetch_ops(cur, o_new, ln);
      }
      if (k > 0 && cur.s == 0) load_carry(cur, ln);  // (block-uniform) the tile before is finished: its carries are dead
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      store_x(cur, xv, k & 1, lt);
      __syncthreads();  // planes of item k + 1 and the input halo of item k complete; planes of item k free
      if (TWO_SETS) o_old = o_new;
      prv = cur;
      cur = nxt;
    }
    // this wave's sums: across the lanes that share a channel group (and a column half), then to LDS (the halo buffers are free:
    // every DMA piece has landed before the last barrier, and the matrix waves read them before it)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int j = 0; j < NH2; ++j) {
        float a = dw[c][j].x, b = dw[c][j].y;
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
          a += __shfl_xor(a, o, 64);
          b += __shfl_xor(b, o, 64);
        }
        const int c0 = (pr & 1) * NH + 2 * j;  // (columns >= NCOL: the padding channel)
        if (lane < 16) {
          if (2 * j < NH && c0 < NCOL) s_part[(w * C32 + 4 * cg + c) * NCOL + c0] = a;
          if (2 * j + 1 < NH && c0 + 1 < NCOL) s_part[(w * C32 + 4 * cg + c) * NCOL + c0 + 1] = b;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int o = 8; o < 64; o <<= 1) {
        sl[k] += __shfl_xor(sl[k], o, 64);
        sth[k] += __shfl_xor(sth[k], o, 64);
      }
      if (lane < 8) {
        s_red[(0 * 4 + w) * C32 + 4 * cg + k] = sl[k];
        s_red[(1 * 4 + w) * C32 + 4 * cg + k] = sth[k];
      }
    }
  }
  __syncthreads();
  // ---------------------------------------------------------------------------------------------------- the block's rows
  const bool any = nitem > 0;  // (more blocks than tiles: a block without a tile adds zeros)
  float* sl_out = A.slab + (size_t)blockIdx.x * (C32 * NCOL);
  for (int e2 = tid; e2 < C32 * NCOL; e2 += 512) {
    const float v = any ? (s_part[e2] + s_part[C32 * NCOL + e2]) + (s_part[2 * C32 * NCOL + e2] + s_part[3 * C32 * NCOL + e2]) : 0.f;
    sl_out[e2] = (A.slab_acc ? sl_out[e2] : 0.f) + v;
  }
  if (!A.slab_acc) {  // the slab's rows no block of this launch owns read as zero
    for (int row = (int)blockIdx.x + (int)gridDim.x; row < A.nrows; row += (int)gridDim.x)
      for (int e2 = tid; e2 < C32 * NCOL; e2 += 512) A.slab[(size_t)row * (C32 * NCOL) + e2] = 0.f;
  }
  if (tid < 64 && any) {
    const int which = tid >> 5, c = tid & 31;
    float v = 0.f;
    for (int q = 0; q < 4; ++q) v += s_red[(which * 4 + q) * C32 + c];
    const size_t ro = (size_t)blockIdx.x * A.row_ld;
    if (which == 0) {
      const float l = hw_sigmoid(A.leak[c]), t = v * l * (1.0f - l);
      if (A.row_ld) A.g_leak[ro + c] += t;
      else evf_atomic_add(A.g_leak + c, t);
    } else if (A.thresh[c] > 0.01f) {  // clamp_min passes gradient only above the floor
      if (A.row_ld) A.g_thresh[ro + c] += v;
      else evf_atomic_add(A.g_thresh + c, v);
    }
  }
}

// -1: environment (EVF_HEAD_DGRAD_WIN=0 switches the path off, EVF_HEAD_DGRAD_BLOCKS=n sets the grid), read once
static int hw_on_select = -1, hw_blocks_select = 0;
extern "C" int evf_head_dgrad_win_select(int on, int blocks) {
  if (on < -1 || on > 1 || blocks < 0 || blocks > 4096) return EVF_EINVAL;
  hw_on_select = on, hw_blocks_select = blocks;
  return EVF_OK;
}
static bool hw_enabled() {
  static const bool env_on = []() {
    const char* e = getenv("EVF_HEAD_DGRAD_WIN");
    return !(e && e[0] == '0');
  }();
  return hw_on_select < 0 ? env_on : hw_on_select == 1;
}
static int hw_blocks() {
  static const int env_n = []() {
    const char* e = getenv("EVF_HEAD_DGRAD_BLOCKS");
    const int n = e ? atoi(e) : 0;
    return n >= 1 && n <= 4096 ? n : 0;
  }();
  return hw_blocks_select > 0 ? hw_blocks_select : env_n;
}

extern "C" int evf_head_dgrad_win_fits(int B, int Cin, int H, int W, int hard_reset, int surrogate, int split_planes,
                                       int planes_per_pass, int deterministic) {
  if (!hw_enabled() || B <= 0 || H <= 0 || W <= 0) return 0;
  if (hard_reset != 1 || surrogate != EVF_ARCTAN) return 0;  // LIF head, FAST neuron (bits 1-2 of the flag: XLIF / ALIF heads)
  if (Cin < 1 || Cin > 3) return 0;
  if (H % HW_ROWS != 0 || W % 32 != 0 || !evf_dgrad_diag_fits(1, B, H, W)) return 0;
  if ((long)B * Cin * H * W >= (1L << 31)) return 0;
  if (!split_planes || !planes_per_pass || deterministic) return 0;
  return 1;
}

int evf_head_dgrad_win_launch(const EvfHdwArgs& A, void* stream) {
  if (A.np < 1 || A.np > EVF_HDW_MAX_P || !A.wt || !A.v_out0 || !A.leak || !A.thresh || !A.g_leak || !A.g_thresh || !A.slab ||
      A.nrows < 1)
    return EVF_EINVAL;
  for (int t = 0; t < A.np; ++t)
    if (!A.g[t] || !A.x_in[t]) return EVF_EINVAL;
  // the potential a pass loads as v_prev is carried as the next pass's v_out: only the LAST pass of the launch (the window's first)
  // may start from the zero state (NULL) -- its substitute loads are discarded at use and carried nowhere
  for (int t = 0; t + 1 < A.np; ++t)
    if (!A.v_prev[t]) return EVF_EINVAL;
  const int B = A.B, H = A.H, W = A.W;
  if (B <= 0 || H <= 0 || W <= 0 || A.Cin < 1 || A.Cin > 3 || H % HW_ROWS != 0 || W % 32 != 0 || !evf_dgrad_diag_fits(1, B, H, W) ||
      (long)B * A.Cin * H * W >= (1L << 31))
    return EVF_ENOTSUP;
  const int ntx = W / 32, nty = H / HW_ROWS;
  const long ntiles = (long)ntx * nty * B;
  const long plane_bytes = (long)B * H * W * 64;
  if (ntiles * A.np >= (1L << 22) || 3 * plane_bytes >= (1L << 32)) return EVF_ENOTSUP;
  static int ncu = 0;
  if (!ncu) {
    int dev = 0;
    hipDeviceProp_t pr;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess) ncu = pr.multiProcessorCount;
    if (ncu <= 0) ncu = 256;
  }
  long nblk = hw_blocks() > 0 ? hw_blocks() : (ntiles < ncu ? ntiles : ncu);  // one block per CU (155 KiB of LDS each)
  if (nblk > A.nrows) nblk = A.nrows;  // (a block writes its own row of the slab and of the parameter rows)
  evf_dynamic_lds_once<k_dgrad_head_win<1>>(HW_LDS);
  evf_dynamic_lds_once<k_dgrad_head_win<2>>(HW_LDS);
  evf_dynamic_lds_once<k_dgrad_head_win<3>>(HW_LDS);
#define HW_GO(CIN_)                                                                                                           \
  hipLaunchKernelGGL(k_dgrad_head_win<CIN_>, dim3((unsigned)nblk), dim3(512), HW_LDS, EVF_STREAM(stream), A, (unsigned)plane_bytes, \
                     ntx, nty, (unsigned)ntiles)
  if (A.Cin == 1) HW_GO(1);
  else if (A.Cin == 2) HW_GO(2);
  else HW_GO(3);
#undef HW_GO
  return evf_status();
}

// Host-side guards of evf_render_sheet (csrc/evf_render.hip) as a stand-alone program: every EVF_EINVAL case of the contract in
// include/evflow.h must be answered before any launch.  Built with the host sanitizers, it needs no GPU and launches nothing:
// every call here is a refused one (the stand-in pointers are host memory; accepted calls are the GPU tests' business).
//
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -I event_flow_amd/csrc -I include tools/render_guards.cpp event_flow_amd/csrc/evf_render.hip -o render_guards
#include <cmath>
#include <cstdint>
#include <cstdio>

extern "C" int evf_render_sheet(const void* const* src, const int* kind, int nimg, int B, int H, int W, int scheme, int k_lo,
                                double g_lo, int k_hi, double g_hi, uint8_t* out, void* stream);

static int failures = 0;
static void expect(const char* what, int got, int want) {
  if (got != want) {
    std::printf("FAIL %s: status %d, expected %d\n", what, got, want);
    ++failures;
  }
}

// stand-ins for device memory: the guards compare and align pointers, they never dereference them
struct Args {
  const void* src[9];
  int kind[9];
  bool null_src, null_kind;
  int nimg, B, H, W, scheme, k_lo;
  double g_lo;
  int k_hi;
  double g_hi;
  uint8_t* out;
  int call() const {
    return evf_render_sheet(null_src ? nullptr : src, null_kind ? nullptr : kind, nimg, B, H, W, scheme, k_lo, g_lo, k_hi, g_hi, out,
                            nullptr);
  }
};

int main() {
  const int EINVAL_ = -22;
  alignas(16) static float planes[64];
  alignas(16) static uint8_t sheet[64];
  // three images of B = 2 samples of 5 x 7 pixels: counts, flow, frame (a frame may sit at any byte address)
  Args ok = {};
  ok.src[0] = planes;
  ok.src[1] = planes + 16;
  ok.src[2] = (const char*)planes + 33;
  ok.kind[0] = 0;
  ok.kind[1] = 1;
  ok.kind[2] = 2;
  for (int k = 3; k < 9; ++k) ok.src[k] = planes, ok.kind[k] = 0;
  ok.nimg = 3, ok.B = 2, ok.H = 5, ok.W = 7, ok.scheme = 0;
  ok.k_lo = 0, ok.g_lo = 0.34, ok.k_hi = 33, ok.g_hi = 0.66;
  ok.out = sheet;
  Args a;
#define BAD(what, stmt) \
  a = ok;               \
  stmt;                 \
  expect(what, a.call(), EINVAL_)
  BAD("null src", a.null_src = true);
  BAD("null kind", a.null_kind = true);
  BAD("null out", a.out = nullptr);
  BAD("null src[0]", a.src[0] = nullptr);
  BAD("null src[2]", a.src[2] = nullptr);
  for (int v : {0, -1, 9, 2147483647, -2147483647 - 1}) {
    BAD("nimg outside 1..8", a.nimg = v);
  }
  for (int v : {-1, 3, 2147483647}) {
    BAD("an unknown kind", a.kind[1] = v);
    BAD("an unknown scheme", a.scheme = v == 3 ? 2 : v);
  }
  for (int v : {0, -1, -2147483647 - 1}) {
    BAD("a non-positive B", a.B = v);
    BAD("a non-positive H", a.H = v);
    BAD("a non-positive W", a.W = v);
  }
  BAD("2^18 + 1 pixels", a.H = 1; a.W = (1 << 18) + 1; a.k_hi = 100);
  BAD("2^18 + 512 pixels", a.H = 513; a.W = 512; a.k_hi = 100);
  BAD("2^62 pixels", a.H = 2147483647; a.W = 2147483647);
  BAD("2^32 pixels (H W wraps to 0 in int)", a.H = 65536; a.W = 65536);
  BAD("B nimg = 65536", a.B = 21846);
  BAD("B = 2^31 - 1", a.B = 2147483647);
  BAD("B nimg wraps in int", a.B = 1431655766);
  BAD("a negative k_lo", a.k_lo = -1);
  BAD("k_lo = H W", a.k_lo = 35);
  BAD("a negative k_hi", a.k_hi = -1);
  BAD("k_hi = H W", a.k_hi = 35);
  BAD("k_hi = 2^31 - 1", a.k_hi = 2147483647);
  BAD("g_lo = 1", a.g_lo = 1.0);
  BAD("a negative g_lo", a.g_lo = -1e-300);
  BAD("g_lo NaN", a.g_lo = std::nan(""));
  BAD("g_lo inf", a.g_lo = INFINITY);
  BAD("g_hi = 1", a.g_hi = 1.0);
  BAD("a negative g_hi", a.g_hi = -0.5);
  BAD("g_hi NaN", a.g_hi = std::nan(""));
  BAD("counts that are not 4-byte aligned", a.src[0] = (const char*)planes + 2);
  BAD("a flow that is not 4-byte aligned", a.src[1] = (const char*)planes + 65);
#undef BAD
  std::printf(failures ? "%d guard(s) failed\n" : "all guards answered EVF_EINVAL before any launch\n", failures);
  return failures ? 1 : 0;
}

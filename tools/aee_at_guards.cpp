// Host-side guards of evf_aee_at (csrc/evf_eval_log.hip) as a stand-alone program: every EVF_EINVAL case of the contract in
// include/evflow.h must be answered before any launch.  Built with the host sanitizers, it needs no GPU: the one accepted call
// at the end reports the launch's status (an error without a device) and is not judged.
//
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -I event_flow_amd/csrc -I include tools/aee_at_guards.cpp event_flow_amd/csrc/evf_eval_log.hip -o aee_at_guards
#include <cstdint>
#include <cstdio>

extern "C" int evf_aee_at_stripes(int H, int W);
extern "C" int evf_aee_at(const float* flow, const float* gt, const float* mask, const double* dt_gt, const double* dt_input, int B,
                          int H, int W, float flow_scaling, const int64_t* row, int64_t nrows, float* log, int64_t row_floats,
                          int offset, float* ws, int64_t ws_floats, void* stream);

static int failures = 0;
static void expect(const char* what, int got, int want) {
  if (got != want) {
    std::printf("FAIL %s: status %d, expected %d\n", what, got, want);
    ++failures;
  }
}

// stand-ins for device memory: the guards compare and align pointers, they never dereference them
struct Args {
  const float *flow, *gt, *mask;
  const double *dt_gt, *dt_input;
  int B, H, W;
  const int64_t* row;
  int64_t nrows;
  float* log;
  int64_t row_floats;
  int offset;
  float* ws;
  int64_t ws_floats;
  int call() const {
    return evf_aee_at(flow, gt, mask, dt_gt, dt_input, B, H, W, 32.0f, row, nrows, log, row_floats, offset, ws, ws_floats, nullptr);
  }
};

int main() {
  const int EINVAL_ = -22;
  alignas(16) static float planes[4 * 64];
  alignas(16) static double dts[8];
  alignas(16) static int64_t row_word[2] = {0, 0};
  alignas(16) static float log_[4 * 32];
  alignas(16) static float ws_[64];
  // B = 3 samples of 45 x 91 pixels: two stripes, a workspace of 18 floats, a row of 8 floats behind offset 5
  const Args ok = {planes, planes + 64, planes + 128, dts, dts + 4, 3, 45, 91, row_word, 4, log_, 32, 5, ws_, 18};
  expect("stripes of 45 x 91", evf_aee_at_stripes(45, 91), 2);
  expect("stripes of 1 x 2048", evf_aee_at_stripes(1, 2048), 1);
  expect("stripes of no rows", evf_aee_at_stripes(0, 91), EINVAL_);
  expect("stripes of a negative width", evf_aee_at_stripes(45, -2147483647 - 1), EINVAL_);
  expect("stripes of 2^31 pixels", evf_aee_at_stripes(65536, 32768), EINVAL_);
  expect("stripes of 2^62 pixels", evf_aee_at_stripes(2147483647, 2147483647), EINVAL_);
  Args a;
#define BAD(what, stmt)         \
  a = ok;                       \
  stmt;                         \
  expect(what, a.call(), EINVAL_)
  BAD("null flow", a.flow = nullptr);
  BAD("null gt", a.gt = nullptr);
  BAD("null mask", a.mask = nullptr);
  BAD("null dt_gt", a.dt_gt = nullptr);
  BAD("null dt_input", a.dt_input = nullptr);
  BAD("null row", a.row = nullptr);
  BAD("null log", a.log = nullptr);
  BAD("null ws", a.ws = nullptr);
  for (int v : {0, -1, -2147483647 - 1}) {
    BAD("a non-positive B", a.B = v);
    BAD("a non-positive H", a.H = v);
    BAD("a non-positive W", a.W = v);
    BAD("a non-positive nrows", a.nrows = v);
    BAD("a non-positive row length", a.row_floats = v);
  }
  BAD("B beyond the grid", a.B = 65536; a.row_floats = 1 << 20; a.ws_floats = (int64_t)1 << 40);
  BAD("B = 2^31 - 1", a.B = 2147483647; a.row_floats = (int64_t)1 << 40; a.ws_floats = (int64_t)1 << 40);
  BAD("more stripes than the grid", a.H = 32768; a.W = 8192; a.ws_floats = (int64_t)1 << 40);
  BAD("2^31 pixels", a.H = 65536; a.W = 32768; a.ws_floats = (int64_t)1 << 40);
  BAD("a negative offset", a.offset = -1);
  BAD("offset + 2 (B + 1) one float behind the row", a.offset = 25);
  BAD("offset = 2^31 - 1", a.offset = 2147483647);
  BAD("a row shorter than 2 (B + 1)", a.row_floats = 7; a.offset = 0);
  BAD("a workspace one float short", a.ws_floats = 17);
  BAD("a workspace of no floats", a.ws_floats = 0);
  BAD("a negative workspace size", a.ws_floats = -18);
  BAD("a log that is not 4-byte aligned", a.log = (float*)((char*)log_ + 2));
  BAD("a workspace that is not 4-byte aligned", a.ws = (float*)((char*)ws_ + 1));
  BAD("a flow that is not 4-byte aligned", a.flow = (const float*)((const char*)planes + 2));
  BAD("a gt that is not 4-byte aligned", a.gt = (const float*)((const char*)planes + 3));
  BAD("a mask that is not 4-byte aligned", a.mask = (const float*)((const char*)planes + 1));
  BAD("a dt_gt that is not 8-byte aligned", a.dt_gt = (const double*)((const char*)dts + 4));
  BAD("a dt_input that is not 8-byte aligned", a.dt_input = (const double*)((const char*)dts + 4));
  BAD("a row word that is not 8-byte aligned", a.row = (const int64_t*)((const char*)row_word + 4));
#undef BAD
  a = ok;
  a.offset = 24;  // the last offset that fits
  const int rc = a.call();
  std::printf("accepted arguments: status %d (0 with a device; the launch's error without one)\n", rc);
  if (rc == EINVAL_) ++failures;
  std::printf(failures ? "%d guard(s) failed\n" : "all guards answered EVF_EINVAL before any launch\n", failures);
  return failures ? 1 : 0;
}

// Host-side guards of evf_rings_append and evf_rings_cut_ragged (csrc/evf_stream.hip) as a stand-alone program: every EVF_EINVAL
// case of the contract in include/evflow.h must be answered before any launch.  Built with the host sanitizers, it needs no GPU:
// the program makes no accepted call that launches, so it never launches (its pointers are host memory).
//
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -I event_flow_amd/csrc -I include tools/rig_stream_guards.cpp event_flow_amd/csrc/evf_stream.hip -o rig_stream_guards
#include <cstdint>
#include <cstdio>

extern "C" int evf_rings_append(const void* staged, int B, int n, int most, uint16_t* xs, uint16_t* ys, double* ts, uint8_t* ps,
                                int64_t R, void* stream);
extern "C" int evf_rings_cut_ragged(const uint16_t* xs, const uint16_t* ys, const double* ts, const uint8_t* ps, int64_t R,
                                    const int64_t* first, const int64_t* appended, const int* count, const int* flags, int B,
                                    int Npad, int H, int W, float* ev, double* dt_input, void* stream);

static int failures = 0;
static void expect(const char* what, int got, int want) {
  if (got != want) {
    std::printf("FAIL %s: status %d, expected %d\n", what, got, want);
    ++failures;
  }
}

// stand-ins for device memory: the guards compare and align pointers, they never dereference them
struct Append {
  const void* staged;
  int B, n, most;
  uint16_t *xs, *ys;
  double* ts;
  uint8_t* ps;
  int64_t R;
  int call() const { return evf_rings_append(staged, B, n, most, xs, ys, ts, ps, R, nullptr); }
};
struct Cut {
  const uint16_t *xs, *ys;
  const double* ts;
  const uint8_t* ps;
  int64_t R;
  const int64_t *first, *appended;
  const int *count, *flags;
  int B, Npad, H, W;
  float* ev;
  double* dt;
  int call() const { return evf_rings_cut_ragged(xs, ys, ts, ps, R, first, appended, count, flags, B, Npad, H, W, ev, dt, nullptr); }
};

int main() {
  const int EINVAL_ = -22;
  alignas(16) static unsigned char staged[8 * 7 + 13 * 3 * 64];
  alignas(16) static int64_t words[8];
  alignas(16) static uint16_t xs[3 * 64], ys[3 * 64];
  alignas(16) static double ts[3 * 64], dt[4];
  alignas(16) static uint8_t ps[3 * 64];
  alignas(16) static int count[4], flags[4];
  alignas(16) static float ev[3 * 16 * 4 + 4];
  const Append ok = {staged, 3, 70, 40, xs, ys, ts, ps, 64};
  Append a;
#define BAD(what, stmt) \
  a = ok;               \
  stmt;                 \
  expect(what, a.call(), EINVAL_)
  BAD("append: null staged buffer", a.staged = nullptr);
  BAD("append: null xs", a.xs = nullptr);
  BAD("append: null ys", a.ys = nullptr);
  BAD("append: null ts", a.ts = nullptr);
  BAD("append: null ps", a.ps = nullptr);
  for (int v : {0, -1, 17, 2147483647, -2147483647 - 1}) {
    BAD("append: B outside [1, 16]", a.B = v);
  }
  for (int v : {-1, -2147483647 - 1}) {
    BAD("append: n < 0", a.n = v);
    BAD("append: most < 0", a.most = v);
  }
  for (int v : {65, 70, 2147483647}) {
    BAD("append: a per-camera count above R", (a.most = v, a.n = v));
  }
  BAD("append: a per-camera count above n", a.most = 71);
  BAD("append: more events than B cameras of `most` hold", a.most = 23);
  BAD("append: more events than B cameras of `most` hold (beyond int32)", (a.B = 16, a.R = 2147483647, a.n = 2147483647, a.most = 1));
  for (int64_t v : {(int64_t)0, (int64_t)-1, INT64_MIN}) {
    BAD("append: R < 1", a.R = v);
  }
  BAD("append: a staged buffer that is not 8-byte aligned", a.staged = staged + 4);
  BAD("append: a ts column that is not 8-byte aligned", a.ts = (double*)((char*)ts + 4));
  BAD("append: an xs column that is not 2-byte aligned", a.xs = (uint16_t*)((char*)xs + 1));
  BAD("append: a ys column that is not 2-byte aligned", a.ys = (uint16_t*)((char*)ys + 1));
#undef BAD
  a = ok;
  a.n = a.most = 0;
  expect("append: no events is accepted and launches nothing", a.call(), 0);

  const Cut okc = {xs, ys, ts, ps, 64, words, words + 3, count, flags, 3, 16, 8, 8, ev, dt};
  Cut c;
#define BAD(what, stmt) \
  c = okc;              \
  stmt;                 \
  expect(what, c.call(), EINVAL_)
  BAD("cut: null xs", c.xs = nullptr);
  BAD("cut: null ys", c.ys = nullptr);
  BAD("cut: null ts", c.ts = nullptr);
  BAD("cut: null ps", c.ps = nullptr);
  BAD("cut: null first", c.first = nullptr);
  BAD("cut: null appended", c.appended = nullptr);
  BAD("cut: null count", c.count = nullptr);
  BAD("cut: null flags", c.flags = nullptr);
  BAD("cut: null ev", c.ev = nullptr);
  BAD("cut: null dt_input", c.dt = nullptr);
  for (int64_t v : {(int64_t)0, (int64_t)-1, INT64_MIN}) {
    BAD("cut: R < 1", c.R = v);
  }
  for (int v : {0, -1, 17, 2147483647, -2147483647 - 1}) {
    BAD("cut: B outside [1, 16]", c.B = v);
  }
  for (int v : {0, -1, -2147483647 - 1}) {
    BAD("cut: a non-positive Npad", c.Npad = v);
    BAD("cut: a non-positive H", c.H = v);
    BAD("cut: a non-positive W", c.W = v);
  }
  BAD("cut: a first column that is not 8-byte aligned", c.first = (const int64_t*)((const char*)words + 4));
  BAD("cut: an appended column that is not 8-byte aligned", c.appended = (const int64_t*)((const char*)words + 28));
  BAD("cut: a count column that is not 4-byte aligned", c.count = (const int*)((const char*)count + 2));
  BAD("cut: a flags column that is not 4-byte aligned", c.flags = (const int*)((const char*)flags + 2));
  BAD("cut: a ts column that is not 8-byte aligned", c.ts = (const double*)((const char*)ts + 4));
  BAD("cut: an xs column that is not 2-byte aligned", c.xs = (const uint16_t*)((const char*)xs + 1));
  BAD("cut: a ys column that is not 2-byte aligned", c.ys = (const uint16_t*)((const char*)ys + 1));
  BAD("cut: rows that are not 16-byte aligned", c.ev = ev + 1);
  BAD("cut: a dt_input that is not 8-byte aligned", c.dt = (double*)((char*)dt + 4));
#undef BAD
  std::printf(failures ? "%d guard(s) failed\n" : "all guards answered EVF_EINVAL before any launch\n", failures);
  return failures ? 1 : 0;
}

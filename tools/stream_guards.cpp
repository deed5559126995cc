// Host-side guards of evf_ring_append and evf_ring_cut (csrc/evf_stream.hip) as a stand-alone program: every EVF_EINVAL case of
// the contract in include/evflow.h must be answered before any launch.  Built with the host sanitizers, it needs no GPU: the
// program makes no accepted call that launches, so it never launches (its pointers are host memory).
//
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -I event_flow_amd/csrc -I include tools/stream_guards.cpp event_flow_amd/csrc/evf_stream.hip -o stream_guards
#include <cstdint>
#include <cstdio>

extern "C" int evf_ring_append(const void* chunk, int n, const int64_t* head, uint16_t* xs, uint16_t* ys, double* ts, uint8_t* ps,
                               int64_t R, void* stream);
extern "C" int evf_ring_cut(const uint16_t* xs, const uint16_t* ys, const double* ts, const uint8_t* ps, int64_t R,
                            const int64_t* first, const int64_t* appended, const int* flags, int B, int P, int N, int H, int W,
                            float* ev, double* dt_input, void* stream);

static int failures = 0;
static void expect(const char* what, int got, int want) {
  if (got != want) {
    std::printf("FAIL %s: status %d, expected %d\n", what, got, want);
    ++failures;
  }
}

// stand-ins for device memory: the guards compare and align pointers, they never dereference them
struct Append {
  const void* chunk;
  int n;
  const int64_t* head;
  uint16_t *xs, *ys;
  double* ts;
  uint8_t* ps;
  int64_t R;
  int call() const { return evf_ring_append(chunk, n, head, xs, ys, ts, ps, R, nullptr); }
};
struct Cut {
  const uint16_t *xs, *ys;
  const double* ts;
  const uint8_t* ps;
  int64_t R;
  const int64_t *first, *appended;
  const int* flags;
  int B, P, N, H, W;
  float* ev;
  double* dt;
  int call() const { return evf_ring_cut(xs, ys, ts, ps, R, first, appended, flags, B, P, N, H, W, ev, dt, nullptr); }
};

int main() {
  const int EINVAL_ = -22;
  alignas(16) static unsigned char chunk[8 + 13 * 64];
  alignas(16) static int64_t words[4] = {0, 0, 0, 0};
  alignas(16) static uint16_t xs[64], ys[64];
  alignas(16) static double ts[64], dt[4];
  alignas(16) static uint8_t ps[64];
  alignas(16) static int flags[4];
  alignas(16) static float ev[4 * 64 * 4];
  const Append ok = {chunk + 8, 7, words, xs, ys, ts, ps, 64};
  Append a;
#define BAD(what, stmt) \
  a = ok;               \
  stmt;                 \
  expect(what, a.call(), EINVAL_)
  BAD("append: null chunk", a.chunk = nullptr);
  BAD("append: null head", a.head = nullptr);
  BAD("append: null xs", a.xs = nullptr);
  BAD("append: null ys", a.ys = nullptr);
  BAD("append: null ts", a.ts = nullptr);
  BAD("append: null ps", a.ps = nullptr);
  for (int v : {-1, -2147483647 - 1}) {
    BAD("append: n < 0", a.n = v);
  }
  for (int v : {65, 2147483647}) {
    BAD("append: n > R", a.n = v);
  }
  for (int64_t v : {(int64_t)0, (int64_t)-1, INT64_MIN}) {
    BAD("append: R < 1", a.R = v);
  }
  BAD("append: n > R = 1", (a.R = 1, a.n = 2));
  BAD("append: a chunk that is not 8-byte aligned", a.chunk = chunk + 4);
  BAD("append: a head word that is not 8-byte aligned", a.head = (const int64_t*)((const char*)words + 4));
  BAD("append: a ts column that is not 8-byte aligned", a.ts = (double*)((char*)ts + 4));
  BAD("append: an xs column that is not 2-byte aligned", a.xs = (uint16_t*)((char*)xs + 1));
  BAD("append: a ys column that is not 2-byte aligned", a.ys = (uint16_t*)((char*)ys + 1));
#undef BAD
  a = ok;
  a.n = 0;
  expect("append: no events is accepted and launches nothing", a.call(), 0);

  const Cut okc = {xs, ys, ts, ps, 64, words, words + 1, flags, 2, 2, 16, 8, 8, ev, dt};
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
  BAD("cut: null flags", c.flags = nullptr);
  BAD("cut: null ev", c.ev = nullptr);
  BAD("cut: null dt_input", c.dt = nullptr);
  for (int64_t v : {(int64_t)0, (int64_t)-1, INT64_MIN}) {
    BAD("cut: R < 1", c.R = v);
  }
  for (int v : {0, -1, -2147483647 - 1}) {
    BAD("cut: a non-positive B", c.B = v);
    BAD("cut: a non-positive P", c.P = v);
    BAD("cut: a non-positive N", c.N = v);
    BAD("cut: a non-positive H", c.H = v);
    BAD("cut: a non-positive W", c.W = v);
  }
  BAD("cut: B * P > 65535", (c.B = 256, c.P = 256));
  BAD("cut: B * P beyond int32", (c.B = 2147483647, c.P = 2147483647));
  BAD("cut: a first word that is not 8-byte aligned", c.first = (const int64_t*)((const char*)words + 4));
  BAD("cut: an appended word that is not 8-byte aligned", c.appended = (const int64_t*)((const char*)words + 12));
  BAD("cut: rows that are not 16-byte aligned", c.ev = ev + 1);
#undef BAD
  std::printf(failures ? "%d guard(s) failed\n" : "all guards answered EVF_EINVAL before any launch\n", failures);
  return failures ? 1 : 0;
}

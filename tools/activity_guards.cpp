// Host-side guards of evf_activity_at (csrc/evf_activity.hip) as a stand-alone program: every EVF_EINVAL case of the contract in
// include/evflow.h must be answered before any launch.  Built with the host sanitizers, it needs no GPU: the program makes no
// accepted call, so it never launches (its pointers are host memory).
//
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -I event_flow_amd/csrc -I include tools/activity_guards.cpp event_flow_amd/csrc/evf_activity.hip -o activity_guards
#include <cstdint>
#include <cstdio>

extern "C" int evf_activity_parts(int64_t n_max);
extern "C" int evf_activity_at(const void* const* src, const int* kind, const int64_t* n, int nsrc, int B, const int64_t* row,
                               int64_t row_mul, int64_t row_add, int64_t nrows, uint32_t* log, void* stream);

static int failures = 0;
static void expect(const char* what, int got, int want) {
  if (got != want) {
    std::printf("FAIL %s: status %d, expected %d\n", what, got, want);
    ++failures;
  }
}

// stand-ins for device memory: the guards compare and align pointers, they never dereference them
struct Args {
  const void* src[16];
  int kind[16];
  int64_t n[16];
  const void* const* srcp;
  const int* kindp;
  const int64_t* np;
  int nsrc, B;
  const int64_t* row;
  int64_t row_mul, row_add, nrows;
  uint32_t* log;
  int call() const {
    return evf_activity_at(srcp ? src : nullptr, kindp ? kind : nullptr, np ? n : nullptr, nsrc, B, row, row_mul, row_add, nrows, log,
                           nullptr);
  }
};

int main() {
  const int EINVAL_ = -22;
  const int64_t N_MAX = ((int64_t)1 << 27) - 1;
  alignas(16) static uint32_t data[64];
  alignas(16) static int64_t row_word[2] = {0, 0};
  alignas(16) static uint32_t log_[64];
  Args ok = {};
  for (int k = 0; k < 16; ++k) {
    ok.src[k] = data + k;  // (any 4-byte alignment serves)
    ok.kind[k] = k & 1;
    ok.n[k] = 1 + k;
  }
  ok.srcp = ok.src, ok.kindp = ok.kind, ok.np = ok.n;
  ok.nsrc = 16, ok.B = 3, ok.row = row_word, ok.row_mul = 3, ok.row_add = 2, ok.nrows = 4, ok.log = log_;
  expect("parts of one element", evf_activity_parts(1) >= 1 ? 0 : 1, 0);
  expect("parts of 2^27 - 1 elements", evf_activity_parts(N_MAX) >= 1 ? 0 : 1, 0);
  expect("parts of no elements", evf_activity_parts(0), EINVAL_);
  expect("parts of a negative size", evf_activity_parts(-1), EINVAL_);
  expect("parts of 2^27 elements", evf_activity_parts(N_MAX + 1), EINVAL_);
  expect("parts of 2^63 - 1 elements", evf_activity_parts(INT64_MAX), EINVAL_);
  Args a;
#define BAD(what, stmt)         \
  a = ok;                       \
  stmt;                         \
  expect(what, a.call(), EINVAL_)
  BAD("null src", a.srcp = nullptr);
  BAD("null kind", a.kindp = nullptr);
  BAD("null n", a.np = nullptr);
  BAD("null row", a.row = nullptr);
  BAD("null log", a.log = nullptr);
  BAD("a null source", a.src[0] = nullptr);
  BAD("a null last source", a.src[15] = nullptr);
  for (int v : {0, -1, 17, 2147483647, -2147483647 - 1}) {
    BAD("nsrc outside 1..16", a.nsrc = v);
  }
  for (int v : {-1, 2, 2147483647, -2147483647 - 1}) {
    BAD("an unknown kind", a.kind[5] = v);
  }
  for (int64_t v : {(int64_t)0, (int64_t)-1, N_MAX + 1, (int64_t)1 << 31, (int64_t)1 << 32, INT64_MAX, INT64_MIN}) {
    BAD("n[k] outside 1 .. 2^27 - 1", a.n[7] = v);
  }
  for (int v : {0, -1, -2147483647 - 1, 65536, 2147483647}) {
    BAD("B outside 1..65535", a.B = v);
  }
  for (int64_t v : {(int64_t)0, (int64_t)-1, INT64_MIN}) {
    BAD("a non-positive nrows", a.nrows = v);
  }
  for (int64_t v : {(int64_t)-1, INT64_MIN}) {
    BAD("a negative row_mul", a.row_mul = v);
    BAD("a negative row_add", a.row_add = v);
  }
  BAD("a source that is not 4-byte aligned", a.src[3] = (const char*)data + 2);
  BAD("a last source that is not 4-byte aligned", a.src[15] = (const char*)data + 1);
  BAD("a log that is not 4-byte aligned", a.log = (uint32_t*)((char*)log_ + 2));
  BAD("a row word that is not 8-byte aligned", a.row = (const int64_t*)((const char*)row_word + 4));
#undef BAD
  std::printf(failures ? "%d guard(s) failed\n" : "all guards answered EVF_EINVAL before any launch\n", failures);
  return failures ? 1 : 0;
}

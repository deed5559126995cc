// Host-side guards of evf_store_segments_at (csrc/evf_eval_log.hip) as a stand-alone program: every EVF_EINVAL case of the
// contract in include/evflow.h must be answered before any launch and without touching the arrays beyond nseg entries.  Built
// with the host sanitizers, it needs no GPU: the one accepted call at the end reports the launch's status (an error without a
// device) and is not judged.
//
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -I event_flow_amd/csrc -I include tools/eval_log_guards.cpp event_flow_amd/csrc/evf_eval_log.hip -o eval_log_guards
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int evf_store_segments_at(const int64_t* row, int64_t nrows, float* log, int64_t row_floats, const void* const* src,
                                     const int* offset, const int* n, int nseg, void* stream);

static int failures = 0;
static void expect(const char* what, int got, int want) {
  if (got != want) {
    std::printf("FAIL %s: status %d, expected %d\n", what, got, want);
    ++failures;
  }
}

int main() {
  const int EINVAL_ = -22;
  const int64_t ROW_FLOATS = 300, NROWS = 4;
  // stand-ins for device memory: the guards compare and align pointers, they never dereference them
  alignas(16) static float arena[64];
  alignas(8) static int64_t row_word[1] = {0};
  static float log_[4 * 300];
  // exactly nseg entries: a guard that reads entry nseg or beyond runs off these heap arrays, which the sanitizer reports
  for (int nseg : {1, 2, 32}) {
    std::vector<const void*> src(nseg, arena + 1);
    std::vector<int> off(nseg, 0), n(nseg, 1);
    for (int k = 0; k < nseg; ++k) off[k] = k;
    auto call = [&](const char* what, int want) {
      expect(what, evf_store_segments_at(row_word, NROWS, log_, ROW_FLOATS, src.data(), off.data(), n.data(), nseg, nullptr), want);
    };
    const int last = nseg - 1;
    src[last] = nullptr;
    call("a null source", EINVAL_);
    n[last] = 0;
    call("a null source of no floats", EINVAL_);
    n[last] = 1;
    src[last] = (const char*)arena + 6;
    call("a source that is not 4-byte aligned", EINVAL_);
    src[last] = arena + 1;
    n[last] = -1;
    call("a negative n", EINVAL_);
    n[last] = 1;
    off[last] = -1;
    call("a negative offset", EINVAL_);
    off[last] = (int)ROW_FLOATS;
    call("offset + n one float behind the row", EINVAL_);
    off[last] = 2147483647;
    n[last] = 2147483647;
    call("offset + n beyond int32", EINVAL_);
    off[last] = last;
    n[last] = 1;
  }
  {
    const void* src[1] = {arena};
    const int off[1] = {0}, n[1] = {1};
    expect("null row", evf_store_segments_at(nullptr, NROWS, log_, ROW_FLOATS, src, off, n, 1, nullptr), EINVAL_);
    expect("null log", evf_store_segments_at(row_word, NROWS, nullptr, ROW_FLOATS, src, off, n, 1, nullptr), EINVAL_);
    expect("null src", evf_store_segments_at(row_word, NROWS, log_, ROW_FLOATS, nullptr, off, n, 1, nullptr), EINVAL_);
    expect("null offset", evf_store_segments_at(row_word, NROWS, log_, ROW_FLOATS, src, nullptr, n, 1, nullptr), EINVAL_);
    expect("null n", evf_store_segments_at(row_word, NROWS, log_, ROW_FLOATS, src, off, nullptr, 1, nullptr), EINVAL_);
    for (int nseg : {0, -1, 33, -2147483647 - 1, 2147483647})
      expect("nseg outside 1..32", evf_store_segments_at(row_word, NROWS, log_, ROW_FLOATS, src, off, n, nseg, nullptr), EINVAL_);
    expect("a row of no floats", evf_store_segments_at(row_word, NROWS, log_, 0, src, off, n, 1, nullptr), EINVAL_);
    expect("a negative row length", evf_store_segments_at(row_word, NROWS, log_, -5, src, off, n, 1, nullptr), EINVAL_);
    const int rc = evf_store_segments_at(row_word, NROWS, log_, ROW_FLOATS, src, off, n, 1, nullptr);
    std::printf("accepted arguments: status %d (0 with a device; the launch's error without one)\n", rc);
    if (rc == EINVAL_) ++failures;
  }
  std::printf(failures ? "%d guard(s) failed\n" : "all guards answered EVF_EINVAL before any launch\n", failures);
  return failures ? 1 : 0;
}

// Host-side guards of the training log's entry points (csrc/evf_train_log.hip) as a stand-alone program: every EVF_EINVAL case of
// the contracts in include/evflow.h must be answered before any launch.  Built with the host sanitizers, it needs no GPU: the
// accepted calls at the end report the launch's status (an error without a device) and are not judged.
//
//   hipcc --offload-arch=gfx950 -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -I event_flow_amd/csrc -I include tools/train_log_guards.cpp event_flow_amd/csrc/evf_train_log.hip -o train_log_guards
#include <cstdint>
#include <cstdio>

extern "C" int evf_grad_stats_chunk(void);
extern "C" int64_t evf_grad_stats_ws(int nseg, int64_t max_n);
extern "C" int evf_grad_stats_partial(const float* grad, const int64_t* seg_off, const int64_t* seg_n, int nseg, int64_t max_n,
                                      float* ws, int64_t ws_floats, void* stream);
extern "C" int evf_grad_stats_store(const float* ws, int64_t ws_floats, const int64_t* seg_n, int nseg, int64_t max_n,
                                    const float* norm_ws, float max_norm, const float* loss, const int64_t* row, int64_t nrows,
                                    float* log, int64_t row_floats, int offset, void* stream);
extern "C" int evf_spike_count_parts(void);
extern "C" int evf_spike_count(const void* const* src, int nsrc, int64_t n_words, void* ws, int slot0, int ws_slots, void* stream);
extern "C" int evf_spike_rates_store(const void* ws, int ws_slots, const int* slot_layer, int nslots, int nlayers,
                                     int64_t total_bits_per_layer, const int64_t* row, int64_t nrows, float* log, int64_t row_floats,
                                     int offset, void* stream);

static int failures = 0;
static void expect(const char* what, long long got, long long want) {
  if (got != want) {
    std::printf("FAIL %s: status %lld, expected %lld\n", what, got, want);
    ++failures;
  }
}

// stand-ins for device memory: the guards compare and align pointers, they never dereference them
struct Partial {
  const float* grad;
  const int64_t *seg_off, *seg_n;
  int nseg;
  int64_t max_n;
  float* ws;
  int64_t ws_floats;
  int call() const { return evf_grad_stats_partial(grad, seg_off, seg_n, nseg, max_n, ws, ws_floats, nullptr); }
};
struct Store {
  const float* ws;
  int64_t ws_floats;
  const int64_t* seg_n;
  int nseg;
  int64_t max_n;
  const float *norm_ws, *loss;
  const int64_t* row;
  int64_t nrows;
  float* log;
  int64_t row_floats;
  int offset;
  int call() const {
    return evf_grad_stats_store(ws, ws_floats, seg_n, nseg, max_n, norm_ws, 100.0f, loss, row, nrows, log, row_floats, offset, nullptr);
  }
};
struct Count {
  const void* src[32];
  const void* const* srcs;
  int nsrc;
  int64_t n_words;
  void* ws;
  int slot0, ws_slots;
  int call() const { return evf_spike_count(srcs ? src : nullptr, nsrc, n_words, ws, slot0, ws_slots, nullptr); }
};
struct Rates {
  const void* ws;
  int ws_slots;
  int layer[256];
  const int* layers;
  int nslots, nlayers;
  int64_t total;
  const int64_t* row;
  int64_t nrows;
  float* log;
  int64_t row_floats;
  int offset;
  int call() const {
    return evf_spike_rates_store(ws, ws_slots, layers ? layer : nullptr, nslots, nlayers, total, row, nrows, log, row_floats, offset,
                                 nullptr);
  }
};

int main() {
  const int EINVAL_ = -22;
  alignas(16) static float grad[64];
  alignas(16) static int64_t segs[16];
  alignas(16) static int64_t row_word[2] = {0, 0};
  alignas(16) static float log_[4 * 32];
  alignas(16) static float ws_[256];
  alignas(16) static float norm[8];
  alignas(16) static int words[64];
  const int chunk = evf_grad_stats_chunk();
  expect("the chunk", chunk, 4096);
  expect("ws of 3 segments up to 2 chunks + 5", evf_grad_stats_ws(3, 2 * chunk + 5), 3 * 3 * 5);
  expect("ws of one element", evf_grad_stats_ws(1, 1), 5);
  expect("ws of no segments", evf_grad_stats_ws(0, 10), EINVAL_);
  expect("ws of a negative segment count", evf_grad_stats_ws(-2147483647 - 1, 10), EINVAL_);
  expect("ws of empty segments", evf_grad_stats_ws(3, 0), EINVAL_);
  expect("ws of a negative length", evf_grad_stats_ws(3, INT64_MIN), EINVAL_);
  expect("ws of more chunks than the grid", evf_grad_stats_ws(3, (int64_t)65535 * chunk + 1), EINVAL_);
  expect("ws of 2^63 - 1 elements", evf_grad_stats_ws(3, INT64_MAX), EINVAL_);
  expect("ws of more segments than the grid", evf_grad_stats_ws(65536, 10), EINVAL_);
  expect("the parts of a spike count", evf_spike_count_parts(), 32);

#define BAD(what, stmt) \
  a = ok;               \
  stmt;                 \
  expect(what, a.call(), EINVAL_)
  {
    // three segments of at most 2 chunks + 5 elements: 3 x 3 chunks x 5 words
    const Partial ok = {grad, segs, segs + 4, 3, 2 * chunk + 5, ws_, 45};
    Partial a;
    BAD("partial: null grad", a.grad = nullptr);
    BAD("partial: null seg_off", a.seg_off = nullptr);
    BAD("partial: null seg_n", a.seg_n = nullptr);
    BAD("partial: null ws", a.ws = nullptr);
    for (int v : {0, -1, -2147483647 - 1}) {
      BAD("partial: a non-positive nseg", a.nseg = v);
      BAD("partial: a non-positive max_n", a.max_n = v);
    }
    BAD("partial: max_n = -2^63", a.max_n = INT64_MIN);
    BAD("partial: more chunks than the grid", a.max_n = INT64_MAX; a.ws_floats = INT64_MAX);
    BAD("partial: more segments than the grid", a.nseg = 65536; a.ws_floats = INT64_MAX);
    BAD("partial: a workspace one float short", a.ws_floats = 44);
    BAD("partial: a workspace of no floats", a.ws_floats = 0);
    BAD("partial: a negative workspace size", a.ws_floats = -45);
    BAD("partial: a grad that is not 4-byte aligned", a.grad = (const float*)((const char*)grad + 2));
    BAD("partial: a ws that is not 4-byte aligned", a.ws = (float*)((char*)ws_ + 1));
    BAD("partial: a seg_off that is not 8-byte aligned", a.seg_off = (const int64_t*)((const char*)segs + 4));
    BAD("partial: a seg_n that is not 8-byte aligned", a.seg_n = (const int64_t*)((const char*)segs + 36));
    a = ok;
    const int rc = a.call();
    std::printf("partial, accepted arguments: status %d (0 with a device; the launch's error without one)\n", rc);
    if (rc == EINVAL_) ++failures;
  }
  {
    // the same three segments, a row of 3 + 9 floats behind offset 5 in rows of 32
    const Store ok = {ws_, 45, segs + 4, 3, 2 * chunk + 5, norm, norm + 1, row_word, 4, log_, 32, 5};
    Store a;
    BAD("store: null ws", a.ws = nullptr);
    BAD("store: null seg_n", a.seg_n = nullptr);
    BAD("store: null norm_ws", a.norm_ws = nullptr);
    BAD("store: null row", a.row = nullptr);
    BAD("store: null log", a.log = nullptr);
    for (int v : {0, -1, -2147483647 - 1}) {
      BAD("store: a non-positive nseg", a.nseg = v);
      BAD("store: a non-positive max_n", a.max_n = v);
      BAD("store: a non-positive nrows", a.nrows = v);
      BAD("store: a non-positive row length", a.row_floats = v);
    }
    BAD("store: a negative offset", a.offset = -1);
    BAD("store: offset + 3 + 3 nseg one float behind the row", a.offset = 21);
    BAD("store: offset = 2^31 - 1", a.offset = 2147483647);
    BAD("store: a row shorter than 3 + 3 nseg", a.row_floats = 11; a.offset = 0);
    BAD("store: a workspace one float short", a.ws_floats = 44);
    BAD("store: a negative workspace size", a.ws_floats = -45);
    BAD("store: more segments than the grid", a.nseg = 65536; a.ws_floats = INT64_MAX; a.row_floats = INT64_MAX);
    BAD("store: a ws that is not 4-byte aligned", a.ws = (const float*)((const char*)ws_ + 2));
    BAD("store: a log that is not 4-byte aligned", a.log = (float*)((char*)log_ + 2));
    BAD("store: a norm_ws that is not 4-byte aligned", a.norm_ws = (const float*)((const char*)norm + 3));
    BAD("store: a loss that is not 4-byte aligned", a.loss = (const float*)((const char*)norm + 1));
    BAD("store: a seg_n that is not 8-byte aligned", a.seg_n = (const int64_t*)((const char*)segs + 4));
    BAD("store: a row word that is not 8-byte aligned", a.row = (const int64_t*)((const char*)row_word + 4));
    a = ok;
    a.offset = 20;      // the last offset that fits
    a.loss = nullptr;   // allowed: the field is left as it is
    const int rc = a.call();
    std::printf("store, accepted arguments: status %d (0 with a device; the launch's error without one)\n", rc);
    if (rc == EINVAL_) ++failures;
  }
  {
    // five sources of 63 words into slots 2 .. 6 of 8
    Count ok = {{}, nullptr, 5, 63, ws_, 2, 8};
    for (int k = 0; k < 5; ++k) ok.src[k] = words;
    ok.srcs = ok.src;
    Count a;
    BAD("count: null src", a.srcs = nullptr);
    BAD("count: null ws", a.ws = nullptr);
    for (int v : {0, -1, 33, -2147483647 - 1, 2147483647}) { BAD("count: nsrc outside 1..32", a.nsrc = v; a.ws_slots = 2147483647); }
    for (long long v : {0LL, -1LL, 2147483648LL, (long long)INT64_MIN}) { BAD("count: n_words outside 1 .. 2^31 - 1", a.n_words = v); }
    BAD("count: a negative first slot", a.slot0 = -1);
    BAD("count: slots one behind the workspace", a.slot0 = 4);
    BAD("count: slot0 = 2^31 - 1", a.slot0 = 2147483647);
    BAD("count: a workspace of no slots", a.ws_slots = 0; a.slot0 = 0);
    BAD("count: a negative workspace size", a.ws_slots = -8);
    BAD("count: a ws that is not 4-byte aligned", a.ws = (char*)ws_ + 2);
    BAD("count: a null source", a.src[3] = nullptr);
    BAD("count: a source that is not 4-byte aligned", a.src[4] = (const char*)words + 2);
    a = ok;
    a.src[1] = words + 1;  // 4-byte aligned is enough
    a.slot0 = 3;           // the last slot that fits
    const int rc = a.call();
    std::printf("count, accepted arguments: status %d (0 with a device; the launch's error without one)\n", rc);
    if (rc == EINVAL_) ++failures;
  }
  {
    // 21 slots of 7 layers, a payload of 7 floats behind offset 17 in rows of 32
    Rates ok = {ws_, 21, {}, nullptr, 21, 7, 3 * 65536, row_word, 4, log_, 32, 17};
    for (int s = 0; s < 21; ++s) ok.layer[s] = s % 7;
    ok.layers = ok.layer;
    Rates a;
    BAD("rates: null ws", a.ws = nullptr);
    BAD("rates: null slot_layer", a.layers = nullptr);
    BAD("rates: null row", a.row = nullptr);
    BAD("rates: null log", a.log = nullptr);
    for (int v : {0, -1, 257, -2147483647 - 1, 2147483647}) {
      BAD("rates: nslots outside 1..256", a.nslots = v; a.ws_slots = 2147483647);
      BAD("rates: nlayers outside 1..256", a.nlayers = v; a.row_floats = INT64_MAX);
    }
    for (int v : {0, -1, -2147483647 - 1}) {
      BAD("rates: a non-positive total", a.total = v);
      BAD("rates: a non-positive nrows", a.nrows = v);
      BAD("rates: a non-positive row length", a.row_floats = v);
    }
    BAD("rates: a workspace one slot short", a.ws_slots = 20);
    BAD("rates: a negative workspace size", a.ws_slots = -21);
    BAD("rates: a layer behind the last", a.layer[20] = 7);
    BAD("rates: a negative layer", a.layer[0] = -1);
    BAD("rates: a negative offset", a.offset = -1);
    BAD("rates: offset + nlayers one float behind the row", a.offset = 26);
    BAD("rates: offset = 2^31 - 1", a.offset = 2147483647);
    BAD("rates: a ws that is not 4-byte aligned", a.ws = (const char*)ws_ + 2);
    BAD("rates: a log that is not 4-byte aligned", a.log = (float*)((char*)log_ + 2));
    BAD("rates: a row word that is not 8-byte aligned", a.row = (const int64_t*)((const char*)row_word + 4));
    a = ok;
    a.offset = 25;  // the last offset that fits
    const int rc = a.call();
    std::printf("rates, accepted arguments: status %d (0 with a device; the launch's error without one)\n", rc);
    if (rc == EINVAL_) ++failures;
  }
#undef BAD
  std::printf(failures ? "%d guard(s) failed\n" : "all guards answered EVF_EINVAL before any launch\n", failures);
  return failures ? 1 : 0;
}

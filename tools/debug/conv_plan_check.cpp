// Host check that the three plan functions of the 3x3 stride-1 convolution family (evf_conv3_b3t_plan, _b3i_plan, _b3n_plan) return the
// same number of K splits with the shared b3_plan_splits (evf_conv_b3_family.h) as with the arithmetic each of them carried before.
// The plans are copied here as plain functions (environment switches on, operands aligned): no GPU, no HIP runtime.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/debug/conv_plan_check.cpp -o /tmp/conv_plan_check && /tmp/conv_plan_check
#include <algorithm>
#include <cstdio>
using std::max;
using std::min;

static inline int evf_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- before: each plan with its own copy of the split arithmetic
static int t_plan_old(int B, int H, int W, int K, int N, int lds, bool force, int max_split, int force_split) {
  if (K % 4 != 0 || lds % 4 != 0) return 0;
  const long tiles = (long)B * evf_cdiv(H, 16) * evf_cdiv(W, 32);
  const long blocks = tiles * evf_cdiv(N, N > 32 ? 64 : 32);
  const int KC = evf_cdiv(K, 16);
  const int smax = max(1, min(max_split, KC / 4));
  int ks = blocks >= 256 ? 1 : (int)min((long)smax, (long)evf_cdiv(512L, blocks));
  if (force_split > 0) ks = max(1, min(min(force_split, max(max_split, 1)), KC));
  if (force) return ks;
  const double fill = (double)H * W / ((double)evf_cdiv(H, 16) * 16 * evf_cdiv(W, 32) * 32);
  return (blocks * ks >= 192 && fill >= 0.7) ? ks : 0;
}
static int i_plan_old(int B, int H, int W, int K, int N, int lds, bool force, int max_split, int force_split) {
  if (H > 16 || W > 16 || H < 1 || W < 1) return 0;
  if (K % 4 != 0 || lds % 4 != 0) return 0;
  if (!force && (K < 64 || N < 32 || H < 4 || W < 4)) return 0;
  const int KC = evf_cdiv(K, 16);
  const long blocks = (long)B * evf_cdiv(N, 64);
  const int smax = max(1, min(max_split, KC / 4));
  int ks = blocks >= 256 ? 1 : (int)min((long)smax, (long)evf_cdiv(256L, blocks));
  if (force_split > 0) ks = max(1, min(min(force_split, max(max_split, 1)), KC));
  if (force) return ks;
  return (blocks * ks >= 96) ? ks : 0;
}
static int n_plan_old(int B, int H, int W, int K, int N, int lds, bool force, int max_split, int force_split) {
  if (K % 4 != 0 || lds % 4 != 0) return 0;
  const int ntiles = evf_cdiv(N, 32);
  if (!force && (ntiles < 3 || K < 16 || K > 64)) return 0;
  const long tiles = (long)B * evf_cdiv(H, 8) * evf_cdiv(W, 32);
  const int nchunk = evf_cdiv(ntiles, 6);
  const long blocks = tiles * nchunk;
  const int KC = evf_cdiv(K, 16);
  const int smax = max(1, min(max_split, KC / 4));
  int ks = blocks >= 192 ? 1 : (int)min((long)smax, (long)evf_cdiv(256L, blocks));
  if (force_split > 0) ks = max(1, min(min(force_split, max(max_split, 1)), KC));
  if (force) return ks;
  const double fill = (double)H * W / ((double)evf_cdiv(H, 8) * 8 * evf_cdiv(W, 32) * 32);
  return (blocks * ks >= 160 && fill >= 0.7) ? ks : 0;
}

// ---- after: the shared helper, each plan passing its constants
static inline int b3_plan_splits(long blocks, int KC, int max_split, int force_split, long unsplit_at, long target) {
  const int smax = max(1, min(max_split, KC / 4));
  int ks = blocks >= unsplit_at ? 1 : (int)min((long)smax, (long)evf_cdiv(target, blocks));
  if (force_split > 0) ks = max(1, min(min(force_split, max(max_split, 1)), KC));
  return ks;
}
static int t_plan_new(int B, int H, int W, int K, int N, int lds, bool force, int max_split, int force_split) {
  if (K % 4 != 0 || lds % 4 != 0) return 0;
  const long tiles = (long)B * evf_cdiv(H, 16) * evf_cdiv(W, 32);
  const long blocks = tiles * evf_cdiv(N, N > 32 ? 64 : 32);
  const int KC = evf_cdiv(K, 16);
  const int ks = b3_plan_splits(blocks, KC, max_split, force_split, 256, 512);
  if (force) return ks;
  const double fill = (double)H * W / ((double)evf_cdiv(H, 16) * 16 * evf_cdiv(W, 32) * 32);
  return (blocks * ks >= 192 && fill >= 0.7) ? ks : 0;
}
static int i_plan_new(int B, int H, int W, int K, int N, int lds, bool force, int max_split, int force_split) {
  if (H > 16 || W > 16 || H < 1 || W < 1) return 0;
  if (K % 4 != 0 || lds % 4 != 0) return 0;
  if (!force && (K < 64 || N < 32 || H < 4 || W < 4)) return 0;
  const int KC = evf_cdiv(K, 16);
  const long blocks = (long)B * evf_cdiv(N, 64);
  const int ks = b3_plan_splits(blocks, KC, max_split, force_split, 256, 256);
  if (force) return ks;
  return (blocks * ks >= 96) ? ks : 0;
}
static int n_plan_new(int B, int H, int W, int K, int N, int lds, bool force, int max_split, int force_split) {
  if (K % 4 != 0 || lds % 4 != 0) return 0;
  const int ntiles = evf_cdiv(N, 32);
  if (!force && (ntiles < 3 || K < 16 || K > 64)) return 0;
  const long tiles = (long)B * evf_cdiv(H, 8) * evf_cdiv(W, 32);
  const int nchunk = evf_cdiv(ntiles, 6);
  const long blocks = tiles * nchunk;
  const int KC = evf_cdiv(K, 16);
  const int ks = b3_plan_splits(blocks, KC, max_split, force_split, 192, 256);
  if (force) return ks;
  const double fill = (double)H * W / ((double)evf_cdiv(H, 8) * 8 * evf_cdiv(W, 32) * 32);
  return (blocks * ks >= 160 && fill >= 0.7) ? ks : 0;
}

int main() {
  const int Bs[] = {1, 2, 8, 16}, HWs[] = {4, 9, 16, 17, 33, 64, 256}, KNs[] = {4, 16, 20, 32, 64, 132, 260, 512, 1028};
  const int MSs[] = {0, 1, 8}, FSs[] = {0, 3}, Fs[] = {0, 1};
  typedef int (*plan_t)(int, int, int, int, int, int, bool, int, int);
  const plan_t olds[3] = {t_plan_old, i_plan_old, n_plan_old}, news[3] = {t_plan_new, i_plan_new, n_plan_new};
  const char* names[3] = {"b3t", "b3i", "b3n"};
  long cases = 0, bad = 0, taken[3] = {0, 0, 0}, split[3] = {0, 0, 0};
  for (int B : Bs)
    for (int H : HWs)
      for (int W : HWs)
        for (int K : KNs)
          for (int N : KNs)
            for (int ms : MSs)
              for (int fs : FSs)
                for (int f : Fs)
                  for (int p = 0; p < 3; ++p) {
                    const int a = olds[p](B, H, W, K, N, K, f != 0, ms, fs), b = news[p](B, H, W, K, N, K, f != 0, ms, fs);
                    ++cases, taken[p] += a > 0, split[p] += a > 1;
                    if (a != b && ++bad <= 10)
                      printf("DIFF %s B=%d H=%d W=%d K=%d N=%d max_split=%d force_split=%d force=%d: %d -> %d\n", names[p], B, H, W, K, N,
                             ms, fs, f, a, b);
                  }
  printf("%ld plan calls, %ld differ; taken / split: b3t %ld / %ld, b3i %ld / %ld, b3n %ld / %ld\n", cases, bad, taken[0], split[0],
         taken[1], split[1], taken[2], split[2]);
  return bad ? 1 : 0;
}

// Stand-alone host check of csrc/wx_dft.h, meant for AddressSanitizer / UBSan.  DftPhase -- the struct the kernels themselves walk the
// twiddle table with -- is driven for every lane (c, g) and every column of every block with the kernels' three parameter sets: the
// forward passes' (4 g, 12), the inverse passes' (2 g, 8) with a look-ahead of one, and the latitude pass' (4 g, 12) with k = l.  At
// every step the index must lie inside the table, equal (k x) mod N computed in 64 bits, and the look-ahead must equal the next step.
// The fold is checked in numbers: the folded sums over dft_table give the plain DFT and every element enters the fold once.  It calls
// no HIP function, so it runs on a machine without a GPU:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/dft_host_check.hip -o dft_host_check && ./dft_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../miles-credit_amd/csrc/wx_dft.h"

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

// One lane's walk of column k: in each chunk of 4 per values of x the lane starts at chunk + per g, takes `steps` steps and skips
// the rest of the chunk, until x passes n_x.  Forward passes: per 4, four steps, skip 12.  Inverse passes: per 2, no step (the second
// bin is the look-ahead), skip 8.
static void walk(int N, int k, int g, int per, int steps, int n_x) {
  wx::DftPhase ph;
  ph.init(k, per * g, 4 * per - steps, N);
  EXPECT(ph.k == k % N);
  const auto check = [&](int64_t x) {
    EXPECT(ph.idx >= 0 && ph.idx < N && ph.idx == (int)(((int64_t)k * x) % N));
    EXPECT(ph.ahead(N) >= 0 && ph.ahead(N) < N && ph.ahead(N) == (int)(((int64_t)k * (x + 1)) % N));
  };
  for (int x0 = 0; x0 < n_x; x0 += 4 * per) {
    check(x0 + per * g);
    for (int j = 1; j <= steps; ++j) {
      ph.step(N);
      check(x0 + per * g + j);
    }
    ph.skip(N);
  }
}

// every lane of every block of `cols` output columns in tiles of `tile` (columns block * tile + 16 t + c, the tail block whole)
static void walk_all(int N, int cols, int tile, int per, int steps, int n_x) {
  for (int n0 = 0; n0 < cols; n0 += tile)
    for (int t = 0; t < tile / 16; ++t)
      for (int c = 0; c < 16; ++c)
        for (int g = 0; g < 4; ++g) walk(N, n0 + 16 * t + c, g, per, steps, n_x);
}

// the folded sums over the table against the plain DFT, rows of W on H rows
static void fold_numeric(int H, int W) {
  const int Wh = W / 2 + 1;
  std::vector<double2> tab;
  wx::dft_table(W, tab);
  std::vector<float> src((size_t)H * W);
  for (size_t i = 0; i < src.size(); ++i) src[i] = 250.f + (float)((i * 2654435761u) % 1000u) * 0.01f;
  const double two_pi = 2.0 * 3.14159265358979323846;
  for (int h = 0; h < H; ++h) {
    const float* r = src.data() + (int64_t)h * W;
    double esum = 0.0, rsum = 0.0;
    for (int x = 0; x < Wh; ++x) {
      double e, o;
      wx::dft_fold(r, W, x, e, o);
      esum += e;
    }
    for (int x = 0; x < W; ++x) rsum += (double)r[x];
    EXPECT(std::fabs(esum - rsum) <= 1e-9 * std::fabs(rsum));      // every element enters the fold once
    for (int k = 0; k < Wh; ++k) {
      double re = 0.0, im = 0.0, re0 = 0.0, im0 = 0.0;
      for (int x = 0; x < Wh; ++x) {
        double e, o;
        wx::dft_fold(r, W, x, e, o);
        const double2 cs = tab.at((size_t)(((int64_t)k * x) % W));
        re += e * cs.x;
        im += o * cs.y;
      }
      for (int x = 0; x < W; ++x) {
        const double a = two_pi * (double)(((int64_t)k * x) % W) / (double)W;
        re0 += (double)r[x] * std::cos(a);
        im0 += (double)r[x] * std::sin(a);
      }
      const double scale = 250.0 * W;
      EXPECT(std::fabs(re - re0) <= 1e-12 * scale && std::fabs(im - im0) <= 1e-12 * scale);
    }
  }
}

int main() {
  using namespace wx;
  // the table and its limit
  std::vector<double2> t;
  dft_table(1440, t);
  EXPECT(t.size() == 1440 && t[0].x == 1.0 && t[0].y == 0.0 && t[720].x == -1.0 && std::fabs(t[360].y - 1.0) < 1e-15);
  EXPECT(dft_lds_bytes(kDftMaxN) == 65536 && dft_lds_bytes(2) == 32 && kDftTileRows == 4 * kDftWaveRows && kDftTileCols == 32);
  EXPECT(dft_wrap(5, 7) == 5 && dft_wrap(7, 7) == 0 && dft_wrap(13, 7) == 6);
  // the fold: x = 0 and the midpoint of an even W enter unfolded, with zero in the sin sum
  const float r[6] = {1.f, 2.f, 3.f, 4.f, 5.f, 6.f};
  const double rd[5] = {1.0, 2.0, 3.0, 4.0, 5.0};
  double e, o;
  dft_fold(r, 6, 0, e, o); EXPECT(e == 1.0 && o == 0.0);
  dft_fold(r, 6, 1, e, o); EXPECT(e == 8.0 && o == -4.0);
  dft_fold(r, 6, 3, e, o); EXPECT(e == 4.0 && o == 0.0);
  dft_fold(r, 5, 2, e, o); EXPECT(e == 7.0 && o == -1.0);
  dft_fold(rd, 5, 2, e, o); EXPECT(e == 7.0 && o == -1.0);
  EXPECT(!dft_has_mirror(6, 0) && !dft_has_mirror(6, 3) && dft_has_mirror(6, 2) && dft_has_mirror(5, 2));
  // the phase walk
  const int sizes[] = {2, 5, 9, 12, 15, 16, 37, 45, 64, 72, 75, 90, 144, 360, 1440, 4096};
  for (const int N : sizes) {
    const int Wh = N / 2 + 1;
    walk_all(N, Wh, kDftTileCols, 4, 4, Wh);             // folded forward: Wh wavenumbers, x < Wh
    walk_all(N, Wh, 32, 4, 4, N);                        // unfolded forward (pass A): wavenumber n >> 1 of 64 columns n, x < N
    walk_all(N, N, 64, 4, 4, N);                         // the latitude pass: k = l, rows of 64, h < N
    walk_all(N, N, 64, 2, 0, Wh);                        // inverse: N columns x, the lane's bins chunk + 2 g and + 1, m < Wh
  }
  for (const int W : {2, 5, 12, 15, 45, 64, 75, 90, 144}) fold_numeric(3, W);
  std::printf("dft_host_check: ok\n");
  return 0;
}

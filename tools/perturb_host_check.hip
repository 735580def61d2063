// Stand-alone host check of the host-only helpers of csrc/wx_perturb.h -- perturb_check_create and perturb_check_apply (what the
// C ABI refuses) and perturb_batch_planes -- meant for AddressSanitizer / UBSan.  The index arithmetic of the three DFT kernels is
// replayed on the host for every lane of every workgroup over exactly-sized heap arrays, the table index taken from the kernels' own
// DftPhase (checked by itself in tools/dft_host_check.hip): every guarded load and store must stay inside its buffer and every output
// is written exactly once, so an index past an array is caught here and not on a GPU.  It calls no HIP function, so it runs on a
// machine without a GPU:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/perturb_host_check.hip -o perturb_host_check && ./perturb_host_check
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../miles-credit_amd/csrc/wx_perturb.h"

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

// passes A and C: M rows, the table of W entries; touches src / in and out as the kernels do
static void replay_rows(int nb, int H, int W) {
  const int Wh = W / 2 + 1, N = 2 * Wh, M = nb * H;
  std::vector<double2> tab;
  wx::dft_table(W, tab);
  std::vector<float> src((size_t)M * W, 1.f);
  std::vector<double> spec((size_t)M * N, 0.0);
  std::vector<char> seen_a((size_t)M * N, 0), seen_c((size_t)M * W, 0);
  for (int by = 0; by < wx::cdiv(M, 64); ++by)
    for (int wave = 0; wave < 4; ++wave) {
      const int m0 = (by * 4 + wave) * 16;
      if (m0 >= M) continue;
      for (int lane = 0; lane < 64; ++lane) {
        const int c = lane & 15, g = lane >> 4, row = m0 + c;
        for (int bx = 0; bx < wx::cdiv(N, 64); ++bx)          // pass A
          for (int t = 0; t < 4; ++t) {
            const int n = bx * 64 + 16 * t + c;
            wx::DftPhase ph;
            ph.init(n >> 1, 4 * g, 12, W);
            for (int kc = 0; kc < W; kc += 16) {
              for (int j = 0; j < 4; ++j) {
                const int x = kc + 4 * g + j;
                (void)tab.at(ph.idx);
                if (row < M && x < W) (void)src.at((size_t)row * W + x);
                ph.step(W);
              }
              ph.skip(W);
            }
            for (int r = 0; r < 4; ++r) {
              const int m = m0 + g + 4 * r;
              if (m < M && n < N) { EXPECT(!seen_a.at((size_t)m * N + n)); seen_a[(size_t)m * N + n] = 1; spec.at((size_t)m * N + n) = 1.0; }
            }
          }
        for (int bx = 0; bx < wx::cdiv(W, 64); ++bx)          // pass C
          for (int t = 0; t < 4; ++t) {
            const int xo = bx * 64 + 16 * t + c;
            wx::DftPhase ph;
            ph.init(xo, 2 * g, 8, W);
            for (int k0 = 0; k0 < Wh; k0 += 8) {
              for (int b = 0; b < 2; ++b) {
                const int k = k0 + 2 * g + b;
                (void)tab.at(b ? ph.ahead(W) : ph.idx);
                if (row < M && k < Wh) { (void)spec.at((size_t)row * N + 2 * k); (void)spec.at((size_t)row * N + 2 * k + 1); }
              }
              ph.skip(W);
            }
            for (int r = 0; r < 4; ++r) {
              const int m = m0 + g + 4 * r;
              if (m < M && xo < W) { EXPECT(m / H < nb && !seen_c.at((size_t)m * W + xo)); seen_c[(size_t)m * W + xo] = 1; }
            }
          }
      }
    }
  for (char s : seen_a) EXPECT(s);      // every element is written, once
  for (char s : seen_c) EXPECT(s);
}

// pass B for one plane
static void replay_cols(int H, int W) {
  const int N = 2 * (W / 2 + 1);
  std::vector<double2> tab;
  wx::dft_table(H, tab);
  std::vector<double> X((size_t)H * N, 1.0);
  std::vector<float> S((size_t)H * (N / 2), 1.f);
  std::vector<char> seen((size_t)H * N, 0);
  for (int by = 0; by < wx::cdiv(H, 64); ++by)
    for (int wave = 0; wave < 4; ++wave) {
      const int m0 = (by * 4 + wave) * 16;
      if (m0 >= H) continue;
      for (int bx = 0; bx < wx::cdiv(N, 64); ++bx)
        for (int lane = 0; lane < 64; ++lane) {
          const int c = lane & 15, g = lane >> 4;
          wx::DftPhase ph;
          ph.init(m0 + c, 4 * g, 12, H);
          for (int kc = 0; kc < H; kc += 16) {
            for (int j = 0; j < 4; ++j) {
              const int h = kc + 4 * g + j;
              (void)tab.at(ph.idx);
              ph.step(H);
              for (int t = 0; t < 4; ++t) {
                const int n = bx * 64 + 16 * t + c;
                if (h < H && n < N) { (void)X.at((size_t)h * N + n); (void)X.at((size_t)h * N + (n ^ 1)); }
              }
            }
            ph.skip(H);
          }
          for (int t = 0; t < 4; ++t)
            for (int r = 0; r < 4; ++r) {
              const int m = m0 + g + 4 * r, n = bx * 64 + 16 * t + c;
              if (m < H && n < N) { (void)S.at((size_t)m * (N >> 1) + (n >> 1)); EXPECT(!seen.at((size_t)m * N + n)); seen[(size_t)m * N + n] = 1; }
            }
        }
    }
  for (char s : seen) EXPECT(s);
}

int main() {
  using namespace wx;
  // create
  std::vector<float> S(5 * 5, 1.f);
  EXPECT(perturb_check_create(5, 8, kPerturbColour, S.data()).empty() && perturb_check_create(5, 8, kPerturbWhite, nullptr).empty());
  EXPECT(has(perturb_check_create(0, 8, 1, S.data()), "H must be >= 1") && has(perturb_check_create(5, 1, 0, nullptr), "W >= 2"));
  EXPECT(has(perturb_check_create(5, 8, 2, S.data()), "kind must be") && has(perturb_check_create(5, 8, 1, nullptr), "null pointer"));
  EXPECT(has(perturb_check_create(1 << 18, 1 << 17, 0, nullptr), "counter") && has(perturb_check_create(5, 5000, 1, S.data()), "4096 points"));
  EXPECT(has(perturb_check_create(std::numeric_limits<int>::max(), std::numeric_limits<int>::max(), 0, nullptr), "counter"));
  S[17] = std::numeric_limits<float>::quiet_NaN();
  EXPECT(has(perturb_check_create(5, 8, 1, S.data()), "entry 17"));
  // apply: pointers are compared, never read
  std::vector<float> a(4 * 40), b(4 * 40);
  const int64_t hw = 40;
  EXPECT(perturb_check_apply(5, 8, 3, a.data(), nullptr, hw, b.data(), hw, nullptr, hw, b.data(), hw).empty());          // in place, from a tape
  EXPECT(has(perturb_check_apply(5, 8, 0, nullptr, nullptr, hw, nullptr, hw, b.data(), hw, nullptr, hw), "n_planes"));
  EXPECT(has(perturb_check_apply(5, 8, std::numeric_limits<int>::max(), nullptr, nullptr, hw, nullptr, hw, b.data(), hw, nullptr, hw), "counter"));
  EXPECT(has(perturb_check_apply(5, 8, 3, nullptr, nullptr, hw, nullptr, hw, nullptr, hw, nullptr, hw), "no output"));
  EXPECT(has(perturb_check_apply(5, 8, 3, nullptr, nullptr, hw, nullptr, hw, nullptr, hw, b.data(), hw), "x_out needs x"));
  EXPECT(has(perturb_check_apply(5, 8, 3, nullptr, nullptr, hw, nullptr, hw, b.data(), 39, nullptr, hw), "stride is smaller"));
  EXPECT(has(perturb_check_apply(5, 8, 3, nullptr, a.data(), 0, nullptr, hw, b.data(), hw, nullptr, hw), "stride is smaller"));
  EXPECT(has(perturb_check_apply(5, 8, 3, nullptr, nullptr, hw, nullptr, hw, b.data(), std::numeric_limits<int64_t>::max(), nullptr, hw), "beyond 2^44"));
  EXPECT(has(perturb_check_apply(5, 8, 3, a.data(), nullptr, hw, nullptr, hw, a.data() + 80, hw, nullptr, hw), "tape overlaps"));
  EXPECT(has(perturb_check_apply(5, 8, 2, nullptr, nullptr, hw, a.data(), hw, nullptr, hw, a.data() + 8, hw), "same view"));
  EXPECT(has(perturb_check_apply(5, 8, 2, nullptr, nullptr, hw, a.data(), hw, b.data(), hw, b.data() + 40, hw), "outputs overlap"));
  EXPECT(perturb_check_apply(5, 8, 2, nullptr, b.data(), hw, a.data(), hw, b.data(), hw, a.data(), hw).empty());          // delta_out = prev, x_out = x
  // batch
  EXPECT(perturb_batch_planes(721, 1440) == 16 && perturb_batch_planes(19, 37) == 64 && perturb_batch_planes(4096, 4096) == 1);
  EXPECT((int64_t)perturb_batch_planes(721, 1440) * perturb_plane_bytes(721, 1440) <= kPerturbScratchBytes);
  // the kernels' indexing on the cases of tests/perturb_cases.py, two planes where a row tile straddles planes
  const int grids[][3] = {{3, 5, 8}, {2, 7, 9}, {4, 19, 37}, {1, 33, 64}, {4, 37, 72}, {1, 181, 360}, {2, 1, 2}, {1, 721, 1440}};
  for (const auto& gr : grids) {
    if (gr[1] < 721) replay_rows(gr[0], gr[1], gr[2]);
    replay_cols(gr[1], gr[2]);
  }
  std::printf("perturb_host_check: ok\n");
  return 0;
}

// Stand-alone host check of the host-only helpers of csrc/wx_spectrum.h -- spectrum_check_create and spectrum_check_apply (what the
// C ABI refuses), spectrum_tiles, spectrum_slot_doubles and spectrum_lds_bytes -- meant for AddressSanitizer / UBSan.
// The index arithmetic of spectrum_rows_kernel and spectrum_finish_kernel is replayed on the host for every lane of every workgroup
// over exactly-sized heap arrays, the table index taken from the kernels' own DftPhase (checked by itself, with the fold, in
// tools/dft_host_check.hip): every guarded load and store must stay inside its buffer and every psd element and every slot must be
// written exactly once.  It calls no HIP function, so it runs on a machine without a GPU:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/spectrum_host_check.hip -o spectrum_host_check && ./spectrum_host_check
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../miles-credit_amd/csrc/wx_spectrum.h"

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

// launch 1 and launch 2 on P planes at `stride` floats
static void replay(int P, int H, int W, int64_t stride) {
  const wx::SpecTiles tl = wx::spectrum_tiles(H, W);
  const int Wh = tl.Wh;
  std::vector<double2> tab;
  wx::dft_table(W, tab);
  std::vector<float> src((size_t)((P - 1) * stride + (int64_t)H * W));
  for (size_t i = 0; i < src.size(); ++i) src[i] = 250.f + (float)((i * 2654435761u) % 1000u) * 0.01f;
  std::vector<char> seen_psd((size_t)P * H * Wh, 0), seen_slot((size_t)wx::spectrum_slot_doubles(H, W, P), 0);
  EXPECT(wx::spectrum_lds_bytes(W) >= (size_t)W * 16 && wx::spectrum_lds_bytes(W) >= wx::kSpecReduceBytes && wx::spectrum_lds_bytes(W) <= 65536);
  const int64_t blocks = (int64_t)P * tl.row_tiles * tl.col_blocks;
  for (int64_t bid = 0; bid < blocks; ++bid) {
    const int cb = (int)(bid % tl.col_blocks), tile = (int)(bid / tl.col_blocks), rt = tile % tl.row_tiles;
    const int64_t p = tile / tl.row_tiles;
    EXPECT(p < P);
    for (int wave = 0; wave < 4; ++wave) {
      const int h0 = rt * wx::kDftTileRows + wave * wx::kDftWaveRows, k0 = cb * wx::kDftTileCols;
      if (h0 >= H) continue;
      for (int lane = 0; lane < 64; ++lane) {
        const int c = lane & 15, g = lane >> 4, row = h0 + c;
        const bool row_ok = row < H;
        const float* arow = src.data() + p * stride + (int64_t)(row_ok ? row : 0) * W;
        for (int t = 0; t < 2; ++t) {
          const int kq = k0 + 16 * t + c;
          wx::DftPhase ph;
          ph.init(kq, 4 * g, 12, W);
          for (int kc = 0; kc < Wh; kc += 16) {
            for (int j = 0; j < 4; ++j) {
              const int x = kc + 4 * g + j;
              (void)tab.at(ph.idx);
              if (row_ok && x < Wh) {
                const size_t at = (size_t)(arow - src.data()) + x;
                (void)src.at(at);
                if (wx::dft_has_mirror(W, x)) { EXPECT(W - x > x); (void)src.at(at - x + (W - x)); }
              }
              ph.step(W);
            }
            ph.skip(W);
          }
          for (int r = 0; r < 4; ++r) {
            const int h = h0 + g + 4 * r;
            if (h < H && kq < Wh) {
              const size_t o = (size_t)((p * H + h) * Wh + kq);
              EXPECT(!seen_psd.at(o));
              seen_psd[o] = 1;
            }
          }
        }
      }
    }
    for (int tid = 0; tid < 2 * wx::kSpecSums * 16; ++tid) {
      const int t = tid / (wx::kSpecSums * 16), i = (tid / 16) % wx::kSpecSums, cc = tid & 15, k = cb * wx::kDftTileCols + 16 * t + cc;
      EXPECT((size_t)(((3 * 2 + t) * wx::kSpecSums + i) * 16 + cc) * sizeof(double) < wx::kSpecReduceBytes);
      if (k < Wh) {
        const size_t o = (size_t)((((p * tl.row_tiles + rt) * wx::kSpecSums) + i) * Wh + k);
        EXPECT(!seen_slot.at(o));
        seen_slot[o] = 1;
      }
    }
  }
  for (char s : seen_psd) EXPECT(s);      // every element is written, once
  for (char s : seen_slot) EXPECT(s);
  for (int64_t p = 0; p < P; ++p)         // launch 2 reads slots that launch 1 wrote
    for (int k = 0; k < Wh; ++k)
      for (int rt = 0; rt < tl.row_tiles; ++rt)
        for (int i = 0; i < wx::kSpecSums; ++i) EXPECT(seen_slot.at((size_t)(((p * tl.row_tiles + rt) * wx::kSpecSums) * Wh + k + (int64_t)i * Wh)));
}

int main() {
  using namespace wx;
  const float inf = std::numeric_limits<float>::infinity();
  // create
  std::vector<float> w(5, 1.f);
  EXPECT(spectrum_check_create(5, 12, nullptr).empty() && spectrum_check_create(5, 12, w.data()).empty() && spectrum_check_create(2, 2, nullptr).empty());
  EXPECT(has(spectrum_check_create(1, 12, nullptr), "must be >= 2") && has(spectrum_check_create(5, 1, nullptr), "must be >= 2"));
  EXPECT(has(spectrum_check_create(5, 4097, nullptr), "W must be <= 4096") && spectrum_check_create(5, 4096, nullptr).empty());
  EXPECT(has(spectrum_check_create(std::numeric_limits<int>::max(), 4096, nullptr), "2^31"));
  w[3] = inf;
  EXPECT(has(spectrum_check_create(5, 12, w.data()), "row 3"));
  w[3] = std::numeric_limits<float>::quiet_NaN();
  EXPECT(has(spectrum_check_create(5, 12, w.data()), "row 3"));
  w[3] = -0.5f;
  EXPECT(has(spectrum_check_create(5, 12, w.data()), "finite and >= 0"));
  w.assign(5, 0.f);
  EXPECT(has(spectrum_check_create(5, 12, w.data()), "sum to zero"));
  // apply: pointers are compared, never read.  5 x 12: hw = 60, Wh = 7
  std::vector<float> a(4 * 60), b(4 * 60), pa(3 * 5 * 7 + 8), pb(3 * 5 * 7);
  std::vector<double> m0(3 * 7), m1(3 * 7), m2(3 * 7), m3(3 * 7), sc(3 * 2);
  const int64_t hw = 60;
  EXPECT(spectrum_check_apply(5, 12, 3, a.data(), hw, b.data(), hw, 2, pa.data(), pb.data(), m0.data(), m1.data(), m2.data(), m3.data(), sc.data()).empty());
  EXPECT(spectrum_check_apply(5, 12, 3, a.data(), hw, nullptr, hw, 0, pa.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr).empty());
  EXPECT(spectrum_check_apply(5, 12, 3, a.data(), hw, a.data(), hw, 6, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, sc.data()).empty());   // compare(x, x)
  EXPECT(has(spectrum_check_apply(5, 12, 0, a.data(), hw, nullptr, hw, 0, pa.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "n_planes"));
  EXPECT(has(spectrum_check_apply(5, 12, 3, nullptr, hw, nullptr, hw, 0, pa.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "null pointer"));
  EXPECT(has(spectrum_check_apply(5, 12, 3, a.data(), hw, nullptr, hw, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, sc.data()), "needs b"));
  EXPECT(has(spectrum_check_apply(5, 12, 3, a.data(), hw, nullptr, hw, 0, pa.data(), pb.data(), nullptr, nullptr, nullptr, nullptr, nullptr), "output of b"));
  EXPECT(has(spectrum_check_apply(5, 12, 3, a.data(), hw, b.data(), hw, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "no output"));
  EXPECT(has(spectrum_check_apply(5, 12, 3, a.data(), hw, b.data(), hw, -1, pa.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "k_init"));
  EXPECT(has(spectrum_check_apply(5, 12, 3, a.data(), hw, b.data(), hw, 7, pa.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "k_init"));
  EXPECT(has(spectrum_check_apply(5, 12, 3, a.data(), 59, nullptr, hw, 0, pa.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "stride is smaller"));
  EXPECT(has(spectrum_check_apply(5, 12, 3, a.data(), hw, b.data(), 0, 0, pa.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "stride is smaller"));
  EXPECT(has(spectrum_check_apply(5, 12, 3, a.data(), std::numeric_limits<int64_t>::max(), nullptr, hw, 0, pa.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "beyond 2^44"));
  EXPECT(has(spectrum_check_apply(5, 130, std::numeric_limits<int>::max(), a.data(), 650, nullptr, 650, 0, pa.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "tiles"));
  EXPECT(has(spectrum_check_apply(5, 12, 3, a.data(), hw, b.data(), hw, 0, a.data() + 100, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "overlaps an input"));
  EXPECT(has(spectrum_check_apply(5, 12, 3, a.data(), hw, b.data(), hw, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (double*)(b.data() + 2)), "overlaps an input"));
  EXPECT(has(spectrum_check_apply(5, 12, 3, a.data(), hw, b.data(), hw, 0, pa.data(), pa.data() + 8, nullptr, nullptr, nullptr, nullptr, nullptr), "two outputs overlap"));
  EXPECT(has(spectrum_check_apply(5, 12, 3, a.data(), hw, b.data(), hw, 0, nullptr, nullptr, m0.data(), nullptr, m0.data(), nullptr, nullptr), "two outputs overlap"));
  // tiles, scratch and LDS
  const SpecTiles t = spectrum_tiles(721, 1440);
  EXPECT(t.Wh == 721 && t.row_tiles == 12 && t.col_blocks == 23 && spectrum_slot_doubles(721, 1440, 64) == 64LL * 12 * 5 * 721);
  EXPECT(spectrum_tiles(5, 12).Wh == 7 && spectrum_tiles(5, 12).row_tiles == 1 && spectrum_tiles(5, 12).col_blocks == 1);
  EXPECT(spectrum_tiles(70, 144).row_tiles == 2 && spectrum_tiles(70, 144).col_blocks == 3 && spectrum_tiles(19, 45).Wh == 23);
  EXPECT(spectrum_lds_bytes(2) == kSpecReduceBytes && kSpecReduceBytes == 5120 && spectrum_lds_bytes(4096) == 65536);
  // the kernels' indexing on the cases of tests/spectrum_cases.py (a strided batch among them), the smallest and the largest grid
  const int grids[][4] = {{3, 5, 12, 60}, {2, 19, 45, 19 * 45 + 7}, {5, 37, 90, 37 * 90}, {2, 70, 144, 70 * 144}, {1, 33, 1440, 33 * 1440},
                          {2, 2, 2, 4},   {1, 3, 4096, 3 * 4096},   {1, 721, 1440, 721 * 1440}, {1, 65, 63, 65 * 63}};
  for (const auto& gr : grids) replay(gr[0], gr[1], gr[2], gr[3]);
  std::printf("spectrum_host_check: ok\n");
  return 0;
}

// Stand-alone check of the host side of csrc/wx_sht.h and csrc/wx_polefilter.h -- the table builder, the fold test, the tile list,
// the ""-or-reason checkers, the plane overlap test and the per-degree scales -- for a sanitizer build.  No device is touched: it runs on a machine without a GPU.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined tools/sht_host_check.hip -o sht_host_check
//   ./sht_host_check          # prints "sht_host_check: ok" and exits 0, or the first failed expectation
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "../miles-credit_amd/csrc/wx_polefilter.h"
#include "../miles-credit_amd/csrc/wx_sht.h"

#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::printf("sht_host_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                               \
    }                                                                         \
  } while (0)

// the equiangular colatitudes, the northern half mirrored from the southern, and weights that are symmetric and sum to 2
static void nodes(int nlat, std::vector<double>& theta, std::vector<double>& w) {
  theta.resize(nlat);
  w.resize(nlat);
  for (int k = 0; k < nlat; ++k) theta[k] = wx::kShtPi * k / (nlat - 1);
  if (nlat % 2) theta[nlat / 2] = wx::kShtPi / 2;
  for (int k = 0; k < nlat / 2; ++k) theta[k] = wx::kShtPi - theta[nlat - 1 - k];
  double sum = 0.0;
  for (int k = 0; k < nlat; ++k) sum += (w[k] = std::sin(theta[k < nlat / 2 ? nlat - 1 - k : k]) + 1e-3);
  for (int k = 0; k < nlat; ++k) w[k] *= 2.0 / sum;
  for (int k = 0; k < nlat / 2; ++k) w[k] = w[nlat - 1 - k];
}

int main() {
  using namespace wx;
  const int sizes[][4] = {{2, 2, 1, 1}, {2, 4, 3, 3}, {8, 16, 9, 9}, {9, 16, 10, 9}, {33, 64, 34, 33}, {33, 64, 20, 7}, {64, 128, 65, 65}, {181, 360, 182, 181}};
  for (const auto& g : sizes) {
    const int nlat = g[0], nlon = g[1], lmax = g[2], mmax = g[3];
    std::vector<double> theta, w;
    nodes(nlat, theta, w);
    EXPECT(sht_check_create(nlat, nlon, lmax, mmax, theta.data(), w.data(), "ortho").empty());
    EXPECT(sht_folds(nlat, theta.data(), w.data()));
    std::vector<double> col, mirror;
    for (int table = 0; table < 3; ++table)
      for (int m = 0; m < mmax; ++m) {
        EXPECT(sht_check_table(nlat, lmax, mmax, theta.data(), table, m).empty());
        sht_table_column(table, m, lmax, theta.data(), nlat, 1, col);
        EXPECT((int)col.size() == (lmax - m) * nlat);
        for (int l = m; l < lmax; ++l)
          for (int k = 0; k < nlat; ++k) {
            const double v = col[(size_t)(l - m) * nlat + k], s = col[(size_t)(l - m) * nlat + nlat - 1 - k];
            EXPECT(std::isfinite(v) && std::fabs(v) <= std::sqrt((2.0 * lmax + 1.0) * (lmax + 1.0)));
            const double sign = (((l + m) & 1) != (table == 1)) ? -1.0 : 1.0;      // the parity about the equator that the fold uses
            EXPECT(std::fabs(v - sign * s) <= 1e-9 * (1.0 + std::fabs(v)));
            if (table != 0 && l == 0) EXPECT(v == 0.0);
          }
        sht_table_column(table, m, lmax, theta.data(), nlat, 0, mirror);
        for (size_t i = 0; i < col.size(); ++i) EXPECT(mirror[i] == ((m & 1) ? -col[i] : col[i]));
        if (table == 0 && m == 0) EXPECT(std::fabs(col[0] - 1.0 / std::sqrt(4.0 * kShtPi)) < 1e-16);
      }
    for (int fold = 0; fold < 2; ++fold) {                   // the tiles cover every (l, m) with l >= m once and nothing else
      std::vector<int2> tiles;
      sht_tiles(lmax, mmax, fold != 0, tiles);
      std::vector<int> seen((size_t)lmax * mmax, 0);
      for (const int2& t : tiles) {
        EXPECT(t.x >= 0 && t.x < mmax && t.y >= t.x && t.y < lmax);
        for (int c = 0; c < 16; ++c) {
          const int l = t.y + (fold ? 2 : 1) * c;
          if (l < lmax) ++seen[(size_t)l * mmax + t.x];
        }
      }
      for (int l = 0; l < lmax; ++l)
        for (int m = 0; m < mmax; ++m) EXPECT(seen[(size_t)l * mmax + m] == (l >= m ? 1 : 0));
    }
    EXPECT(sht_table_offset(mmax, lmax, nlat) == [&] { int64_t n = 0; for (int m = 0; m < mmax; ++m) n += (int64_t)(lmax - m) * nlat; return n; }());
    // refusals
    EXPECT(!sht_check_create(nlat, nlon, lmax, mmax, theta.data(), w.data(), "backward").empty());
    EXPECT(!sht_check_create(nlat, nlon, lmax, mmax, theta.data(), w.data(), nullptr).empty());
    EXPECT(!sht_check_create(nlat, nlon, 0, mmax, theta.data(), w.data(), "ortho").empty());
    EXPECT(!sht_check_create(nlat, nlon, lmax, lmax + 1, theta.data(), w.data(), "ortho").empty());
    EXPECT(!sht_check_create(nlat, kDftMaxN + 2, lmax, mmax, theta.data(), w.data(), "ortho").empty());
    std::vector<double> bad = theta;
    bad[nlat - 1] = bad[0];
    EXPECT(!sht_check_create(nlat, nlon, lmax, mmax, bad.data(), w.data(), "ortho").empty());
    bad = theta;
    bad[nlat - 1 - nlat / 3] -= 0x1p-50;
    EXPECT(!sht_folds(nlat, bad.data(), w.data()));
    bad = w;
    bad[0] = NAN;
    EXPECT(!sht_check_create(nlat, nlon, lmax, mmax, theta.data(), bad.data(), "ortho").empty());
    // the calls' checkers: pointers are only compared, never followed
    std::vector<float> x((size_t)2 * nlat * nlon + 8);
    std::vector<double> c((size_t)2 * lmax * mmax * 2), z((size_t)2 * (lmax + mmax));
    const int64_t hw = (int64_t)nlat * nlon;
    EXPECT(sht_check_analysis(nlat, nlon, lmax, mmax, 2, x.data(), hw, kShtF32, c.data()).empty());
    EXPECT(!sht_check_analysis(nlat, nlon, lmax, mmax, 0, x.data(), hw, kShtF32, c.data()).empty());
    EXPECT(!sht_check_analysis(nlat, nlon, lmax, mmax, 2, x.data(), hw - 1, kShtF32, c.data()).empty());
    EXPECT(!sht_check_analysis(nlat, nlon, lmax, mmax, 2, x.data(), INT64_MAX / 2, kShtF32, c.data()).empty());
    EXPECT(!sht_check_analysis(nlat, nlon, lmax, mmax, 2, x.data(), hw, 7, c.data()).empty());
    EXPECT(!sht_check_analysis(nlat, nlon, lmax, mmax, 1, c.data(), hw, kShtF32, c.data()).empty());
    EXPECT(!sht_check_analysis(nlat, nlon, lmax, mmax, 2, nullptr, hw, kShtF32, c.data()).empty());
    EXPECT(sht_check_synthesis(nlat, nlon, lmax, mmax, 2, c.data(), x.data(), kShtF32).empty());
    EXPECT(!sht_check_synthesis(nlat, nlon, lmax, mmax, 2, c.data(), c.data(), kShtF64).empty());
    EXPECT(sht_check_vector(nlat, nlon, lmax, mmax, 1, x.data(), hw, x.data() + hw, hw, kShtF32, c.data(), c.data() + (size_t)lmax * mmax * 2).empty());
    EXPECT(!sht_check_vector(nlat, nlon, lmax, mmax, 1, x.data(), hw, x.data() + hw, hw, kShtF32, c.data(), c.data()).empty());
    EXPECT(sht_check_spectra(lmax, mmax, 2, c.data(), z.data(), z.data() + 2 * mmax).empty());
    EXPECT(!sht_check_spectra(lmax, mmax, 2, c.data(), nullptr, nullptr).empty());
    EXPECT(!sht_check_spectra(lmax, mmax, 2, c.data(), z.data(), z.data() + 1).empty());
    // the inverse vector transform: the toroidal part and one component may be missing
    EXPECT(sht_check_vector_synthesis(nlat, nlon, lmax, mmax, 1, c.data(), c.data() + (size_t)lmax * mmax * 2, x.data(), x.data() + hw, kShtF32).empty());
    EXPECT(sht_check_vector_synthesis(nlat, nlon, lmax, mmax, 1, c.data(), nullptr, nullptr, x.data(), kShtF32).empty());
    EXPECT(!sht_check_vector_synthesis(nlat, nlon, lmax, mmax, 1, nullptr, c.data(), x.data(), x.data() + hw, kShtF32).empty());
    EXPECT(!sht_check_vector_synthesis(nlat, nlon, lmax, mmax, 1, c.data(), nullptr, nullptr, nullptr, kShtF32).empty());
    EXPECT(!sht_check_vector_synthesis(nlat, nlon, lmax, mmax, 1, c.data(), nullptr, x.data(), x.data() + 1, kShtF32).empty());
    // the pole filter's checkers and its per-degree scales
    std::vector<float> sig((size_t)nlat, 1.f);
    const int indpol = (nlat - 1) / 2;
    EXPECT(polefilter_check_create(nlat, nlon, 6.37122e6, indpol, nlon / 2, sig.data()).empty());
    EXPECT(!polefilter_check_create(nlat, nlon, 6.37122e6, indpol + 1, 0, sig.data()).empty());
    EXPECT(!polefilter_check_create(nlat, nlon, 0.0, indpol, 0, sig.data()).empty());
    EXPECT(!polefilter_check_create(nlat, nlon, NAN, indpol, 0, sig.data()).empty());
    EXPECT(!polefilter_check_create(nlat, nlon, 1.0, indpol, nlon / 2 + 1, sig.data()).empty());
    EXPECT(!polefilter_check_create(nlat, nlon, 1.0, -1, 0, sig.data()).empty());
    sig[nlat - 1] = INFINITY;
    EXPECT(!polefilter_check_create(nlat, nlon, 1.0, indpol, 0, sig.data()).empty());
    const PoleField a = {x.data(), hw}, b = {x.data() + hw, hw}, ai = {x.data(), 2 * hw}, bi = {x.data() + hw, 2 * hw}, shifted = {x.data() + 1, hw};
    EXPECT(polefilter_check_call(nlat, nlon, 1, kShtF32, 3, 1e8, &a, &b, 1).empty());
    EXPECT(polefilter_check_call(nlat, nlon, 2, kShtF32, 0, 0.0, &a, &a, 1).empty());           // in place
    EXPECT(!polefilter_check_call(nlat, nlon, 2, kShtF32, 3, 1e8, &a, &b, 1).empty());          // plane 1 of a is plane 0 of b
    EXPECT(!polefilter_check_call(nlat, nlon, 1, kShtF32, 3, 1e8, &a, &shifted, 1).empty());
    EXPECT(!polefilter_check_call(nlat, nlon, 1, kShtF32, -1, 1e8, &a, &b, 1).empty());
    EXPECT(!polefilter_check_call(nlat, nlon, 1, kShtF32, 1, INFINITY, &a, &b, 1).empty());
    EXPECT(!polefilter_check_call(nlat, nlon, 0, kShtF32, 1, 1e8, &a, &b, 1).empty());
    EXPECT(!polefilter_check_call(nlat, nlon, 1, 9, 1, 1e8, &a, &b, 1).empty());
    const PoleField pair_in[2] = {ai, bi}, pair_bad[2] = {ai, ai};
    EXPECT(polefilter_check_call(nlat, nlon, 1, kShtF32, 1, 2e16, pair_in, pair_in, 2).empty()); // interleaved planes, in place
    EXPECT(!polefilter_check_call(nlat, nlon, 1, kShtF32, 1, 2e16, pair_in, pair_bad, 2).empty());
    EXPECT(!polefilter_planes_overlap(ai, bi, 1, hw, 4) && polefilter_planes_overlap(ai, shifted, 1, hw, 4));
    EXPECT(polefilter_workspace(nlat, nlon, lmax, mmax, 40) == polefilter_workspace(nlat, nlon, lmax, mmax, kPoleChunk));
    std::vector<double> sg, sdg;
    polefilter_scales(lmax, 6.37122e6, sg, sdg);
    EXPECT((int)sg.size() == lmax && sg[0] == 0.0 && sdg[0] == 0.0);
    for (int l = 1; l < lmax; ++l) EXPECT(sg[l] > sg[l - 1] && sdg[l] == -(sg[l] * sg[l]));
  }
  std::printf("sht_host_check: ok\n");
  return 0;
}

// Stand-alone host check of the host-only helpers of csrc/wx_regrid.h -- regrid_check_create (what wx_regrid_create refuses) and
// regrid_plan (the sliced-ELL layout and the long-row list the kernels index) -- meant for AddressSanitizer / UBSan.  The kernels'
// own index arithmetic is replayed on the host over exactly-sized heap arrays, so an index past an array is caught here and not on
// a GPU.  It calls no HIP function, so it runs on a machine without a GPU:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/regrid_host_check.hip -o regrid_host_check && ./regrid_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../miles-credit_amd/csrc/wx_regrid.h"

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rng() { return rng_state = rng_state * 1664525u + 1013904223u; }

// the two kernels for one plane, with their indexing: short rows through the slices, long rows lane by lane and a butterfly
static std::vector<float> replay(const wx::RegridPlan& p, int64_t n_a, int64_t n_b, const std::vector<float>& x) {
  using namespace wx;
  std::vector<float> y((size_t)n_b, -1.f);
  EXPECT((int64_t)x.size() == n_a && (int64_t)p.row_len.size() == n_b);
  EXPECT((int64_t)p.slice_base.size() == (n_b + kRegridSlice - 1) / kRegridSlice + 1 && p.ell_col.size() == (size_t)p.slice_base.back());
  for (int64_t r = 0; r < n_b; ++r) {
    const int len = p.row_len[r];
    if (len < 0) continue;
    EXPECT(len <= kRegridLongRow);
    float acc = 0.f;
    const int64_t base = p.slice_base[r / kRegridSlice] + (r % kRegridSlice);
    for (int j = 0; j < len; ++j) {
      const int64_t at = base + (int64_t)j * kRegridSlice;
      EXPECT(at < p.slice_base[r / kRegridSlice + 1]);
      acc = fmaf(p.ell_val.at(at), x.at(p.ell_col.at(at)), acc);
    }
    y[r] = acc;
  }
  EXPECT(p.long_ptr.size() == p.long_row.size() + 1 && p.long_col.size() == (size_t)p.long_ptr.back());
  for (size_t i = 0; i < p.long_row.size(); ++i) {
    float lane[64];
    for (int l = 0; l < 64; ++l) {
      lane[l] = 0.f;
      for (int64_t e = p.long_ptr[i] + l; e < p.long_ptr[i + 1]; e += 64) lane[l] = fmaf(p.long_val.at(e), x.at(p.long_col.at(e)), lane[l]);
    }
    for (int off = 32; off >= 1; off >>= 1) {
      float next[64];
      for (int l = 0; l < 64; ++l) next[l] = lane[l] + lane[l ^ off];
      for (int l = 0; l < 64; ++l) lane[l] = next[l];
    }
    EXPECT(p.row_len.at(p.long_row[i]) == -1 && y[p.long_row[i]] == -1.f);
    y[p.long_row[i]] = lane[0];
  }
  return y;
}

static void check_matrix(int64_t n_a, const std::vector<int>& lens) {
  using namespace wx;
  const int64_t n_b = (int64_t)lens.size();
  std::vector<int64_t> row_ptr(1, 0);
  std::vector<int> col;
  std::vector<float> val;
  for (int len : lens) {
    for (int j = 0; j < len; ++j) {
      col.push_back((int)(rng() % n_a));
      val.push_back((float)(rng() % 1000) / 512.f - 0.9f);
    }
    row_ptr.push_back((int64_t)col.size());
  }
  if (col.empty()) { col.push_back(0); val.push_back(0.f); }      // never read: the entry count is 0
  EXPECT(regrid_check_create(n_a, n_b, row_ptr.data(), col.data(), val.data()).empty());
  const RegridPlan p = regrid_plan(n_b, row_ptr.data(), col.data(), val.data());
  std::vector<float> x((size_t)n_a);
  for (float& v : x) v = (float)(rng() % 4096) / 64.f - 20.f;
  const std::vector<float> y = replay(p, n_a, n_b, x);
  int n_long = 0;
  for (int64_t r = 0; r < n_b; ++r) {
    double ref = 0.0, mag = 0.0;
    for (int64_t e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
      ref += (double)val[e] * x[col[e]];
      mag += std::fabs((double)val[e] * x[col[e]]);
    }
    EXPECT(std::fabs(y[r] - ref) <= (lens[r] + 2) * 5.9604644775390625e-08 * mag);      // every row written, 0 for an empty one
    EXPECT(p.row_len[r] == (lens[r] > kRegridLongRow ? -1 : lens[r]));
    n_long += lens[r] > kRegridLongRow;
  }
  EXPECT((int)p.long_row.size() == n_long);
  for (int64_t s = 0; s * kRegridSlice < n_b; ++s) {                                      // a slice is as wide as its longest short row
    int width = 0;
    for (int64_t r = s * kRegridSlice; r < std::min(n_b, (s + 1) * kRegridSlice); ++r) width = std::max(width, p.row_len[r]);
    EXPECT(p.slice_base[s + 1] - p.slice_base[s] == (int64_t)width * kRegridSlice);
  }
}

int main() {
  using namespace wx;
  // ---- regrid_plan, replayed
  check_matrix(7, {3});
  check_matrix(7, {0});
  check_matrix(50, std::vector<int>(64, 4));
  check_matrix(50, std::vector<int>(65, 4));
  {
    std::vector<int> lens;                    // 301 rows: empty, 1, both sides of the long-row threshold, several passes of the wave loop
    for (int r = 0; r < 301; ++r) lens.push_back(1 + (int)(rng() % 40));
    lens[3] = 0; lens[5] = 1; lens[64] = 63; lens[70] = 64; lens[71] = 65; lens[130] = 200; lens[200] = 700; lens[299] = 0; lens[300] = 65;
    check_matrix(2211, lens);
    for (int& l : lens) l = 0;
    check_matrix(2211, lens);
    for (int& l : lens) l = 65 + (int)(rng() % 100);      // every row long: slices of width 0
    check_matrix(2211, lens);
  }
  // ---- regrid_check_create: exactly-sized heap arrays, so a read the check should not make is caught
  {
    std::vector<int64_t> rp = {0, 1, 3};
    std::vector<int> col = {0, 1, 2};
    std::vector<float> val = {1.f, .5f, .5f};
    EXPECT(regrid_check_create(3, 2, rp.data(), col.data(), val.data()).empty());
    EXPECT(regrid_check_create(3, 2, nullptr, col.data(), val.data()) == "null weight array");
    EXPECT(regrid_check_create(3, 2, rp.data(), nullptr, val.data()) == "null weight array");
    EXPECT(regrid_check_create(3, 2, rp.data(), col.data(), nullptr) == "null weight array");
    EXPECT(regrid_check_create(0, 2, rp.data(), col.data(), val.data()) == "n_a must be 1 .. 2^31 - 1, got 0");
    EXPECT(regrid_check_create(2147483648LL, 2, rp.data(), col.data(), val.data()) == "n_a must be 1 .. 2^31 - 1, got 2147483648");
    EXPECT(regrid_check_create(3, 0, rp.data(), col.data(), val.data()) == "n_b must be 1 .. 2^31 - 1, got 0");
    EXPECT(regrid_check_create(3, 2147483648LL, rp.data(), col.data(), val.data()) == "n_b must be 1 .. 2^31 - 1, got 2147483648");   // row_ptr not read
    EXPECT(regrid_check_create(3, -5, rp.data(), col.data(), val.data()) == "n_b must be 1 .. 2^31 - 1, got -5");
    EXPECT(regrid_check_create(2, 2, rp.data(), col.data(), val.data()) == "column index 2 at entry 2 lies outside [0, n_a = 2)");
    col[1] = -1;
    EXPECT(regrid_check_create(3, 2, rp.data(), col.data(), val.data()) == "column index -1 at entry 1 lies outside [0, n_a = 3)");
    rp = {1, 1, 3};
    EXPECT(regrid_check_create(3, 2, rp.data(), col.data(), val.data()) == "row_ptr must start at 0, got 1");
    rp = {0, 2, 1};
    EXPECT(regrid_check_create(3, 2, rp.data(), col.data(), val.data()) == "row_ptr decreases at row 1");
    rp = {0, 2147483648LL};
    EXPECT(regrid_check_create(3, 1, rp.data(), col.data(), val.data()) == "the entry count must stay below 2^31, got 2147483648");      // col not read
    rp = {0, 0, 0};
    EXPECT(regrid_check_create(3, 2, rp.data(), col.data(), val.data()).empty());      // no entries: col is not read
  }
  std::puts("regrid host check ok");
  return 0;
}

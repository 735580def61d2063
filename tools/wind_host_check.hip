// Stand-alone host check of the two host-only helpers of csrc/wx_wind.h -- wind_check_create (what wx_wind_create refuses) and
// wind_build_vars (the plane table wx_wind_apply hands to the kernels) -- meant for AddressSanitizer / UBSan.  It calls no HIP
// function, so it runs on a machine without a GPU:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/wind_host_check.hip -o wind_host_check && ./wind_host_check
#include <cstdio>
#include <cstdlib>

#include "../miles-credit_amd/csrc/wx_wind.h"

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

int main() {
  using namespace wx;
  // ---- wind_check_create: exactly-sized heap arrays, so a read past a kernel's end is caught
  std::vector<float> k5(5, 0.2f), k13(13, 1.0f / 13), k17(17, 1.0f / 17), k33(33, 1.0f / 33), k65(65, 1.0f / 65), k35(35, 1.0f / 35);
  {
    const float* w[4] = {k5.data(), k13.data(), k17.data(), k33.data()};
    const int n[4] = {5, 13, 17, 33};
    EXPECT(wind_check_create(192, 288, w, n, 5, 15, 2.8f).empty());
    EXPECT(wind_check_create(1, 1, w, n, 1, 1, 0.f).empty());
    EXPECT(has(wind_check_create(0, 288, w, n, 5, 15, 2.8f), "bad geometry"));
    EXPECT(has(wind_check_create(192, 288, w, n, 4, 15, 2.8f), "must be odd"));
    EXPECT(has(wind_check_create(192, 288, w, n, 5, 0, 2.8f), "must be odd"));
    EXPECT(has(wind_check_create(192, 288, w, n, 35, 15, 2.8f), "exceeds the supported 33 x 65"));
    EXPECT(has(wind_check_create(192, 288, w, n, 5, 67, 2.8f), "exceeds the supported 33 x 65"));
    EXPECT(has(wind_check_create(192, 288, w, n, 5, 15, INFINITY), "threshold must be finite"));
    const int even[4] = {5, 12, 17, 33};
    EXPECT(has(wind_check_create(192, 288, w, even, 5, 15, 2.8f), "smoothing longitude kernel size 12 must be odd"));
    const float* null_w[4] = {k5.data(), k13.data(), nullptr, k33.data()};
    EXPECT(has(wind_check_create(192, 288, null_w, n, 5, 15, 2.8f), "null falloff latitude weights"));
  }
  {
    const float* w[4] = {k33.data(), k65.data(), k33.data(), k65.data()};     // the largest supported
    const int n[4] = {33, 65, 33, 65};
    EXPECT(wind_check_create(721, 1440, w, n, 33, 65, 3.0f).empty());
    const float* big[4] = {k35.data(), k65.data(), k33.data(), k65.data()};
    const int nbig[4] = {35, 65, 33, 65};
    EXPECT(has(wind_check_create(721, 1440, big, nbig, 33, 65, 3.0f), "smoothing latitude kernel size 35 exceeds the supported 33"));
    k65[64] = NAN;
    EXPECT(has(wind_check_create(721, 1440, w, n, 33, 65, 3.0f), "weights must be finite"));
  }
  // ---- wind_build_vars
  std::vector<float> a(8), b(8);     // never dereferenced: only their addresses travel
  {
    std::vector<const float*> src = {a.data(), b.data(), a.data() + 1};
    std::vector<float*> dst = {b.data(), a.data(), b.data() + 1};
    std::vector<int64_t> bs = {100, 200, 300};
    std::vector<int32_t> nl = {5, 32, 256};
    std::vector<int32_t> lv = {1, 2, 3, 7, 63, 64, 255, 300};
    WindVars t;
    EXPECT(wind_build_vars(t, 3, src.data(), bs.data(), nl.data(), dst.data(), lv.data(), (int)lv.size(), 2, 60).empty());
    EXPECT(t.n_vars == 3 && t.lvl0[0] == 0 && t.lvl0[1] == 5 && t.lvl0[2] == 37 && t.lvl0[3] == 293);
    EXPECT(t.target[0][0] == 0xEull && t.target[0][1] == 0);                                          // 7 and up do not exist: skipped
    EXPECT(t.target[1][0] == 0x8Eull);
    EXPECT(t.target[2][0] == (0x8Eull | (1ull << 63)) && t.target[2][1] == 1ull && t.target[2][3] == (1ull << 63));
    EXPECT(t.src[2] == a.data() + 1 && t.dst[1] == a.data() && t.bstride[2] == 300);
    EXPECT(wind_build_vars(t, 3, src.data(), bs.data(), nl.data(), dst.data(), nullptr, 0, 1, 60).empty() && t.target[2][0] == 0);
    EXPECT(has(wind_build_vars(t, 3, src.data(), bs.data(), nl.data(), dst.data(), nullptr, 2, 1, 60), "null target-level list"));
    EXPECT(has(wind_build_vars(t, 0, src.data(), bs.data(), nl.data(), dst.data(), lv.data(), 1, 1, 60), "1..32 variables"));
    EXPECT(has(wind_build_vars(t, 33, src.data(), bs.data(), nl.data(), dst.data(), lv.data(), 1, 1, 60), "1..32 variables"));
    EXPECT(has(wind_build_vars(t, 3, src.data(), bs.data(), nl.data(), dst.data(), lv.data(), 1, 0, 60), "batch must be >= 1"));
    EXPECT(has(wind_build_vars(t, 3, src.data(), bs.data(), nl.data(), dst.data(), lv.data(), 8, 1 << 20, 60), "grid limit"));
    std::vector<int32_t> neg = {2, -1};
    EXPECT(has(wind_build_vars(t, 3, src.data(), bs.data(), nl.data(), dst.data(), neg.data(), 2, 1, 60), "negative target level"));
    nl[1] = 257;
    EXPECT(has(wind_build_vars(t, 3, src.data(), bs.data(), nl.data(), dst.data(), lv.data(), 8, 1, 60), "1..256 levels"));
    nl[1] = 32;
    bs[0] = -1;
    EXPECT(has(wind_build_vars(t, 3, src.data(), bs.data(), nl.data(), dst.data(), lv.data(), 8, 2, 60), "negative batch stride"));
    EXPECT(wind_build_vars(t, 3, src.data(), bs.data(), nl.data(), dst.data(), lv.data(), 8, 1, 60).empty());   // a single item: the stride is not used
    src[1] = nullptr;
    EXPECT(has(wind_build_vars(t, 3, src.data(), bs.data(), nl.data(), dst.data(), lv.data(), 8, 1, 60), "null tensor pointer"));
  }
  {   // the full table: 32 variables of 256 levels, every level a target
    std::vector<const float*> src(32, a.data());
    std::vector<float*> dst(32, b.data());
    std::vector<int64_t> bs(32, 0);
    std::vector<int32_t> nl(32, 256), lv(256);
    for (int i = 0; i < 256; ++i) lv[i] = i;
    WindVars t;
    EXPECT(wind_build_vars(t, 32, src.data(), bs.data(), nl.data(), dst.data(), lv.data(), 256, 1, 4).empty());
    EXPECT(t.lvl0[32] == 8192 && t.target[31][3] == ~0ull);
  }
  EXPECT(wind_lds_floats(33, 65) * sizeof(float) <= 65536);     // the largest tile fits the default dynamic LDS limit
  EXPECT(wind_halo4(13) == 8 && wind_halo4(65) == 32 && wind_halo4(1) == 0 && wind_halo4(3) == 4);
  std::puts("wind host check ok");
  return 0;
}

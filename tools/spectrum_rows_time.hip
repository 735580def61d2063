// Stand-alone timing of the folded transform of csrc/wx_spectrum.h against the unfolded one it grew out of, on the same planes on the
// same GPU: spectrum_rows_kernel<true> once (two fields, squares and row sums included) against perturb_rows_fwd_kernel of
// csrc/wx_perturb.h twice (one run per field, the half-complex rows written to memory and nothing else done with them).  HIP events,
// warm-up, repeats, median / min / max, one JSON line.
//   hipcc --offload-arch=gfx950 -std=c++17 -O3 tools/spectrum_rows_time.hip -o tools/_build/spectrum_rows_time
//   tools/_build/spectrum_rows_time [planes = 64] [H = 721] [W = 1440] [reps = 5] [warmup = 2]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../miles-credit_amd/csrc/wx_perturb.h"
#include "../miles-credit_amd/csrc/wx_spectrum.h"

#define CHECK(expr)                                                                              \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
      std::exit(1);                                                                              \
    }                                                                                            \
  } while (0)

template <typename F>
static void timed(F&& fn, int warmup, int reps, float out[3]) {
  for (int i = 0; i < warmup; ++i) fn();
  CHECK(hipDeviceSynchronize());
  std::vector<float> ms(reps);
  hipEvent_t a, b;
  CHECK(hipEventCreate(&a));
  CHECK(hipEventCreate(&b));
  for (int i = 0; i < reps; ++i) {
    CHECK(hipEventRecord(a, nullptr));
    fn();
    CHECK(hipEventRecord(b, nullptr));
    CHECK(hipEventSynchronize(b));
    CHECK(hipEventElapsedTime(&ms[i], a, b));
  }
  CHECK(hipEventDestroy(a));
  CHECK(hipEventDestroy(b));
  std::sort(ms.begin(), ms.end());
  out[0] = ms[reps / 2];
  out[1] = ms.front();
  out[2] = ms.back();
}

int main(int argc, char** argv) {
  const int P = argc > 1 ? std::atoi(argv[1]) : 64, H = argc > 2 ? std::atoi(argv[2]) : 721, W = argc > 3 ? std::atoi(argv[3]) : 1440;
  const int reps = argc > 4 ? std::atoi(argv[4]) : 5, warmup = argc > 5 ? std::atoi(argv[5]) : 2;
  const std::string why = wx::spectrum_check_create(H, W, nullptr);
  if (!why.empty() || P < 1 || reps < 1 || warmup < 0) {
    std::fprintf(stderr, "spectrum_rows_time: %s\n", why.empty() ? "planes and reps must be >= 1" : why.c_str());
    return 2;
  }
  const wx::SpecTiles t = wx::spectrum_tiles(H, W);
  const int Wh = t.Wh, N = 2 * Wh, M = P * H;
  const size_t n = (size_t)P * H * W;
  std::vector<float> host(n);
  uint32_t s = 12345u;
  float walk = 0.f;
  for (size_t i = 0; i < n; ++i) {      // a red field around 250, like the cases of the tests
    s = s * 1664525u + 1013904223u;
    walk = (i % W == 0) ? 0.f : walk + ((float)(s >> 8) / 16777216.f - 0.5f) * 6.f;
    host[i] = 250.f + walk;
  }
  float *a = nullptr, *b = nullptr;
  double *half = nullptr, *slots = nullptr;
  double2* tab = nullptr;
  CHECK(hipMalloc(&a, n * 4));
  CHECK(hipMalloc(&b, n * 4));
  CHECK(hipMalloc(&half, (size_t)M * N * 8));
  CHECK(hipMalloc(&slots, (size_t)wx::spectrum_slot_doubles(H, W, P) * 8));
  CHECK(hipMemcpy(a, host.data(), n * 4, hipMemcpyHostToDevice));
  for (size_t i = 0; i < n; ++i) host[i] += (float)(i % 7) * 0.1f;
  CHECK(hipMemcpy(b, host.data(), n * 4, hipMemcpyHostToDevice));
  std::vector<double2> tw;
  wx::dft_table(W, tw);
  CHECK(hipMalloc(&tab, tw.size() * sizeof(double2)));
  CHECK(hipMemcpy(tab, tw.data(), tw.size() * sizeof(double2), hipMemcpyHostToDevice));

  wx::SpecRowsArgs r;
  r.a = a; r.b = b; r.a_stride = r.b_stride = (int64_t)H * W; r.w = nullptr; r.psd_a = r.psd_b = nullptr; r.slots = slots;
  r.H = H; r.W = W; r.row_tiles = t.row_tiles; r.col_blocks = t.col_blocks;
  const dim3 fold_grid((unsigned)((int64_t)P * t.row_tiles * t.col_blocks));
  const dim3 rows_grid((unsigned)wx::cdiv(N, 64), (unsigned)wx::cdiv(M, 64));
  float folded[3], plain[3];
  timed([&] { hipLaunchKernelGGL(wx::spectrum_rows_kernel<true>, fold_grid, dim3(256), wx::spectrum_lds_bytes(W), nullptr, r, tab); }, warmup, reps,
        folded);
  CHECK(hipGetLastError());
  timed(
      [&] {
        hipLaunchKernelGGL(wx::perturb_rows_fwd_kernel, rows_grid, dim3(256), wx::dft_lds_bytes(W), nullptr, a, M, W, tab, half);
        hipLaunchKernelGGL(wx::perturb_rows_fwd_kernel, rows_grid, dim3(256), wx::dft_lds_bytes(W), nullptr, b, M, W, tab, half);
      },
      warmup, reps, plain);
  CHECK(hipGetLastError());
  const double fold_flop = 2.0 * M * 2.0 * 2.0 * Wh * Wh, plain_flop = 2.0 * 2.0 * M * (double)N * W;
  std::printf("{\"what\": \"folded spectrum_rows_kernel<b> vs two perturb_rows_fwd_kernel\", \"planes\": %d, \"grid\": [%d, %d], "
              "\"folded_ms\": %.3f, \"folded_ms_min\": %.3f, \"folded_ms_max\": %.3f, \"folded_TFLOP_per_s\": %.2f, "
              "\"two_pass_a_ms\": %.3f, \"two_pass_a_ms_min\": %.3f, \"two_pass_a_ms_max\": %.3f, \"pass_a_TFLOP_per_s\": %.2f, "
              "\"two_pass_a_over_folded\": %.2f, \"reps\": %d}\n",
              P, H, W, folded[0], folded[1], folded[2], fold_flop / (folded[0] * 1e-3) / 1e12, plain[0], plain[1], plain[2],
              plain_flop / (plain[0] * 1e-3) / 1e12, plain[0] / folded[0], reps);
  CHECK(hipFree(a));
  CHECK(hipFree(b));
  CHECK(hipFree(half));
  CHECK(hipFree(slots));
  CHECK(hipFree(tab));
  return 0;
}

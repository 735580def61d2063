// Stand-alone host check of csrc/wx_tisr.h, meant for AddressSanitizer / UBSan.  The per-sub-step arithmetic of the table kernel is
// host-device code (tisr_civil, tisr_days32, tisr_tsi, tisr_entry, tisr_term) and runs here as it is; the two kernels' index arithmetic
// -- launch pairs, table rows, LDS chunks, points per thread, plane strides -- is replayed over exactly-sized heap arrays, so an index
// past an array is caught here and not on a GPU.  The planes are held to a direct fp64 evaluation with cos(hour angle) per term.  It
// calls no HIP function, so it runs on a machine without a GPU:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/tisr_host_check.hip -o tisr_host_check && ./tisr_host_check
// `tisr_host_check --table tsi.f32 t_end_ns period_ns n_steps out.bin` writes the float32 days [n_steps + 1] and the table
// [n_steps + 1][4] of one target time (tsi.f32: the table's times, then its values, raw float32), to compare with tests/tisr_oracle.py.
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <vector>

#include "../miles-credit_amd/csrc/wx_tisr.h"

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rng() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

// Tisr::compute without HIP: the same launch pairs, grids and kernels' indexing.  dst holds exactly what the caller promises.
static void replay(int64_t npts, const std::vector<float>& a, const std::vector<float>& b, const std::vector<float>& c,
                   const std::vector<float>& tsi_t, const std::vector<float>& tsi_v, const std::vector<int64_t>& t_end, int64_t period_ns,
                   int n_steps, std::vector<float>& dst, int64_t plane_stride) {
  using namespace wx;
  const int n_times = (int)t_end.size(), n_tsi = (int)tsi_t.size();
  const int64_t n_entries = (int64_t)n_steps + 1;
  const int per_launch = (int)std::max<int64_t>(1, std::min<int64_t>(kTisrMaxTimes, kTisrTableEntries / n_entries));
  std::vector<float4> table((size_t)(std::min<int64_t>(per_launch, n_times) * n_entries));
  const int64_t step_ns = period_ns / n_steps;
  for (int t0 = 0; t0 < n_times; t0 += per_launch) {
    const int nt = std::min(per_launch, n_times - t0);
    TisrTimes tt;
    std::memset(&tt, 0, sizeof(tt));
    for (int i = 0; i < nt; ++i) tt.t_end[i] = t_end.at(t0 + i);
    const int64_t total = (int64_t)nt * n_entries;
    for (int64_t blk = 0; blk < (total + 255) / 256; ++blk)             // tisr_table_kernel
      for (int tid = 0; tid < 256; ++tid) {
        const int64_t idx = blk * 256 + tid;
        if (idx >= (int64_t)nt * n_entries) continue;
        const int i = (int)(idx / n_entries);
        const int k = (int)(idx - (int64_t)i * n_entries);
        EXPECT(i >= 0 && i < kTisrMaxTimes && k >= 0 && k <= n_steps);
        const int64_t ns = tt.t_end[i] - (int64_t)(n_steps - k) * step_ns;
        table.at(idx) = tisr_entry(ns, (k == 0 || k == n_steps) ? 0.5 : 1.0, (double)step_ns / 1e9, tsi_t.data(), tsi_v.data(), n_tsi);
      }
    const int64_t gx = (npts + 256 * kTisrPoints - 1) / (256 * kTisrPoints), gy = (nt + kTisrTimesPerBlock - 1) / kTisrTimesPerBlock;
    const int64_t dst0 = (int64_t)t0 * plane_stride;
    for (int64_t by = 0; by < gy; ++by)                                  // tisr_integrate_kernel
      for (int64_t bx = 0; bx < gx; ++bx) {
        const int t_first = (int)by * kTisrTimesPerBlock, t_last = std::min(nt, t_first + kTisrTimesPerBlock);
        for (int t = t_first; t < t_last; ++t) {
          std::vector<double> acc(256 * kTisrPoints, 0.0);
          for (int k0 = 0; k0 < (int)n_entries; k0 += kTisrChunk) {
            const int m = std::min(kTisrChunk, (int)n_entries - k0);
            std::vector<float4> tab(kTisrChunk);
            for (int tid = 0; tid < 256; ++tid)
              if (tid < m) tab.at(tid) = table.at((int64_t)t * n_entries + k0 + tid);
            for (int tid = 0; tid < 256; ++tid)
              for (int q = 0; q < kTisrPoints; ++q) {
                const int64_t p = bx * (256 * kTisrPoints) + tid + (int64_t)q * 256;
                if (p >= npts) continue;
                for (int k = 0; k < m; ++k) acc[q * 256 + tid] += (double)tisr_term(tab.at(k), a.at(p), b.at(p), c.at(p));
              }
          }
          for (int tid = 0; tid < 256; ++tid)
            for (int q = 0; q < kTisrPoints; ++q) {
              const int64_t p = bx * (256 * kTisrPoints) + tid + (int64_t)q * 256;
              if (p < npts) {
                float& out = dst.at(dst0 + (int64_t)t * plane_stride + p);
                EXPECT(out == -7777.25f);                               // every element is written once
                out = (float)acc[q * 256 + tid];
              }
            }
        }
      }
  }
}

// The reference's formula term by term in fp64, from the same float32 days and float32 TSI.
static double direct(double lat, double lon, int64_t t_end, int64_t period_ns, int n_steps, const std::vector<float>& tsi_t,
                     const std::vector<float>& tsi_v) {
  using namespace wx;
  const int64_t step = period_ns / n_steps;
  const double rad = 3.14159265358979323846 / 180.0;
  double sum = 0.0;
  for (int k = 0; k <= n_steps; ++k) {
    const int64_t ns = t_end - (int64_t)(n_steps - k) * step;
    const TisrDate d = tisr_civil(ns);
    const float fy = (float)((double)d.year + ((double)(d.doy - 1) + (double)d.ns_of_day / 86400e9) / (365 + d.leap));
    const double tsi = tisr_tsi(fy, tsi_t.data(), tsi_v.data(), (int)tsi_t.size());
    const double j = tisr_days32(ns), theta = j / 365.25, phase = std::fmod(std::fmod(j, 1.0) + 1.0, 1.0);
    const double rel = 1.7535 + 6.283076 * theta, rem = 6.240041 + 6.283020 * theta, rlls = 4.8951 + 6.283076 * theta;
    const double rllls = 4.8952 + 6.283320 * theta - 0.0075 * std::sin(rel) - 0.0326 * std::cos(rel) - 0.0003 * std::sin(2 * rel) + 0.0002 * std::cos(2 * rel);
    const double sd = std::sin(0.409093) * std::sin(rllls), cd = std::sqrt(1.0 - sd * sd);
    const double eot = 591.8 * std::sin(2 * rlls) - 459.4 * std::sin(rem) + 39.5 * std::sin(rem) * std::cos(2 * rlls) - 12.7 * std::sin(4 * rlls) - 4.8 * std::sin(2 * rem);
    const double dist = 1.0001 - 0.0163 * std::sin(rel) + 0.0037 * std::cos(rel);
    const double ha = 360.0 * (phase + eot / 86400.0) + lon;
    const double cz = std::cos(lat * rad) * cd * std::cos(ha * rad) + std::sin(lat * rad) * sd;
    sum += ((k == 0 || k == n_steps) ? 0.5 : 1.0) * tsi / (dist * dist) * std::max(cz, 0.0);
  }
  return sum * ((double)step / 1e9);
}

static int write_table(char** argv) {
  using namespace wx;
  std::FILE* f = std::fopen(argv[2], "rb");
  EXPECT(f);
  std::vector<float> raw;
  float x;
  while (std::fread(&x, 4, 1, f) == 1) raw.push_back(x);
  std::fclose(f);
  EXPECT(raw.size() >= 4 && raw.size() % 2 == 0);
  const int n = (int)raw.size() / 2;
  const int64_t t_end = std::atoll(argv[3]), period = std::atoll(argv[4]);
  const int n_steps = std::atoi(argv[5]);
  EXPECT(n_steps >= 1 && period >= n_steps);
  const int64_t step = period / n_steps;
  std::FILE* out = std::fopen(argv[6], "wb");
  EXPECT(out);
  for (int k = 0; k <= n_steps; ++k) {
    const float j = tisr_days32(t_end - (int64_t)(n_steps - k) * step);
    std::fwrite(&j, 4, 1, out);
  }
  for (int k = 0; k <= n_steps; ++k) {
    const float4 e = tisr_entry(t_end - (int64_t)(n_steps - k) * step, (k == 0 || k == n_steps) ? 0.5 : 1.0, (double)step / 1e9, raw.data(),
                                raw.data() + n, n);
    const float v[4] = {e.x, e.y, e.z, e.w};
    std::fwrite(v, 4, 4, out);
  }
  std::fclose(out);
  return 0;
}

int main(int argc, char** argv) {
  using namespace wx;
  if (argc == 7 && std::string(argv[1]) == "--table") return write_table(argv);

  // the calendar against the C library's, 1678 .. 2262
  for (int i = 0; i < 200000; ++i) {
    const int64_t ns = (int64_t)(rng() % 18400000000000000000ull - 9200000000000000000ull);
    int64_t sec = ns / 1000000000;
    if (sec * 1000000000 > ns) --sec;
    const time_t tsec = (time_t)sec;
    std::tm tm;
    EXPECT(gmtime_r(&tsec, &tm));
    const TisrDate d = tisr_civil(ns);
    EXPECT(d.year == tm.tm_year + 1900 && d.doy == tm.tm_yday + 1);
    EXPECT(d.leap == ((d.year % 4 == 0 && d.year % 100 != 0) || d.year % 400 == 0));
    EXPECT(d.ns_of_day == ((int64_t)tm.tm_hour * 3600 + tm.tm_min * 60 + tm.tm_sec) * 1000000000 + (ns - sec * 1000000000));
  }
  EXPECT(tisr_days32(946728000000000000ll) == 0.f && tisr_days32(946663200000000000ll) == -0.75f);

  // a TSI table like the CMIP6 one
  std::vector<float> tsi_t, tsi_v;
  for (int y = 1850; y < 2300; ++y) { tsi_t.push_back(y + 0.5f); tsi_v.push_back(1360.5f + 0.6f * std::sin(0.571f * y)); }
  EXPECT(tisr_tsi(1850.25f, tsi_t.data(), tsi_v.data(), 450) == tsi_v[0] + (1850.25f - 1850.5f) / 1.0f * (tsi_v[1] - tsi_v[0]));   // extrapolated
  EXPECT(tisr_tsi(2299.75f, tsi_t.data(), tsi_v.data(), 450) == tsi_v[448] + 1.25f * (tsi_v[449] - tsi_v[448]));
  EXPECT(tisr_tsi(2000.5f, tsi_t.data(), tsi_v.data(), 450) == tsi_v[149] + 1.0f * (tsi_v[150] - tsi_v[149]));      // left: (1999.5, 2000.5]

  // what the create and compute calls refuse
  const float two[2] = {1.f, 2.f}, down[2] = {2.f, 2.f}, nanv[2] = {1.f, NAN};
  EXPECT(tisr_check_create(1, 2, two, two, 2, two, two).empty());
  EXPECT(tisr_check_create(1, 2, nullptr, two, 2, two, two) == "null argument");
  EXPECT(tisr_check_create(0, 2, two, two, 2, two, two).rfind("ny and nx must be", 0) == 0);
  EXPECT(tisr_check_create(65536, 65536, two, two, 2, two, two).rfind("ny and nx must be", 0) == 0);
  EXPECT(tisr_check_create(1, 2, two, two, 1, two, two) == "the TSI table needs at least two entries, got 1");
  EXPECT(tisr_check_create(1, 2, two, two, 2, down, two) == "the TSI times must ascend, entry 1 does not");
  EXPECT(tisr_check_create(1, 2, two, two, 2, two, nanv).rfind("the TSI table must be finite", 0) == 0);
  EXPECT(tisr_check_create(1, 2, two, nanv, 2, two, two) == "latitude and longitude must be finite, point 1 is not");
  const int64_t t2021 = 1622527200000000000ll, hour = 3600000000000ll;       // 2021-06-01 06:00
  float sink = 0.f;
  EXPECT(tisr_check_compute(1, &t2021, hour, 360, &sink, 7, 7, 1850, 2299).empty());
  EXPECT(tisr_check_compute(1, nullptr, hour, 360, &sink, 7, 7, 1850, 2299) == "null argument");
  EXPECT(tisr_check_compute(1, &t2021, hour, 360, nullptr, 7, 7, 1850, 2299) == "null argument");
  EXPECT(tisr_check_compute(0, &t2021, hour, 360, &sink, 7, 7, 1850, 2299) == "n_times must be >= 1, got 0");
  EXPECT(tisr_check_compute(1, &t2021, hour, 0, &sink, 7, 7, 1850, 2299) == "n_steps must be 1 .. 2^22 - 1, got 0");
  EXPECT(tisr_check_compute(1, &t2021, 0, 360, &sink, 7, 7, 1850, 2299) == "period_ns must be >= 1, got 0");
  EXPECT(tisr_check_compute(1, &t2021, 359, 360, &sink, 7, 7, 1850, 2299).rfind("a period of 359 ns holds no 360 steps", 0) == 0);
  EXPECT(tisr_check_compute(1, &t2021, hour, 360, &sink, 6, 7, 1850, 2299) == "plane_stride must be >= ny * nx = 7, got 6");
  EXPECT(tisr_check_compute(1, &t2021, hour, 360, &sink, 7, 7, 1850, 2020).rfind("a sub-step of target time 0 lies in the year 2021", 0) == 0);
  EXPECT(tisr_check_compute(1, &t2021, hour, 360, &sink, 7, 7, 2022, 2299).rfind("a sub-step of target time 0 lies in the year 2021", 0) == 0);
  const int64_t low = INT64_MIN + 5;
  EXPECT(tisr_check_compute(1, &low, hour, 360, &sink, 7, 7, 1850, 2299).rfind("the window of target time 0 leaves", 0) == 0);

  // both kernels' indexing over exactly-sized arrays: point counts around the workgroup's 512, step counts around the chunk's 256,
  // target times around the 4 of a workgroup and the 64 of a launch, plane strides with gaps
  struct Shape { int ny, nx, n_steps, n_times; int64_t gap; };
  const Shape shapes[] = {{1, 1, 1, 1, 0}, {19, 37, 255, 3, 5}, {16, 32, 256, 4, 0}, {3, 171, 257, 5, 1}, {23, 45, 513, 2, 100}, {5, 3, 7, 65, 0},
                          {1, 129, 2, 130, 3}};
  for (const Shape& s : shapes) {
    const int64_t npts = (int64_t)s.ny * s.nx, stride = npts + s.gap;
    std::vector<float> lat(npts), lon(npts), a, b, c;
    for (int64_t p = 0; p < npts; ++p) {
      lat[p] = (float)((double)(rng() % 1800001) / 10000.0 - 90.0);
      lon[p] = (float)((double)(rng() % 3600000) / 10000.0);
    }
    lat[0] = 90.f;
    lat[npts - 1] = -90.f;
    tisr_point_terms(npts, lat.data(), lon.data(), a, b, c);
    EXPECT((int64_t)a.size() == npts && (int64_t)b.size() == npts && (int64_t)c.size() == npts);
    std::vector<int64_t> t_end(s.n_times);
    for (int i = 0; i < s.n_times; ++i) t_end[i] = 788918400000000000ll + (int64_t)(rng() % 1200000000ull) * 1000000000ll;   // 1995 .. 2033
    const int64_t period = (1 + (int64_t)(rng() % 6)) * hour;
    EXPECT(tisr_check_compute(s.n_times, t_end.data(), period, s.n_steps, &sink, stride, npts, 1850, 2299).empty());
    std::vector<float> dst((size_t)((int64_t)(s.n_times - 1) * stride + npts), -7777.25f);
    replay(npts, a, b, c, tsi_t, tsi_v, t_end, period, s.n_steps, dst, stride);
    double worst = 0.0, top = 0.0;
    for (int i = 0; i < s.n_times; ++i) {
      for (int64_t p = 0; p < npts; ++p) {
        const double want = direct(lat[p], lon[p], t_end[i], period, s.n_steps, tsi_t, tsi_v);
        worst = std::max(worst, std::fabs((double)dst[(int64_t)i * stride + p] - want));
        top = std::max(top, want);
      }
      if (i + 1 < s.n_times)
        for (int64_t p = npts; p < stride; ++p) EXPECT(dst[(int64_t)i * stride + p] == -7777.25f);       // the gap between two planes
    }
    std::printf("%2d x %3d, n_steps %3d, %3d times, gap %3lld: max |replay - direct fp64| %.3e of the maximum %.3e\n", s.ny, s.nx, s.n_steps,
                s.n_times, (long long)s.gap, top > 0 ? worst / top : 0.0, top);
    EXPECT((npts == 1 || top > 1.0e6) && worst <= 5.0e-7 * top);
  }
  std::printf("tisr_host_check: ok\n");
  return 0;
}

// Stand-alone host check of the two host-only helpers of csrc/wx_reduce.h -- row_tiles (the row tiling the metrics and ensemble
// kernels index by) and grid_check (what wx_metrics_create and wx_ensemble_create refuse) -- meant for AddressSanitizer / UBSan.
// It calls no HIP function, so it runs on a machine without a GPU:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/reduce_host_check.hip -o reduce_host_check && ./reduce_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../miles-credit_amd/csrc/wx_reduce.h"

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

// rows of the last block
static int last_rows(const wx::RowTiles& g) { return g.H - (g.row_blocks - 1) * g.rows; }

int main() {
  using namespace wx;
  // ---- row_tiles
  {
    const RowTiles g = row_tiles(1, 1);
    EXPECT(g.H == 1 && g.W == 1 && g.rows == 1 && g.row_blocks == 1);
  }
  {
    const RowTiles g = row_tiles(33, 67);
    EXPECT(g.H == 33 && g.W == 67 && g.rows == 8 && g.row_blocks == 5 && last_rows(g) == 1);
  }
  {
    const RowTiles g = row_tiles(721, 1440);      // 8192 / 1440 = 5 rows
    EXPECT(g.rows == 5 && g.row_blocks == 145 && last_rows(g) == 1);
  }
  EXPECT(row_tiles(721, 9000).rows == 1 && row_tiles(721, 9000).row_blocks == 721);      // a row longer than a tile: 1, not 0
  EXPECT(row_tiles(3, 19).rows == 3 && row_tiles(3, 19).row_blocks == 1);
  EXPECT(row_tiles(521, 4).rows == 8 && row_tiles(521, 4).row_blocks == 66 && last_rows(row_tiles(521, 4)) == 1);
  EXPECT(row_tiles(8, 1024).rows == 8 && row_tiles(8, 1025).rows == 7);                  // rows * W stays within kTileElems
  for (int H : {1, 2, 7, 8, 9, 33, 721})
    for (int W : {1, 4, 67, 1024, 1440, 8192, 8193}) {
      const RowTiles g = row_tiles(H, W);
      EXPECT(g.rows >= 1 && g.rows <= kTileRows && g.rows <= H && (g.rows == 1 || (int64_t)g.rows * W <= kTileElems));
      EXPECT(last_rows(g) >= 1 && last_rows(g) <= g.rows);
    }
  // ---- grid_check: an exactly-sized heap array, so a read past the last row is caught
  {
    std::vector<float> w(33, 1.0f);
    EXPECT(grid_check(33, 67, w.data()).empty());
    EXPECT(grid_check(33, 67, nullptr).empty());
    EXPECT(grid_check(1, 2147483647, nullptr).empty());
    EXPECT(grid_check(65536, 32768, nullptr) == "bad geometry");      // 2^31
    EXPECT(grid_check(46341, 46341, nullptr) == "bad geometry");
    EXPECT(grid_check(0, 67, w.data()) == "bad geometry" && grid_check(33, 0, nullptr) == "bad geometry");
    EXPECT(grid_check(-1, 67, nullptr) == "bad geometry");
    w[32] = NAN;
    EXPECT(grid_check(33, 67, w.data()) == "non-finite latitude weight at row 32");
    w[5] = INFINITY;
    EXPECT(grid_check(33, 67, w.data()) == "non-finite latitude weight at row 5");
    EXPECT(grid_check(5, 67, w.data()).empty());      // only the grid's rows are read
  }
  std::puts("reduce host check ok");
  return 0;
}

// Horizontal regridding of the gen-2 pre-block chain on the device: an ESMF sparse weight matrix applied to every plane of the listed
// variables,
//   credit/preblock/regrid.py:123-128   W = sparse_coo_tensor([row, col], S, (n_b, n_a)).coalesce()
//   credit/preblock/regrid.py:166-167   y_flat = sparse.mm(W, x.reshape(-1, n_a).T).T
// as  y[p, r] = sum_j S[r, j] x[p, col[r, j]]  in fp32; p runs over the planes (all leading dimensions of a variable, flattened), r
// over the n_b destination points.  The reference transposes the batch twice around a CSR product; here x is read where it lies,
// [planes][n_a], and y is written [planes][n_b]: nothing is transposed, staged or written twice.
//
// Device format, built once per handle on the host from coalesced CSR (RegridPlan): sliced ELL with a slice height of one wave.
// Entry j of row r sits at slice_base[r / 64] + j * 64 + (r % 64), so the 64 lanes of a wave read 64 adjacent col words and 64
// adjacent val words per step (one-thread-per-row CSR reads 64 scattered words).  A slice is padded to its longest short row; rows
// are not reordered.  row_len[r] bounds the loop and padding is never multiplied: 0 * NaN would put a masked source point (SST over
// land) into rows that do not reference it.
// Short rows (regrid_short_kernel): one thread per destination point, 256 per workgroup.  A thread walks its row once per group of
// up to kRegridPlanes = 8 planes with the accumulators in registers: a col / val word is loaded once and used for every plane of the
// group, each term is one fmaf, in stored order.  Stores are coalesced, y[p * n_b + r].  The gathers x[p * n_a + col] are as
// coalesced as the weights make them: neighbouring destination points read neighbouring source points.
// Long rows (regrid_long_kernel): a row with more than kRegridLongRow = 64 coalesced entries (a polar destination cell, a coarse
// conservative target) would hold a whole slice to its length.  It gets no entries in its slice (row_len = -1: the short kernel
// neither walks nor stores it) and goes on a list; one wave takes one listed row, lane l the entries l, l + 64, ... of the row's
// contiguous CSR segment, a fixed-order butterfly sums the 64 partial sums and lane 0 stores.  64 is structural, not tuned: above
// one wave's width every lane has work in the first pass.  Second launch, made only when the list is not empty.
// A row without entries stores 0.0f: output buffers arrive uninitialised.
// One call takes up to kRegridMaxVars = 32 variables in one launch: (source pointer, batch stride, planes per batch item, batch,
// destination pointer) per variable, and the per-variable prefix of plane groups in the kernel argument; blockIdx.y selects the
// variable and the group.  A plane's result depends on its own values and on the row's stored order alone, so every grouping of
// variables and planes gives the same bits per plane.
// Ranges: n_a, n_b, the entry count and a variable's plane count are each below 2^31; offsets are 64-bit.  Every column index is
// checked against [0, n_a) on the host before anything is uploaded (regrid_check_create): a bad index would be an out-of-bounds read.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "wx_common.h"

namespace wx {

constexpr int kRegridPlanes = 8;
constexpr int kRegridLongRow = 64;
constexpr int kRegridMaxVars = 32;
constexpr int kRegridSlice = 64;
constexpr int64_t kRegridLimit = 2147483647LL;   // n_a, n_b, entries, planes: each <= 2^31 - 1

struct RegridVars {
  const float* src[kRegridMaxVars];   // plane p = b * ppi + q of variable v at src[v] + b * bstride[v] + q * n_a: [n_a]
  float* dst[kRegridMaxVars];         // [planes][n_b]
  int64_t bstride[kRegridMaxVars];    // in floats
  int ppi[kRegridMaxVars];            // planes per batch item
  int planes[kRegridMaxVars];         // batch * ppi
  int group0[kRegridMaxVars + 1];     // prefix of plane groups: variable v owns the groups group0[v] .. group0[v + 1] - 1
  int n_vars;
};

struct RegridMatrix {
  int64_t n_a, n_b;
  const int64_t* slice_base;   // [ceil(n_b / 64) + 1]
  const int* row_len;          // [n_b]; -1: the row is on the long list
  const int* ell_col;          // sliced ELL, padded
  const float* ell_val;
  int n_long;
  const int* long_row;         // [n_long]
  const int64_t* long_ptr;     // [n_long + 1] into long_col / long_val
  const int* long_col;
  const float* long_val;
};

// ---- host-only helpers (no HIP call) ---------------------------------------------------------------------------------------------
// "" or the reason wx_regrid_create refuses.  Nothing is read before the test that makes reading it safe.
inline std::string regrid_check_create(int64_t n_a, int64_t n_b, const int64_t* row_ptr, const int* col, const float* val) {
  if (!row_ptr || !col || !val) return "null weight array";
  if (n_a < 1 || n_a > kRegridLimit) return "n_a must be 1 .. 2^31 - 1, got " + std::to_string(n_a);
  if (n_b < 1 || n_b > kRegridLimit) return "n_b must be 1 .. 2^31 - 1, got " + std::to_string(n_b);
  if (row_ptr[0] != 0) return "row_ptr must start at 0, got " + std::to_string(row_ptr[0]);
  for (int64_t r = 0; r < n_b; ++r)
    if (row_ptr[r + 1] < row_ptr[r]) return "row_ptr decreases at row " + std::to_string(r);
  const int64_t nnz = row_ptr[n_b];
  if (nnz > kRegridLimit) return "the entry count must stay below 2^31, got " + std::to_string(nnz);
  for (int64_t e = 0; e < nnz; ++e)
    if (col[e] < 0 || col[e] >= n_a)
      return "column index " + std::to_string(col[e]) + " at entry " + std::to_string(e) + " lies outside [0, n_a = " + std::to_string(n_a) + ")";
  return "";
}

// The device format from coalesced CSR (checked by regrid_check_create).
struct RegridPlan {
  std::vector<int64_t> slice_base;
  std::vector<int> row_len;
  std::vector<int> ell_col;
  std::vector<float> ell_val;
  std::vector<int> long_row;
  std::vector<int64_t> long_ptr;
  std::vector<int> long_col;
  std::vector<float> long_val;
};
inline RegridPlan regrid_plan(int64_t n_b, const int64_t* row_ptr, const int* col, const float* val) {
  RegridPlan p;
  const int64_t n_slices = (n_b + kRegridSlice - 1) / kRegridSlice;
  p.slice_base.assign(n_slices + 1, 0);
  p.row_len.resize(n_b);
  p.long_ptr.push_back(0);
  for (int64_t r = 0; r < n_b; ++r) {
    const int64_t len = row_ptr[r + 1] - row_ptr[r];
    if (len > kRegridLongRow) {
      p.row_len[r] = -1;
      p.long_row.push_back((int)r);
      p.long_col.insert(p.long_col.end(), col + row_ptr[r], col + row_ptr[r + 1]);
      p.long_val.insert(p.long_val.end(), val + row_ptr[r], val + row_ptr[r + 1]);
      p.long_ptr.push_back((int64_t)p.long_col.size());
    } else {
      p.row_len[r] = (int)len;
    }
  }
  for (int64_t s = 0; s < n_slices; ++s) {
    int width = 0;
    for (int64_t r = s * kRegridSlice; r < std::min(n_b, (s + 1) * kRegridSlice); ++r) width = std::max(width, p.row_len[r]);
    p.slice_base[s + 1] = p.slice_base[s] + (int64_t)width * kRegridSlice;
  }
  p.ell_col.assign((size_t)p.slice_base[n_slices], 0);      // padding: column 0, weight 0, never read (row_len bounds the loop)
  p.ell_val.assign((size_t)p.slice_base[n_slices], 0.f);
  for (int64_t r = 0; r < n_b; ++r)
    for (int j = 0; j < p.row_len[r]; ++j) {
      const int64_t at = p.slice_base[r / kRegridSlice] + (int64_t)j * kRegridSlice + r % kRegridSlice;
      p.ell_col[at] = col[row_ptr[r] + j];
      p.ell_val[at] = val[row_ptr[r] + j];
    }
  return p;
}

// ---- device side -------------------------------------------------------------------------------------------------------------------
// The variable and the planes that plane group `g` of the launch stands for (wave-uniform) -> number of planes, 1 .. kRegridPlanes.
__device__ __forceinline__ int regrid_group(const RegridVars& a, int g, int64_t n_a, int64_t n_b, const float* (&x)[kRegridPlanes],
                                            float* (&y)[kRegridPlanes]) {
  int v = 0;
  while (v + 1 < a.n_vars && g >= a.group0[v + 1]) ++v;
  const int p0 = (g - a.group0[v]) * kRegridPlanes;
  const int np = min(kRegridPlanes, a.planes[v] - p0);
#pragma unroll
  for (int k = 0; k < kRegridPlanes; ++k) {
    const int p = p0 + min(k, np - 1);            // a tail group's unused slots repeat its last plane: never loaded, never stored
    const int b = p / a.ppi[v], q = p - b * a.ppi[v];
    x[k] = a.src[v] + (int64_t)b * a.bstride[v] + (int64_t)q * n_a;
    y[k] = a.dst[v] + (int64_t)p * n_b;
  }
  return np;
}

// grid = (ceil(n_b / 256), plane groups of this launch); g_first: the first plane group of this launch
__global__ __launch_bounds__(256) void regrid_short_kernel(const RegridVars a, const RegridMatrix m, int g_first) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= m.n_b) return;
  const int len = m.row_len[r];
  if (len < 0) return;                            // a long row: regrid_long_kernel stores it
  const float* x[kRegridPlanes];
  float* y[kRegridPlanes];
  const int np = regrid_group(a, g_first + (int)blockIdx.y, m.n_a, m.n_b, x, y);
  float acc[kRegridPlanes];
#pragma unroll
  for (int k = 0; k < kRegridPlanes; ++k) acc[k] = 0.f;
  const int64_t base = m.slice_base[r / kRegridSlice] + (r % kRegridSlice);
  for (int j = 0; j < len; ++j) {
    const int64_t at = base + (int64_t)j * kRegridSlice;
    const int64_t c = m.ell_col[at];
    const float w = m.ell_val[at];
#pragma unroll
    for (int k = 0; k < kRegridPlanes; ++k)
      if (k < np) acc[k] = fmaf(w, x[k][c], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < kRegridPlanes; ++k)
    if (k < np) y[k][r] = acc[k];
}

// grid = (ceil(n_long / 4), plane groups of this launch): one wave per long row
__global__ __launch_bounds__(256) void regrid_long_kernel(const RegridVars a, const RegridMatrix m, int g_first) {
  const int i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (i >= m.n_long) return;                      // wave-uniform
  const int lane = threadIdx.x & 63;
  const float* x[kRegridPlanes];
  float* y[kRegridPlanes];
  const int np = regrid_group(a, g_first + (int)blockIdx.y, m.n_a, m.n_b, x, y);
  float acc[kRegridPlanes];
#pragma unroll
  for (int k = 0; k < kRegridPlanes; ++k) acc[k] = 0.f;
  const int64_t end = m.long_ptr[i + 1];
  for (int64_t e = m.long_ptr[i] + lane; e < end; e += 64) {
    const int64_t c = m.long_col[e];
    const float w = m.long_val[e];
#pragma unroll
    for (int k = 0; k < kRegridPlanes; ++k)
      if (k < np) acc[k] = fmaf(w, x[k][c], acc[k]);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)         // butterfly: the same tree in every lane, whatever the grouping
#pragma unroll
    for (int k = 0; k < kRegridPlanes; ++k) acc[k] += __shfl_xor(acc[k], off, 64);
  if (lane == 0) {
    const int64_t r = m.long_row[i];
#pragma unroll
    for (int k = 0; k < kRegridPlanes; ++k)
      if (k < np) y[k][r] = acc[k];
  }
}

class Regrid {
 public:
  Regrid(int64_t n_a_, int64_t n_b_, const int64_t* row_ptr, const int* col, const float* val, int dev)
      : n_a(n_a_), n_b(n_b_), device(dev), mem(dev) {
    const RegridPlan p = regrid_plan(n_b, row_ptr, col, val);
    n_long = (int)p.long_row.size();
    WX_HIP(hipSetDevice(device));
    auto up = [&](const auto& v) {       // an empty array still gets an address of its own (never read)
      using T = typename std::decay<decltype(v)>::type::value_type;
      const T none = T();
      return v.empty() ? mem.upload(&none, 1) : mem.upload(v.data(), v.size());
    };
    slice_base = up(p.slice_base); row_len = up(p.row_len); ell_col = up(p.ell_col); ell_val = up(p.ell_val);
    long_row = up(p.long_row); long_ptr = up(p.long_ptr); long_col = up(p.long_col); long_val = up(p.long_val);
  }
  void apply(int n_vars, const float* const* src, const int64_t* bstride, const int* ppi, int batch, float* const* dst, hipStream_t stream) {
    if (n_vars < 1 || n_vars > kRegridMaxVars) throw std::runtime_error("wx_regrid_apply: 1.." + std::to_string(kRegridMaxVars) + " variables");
    if (batch < 1) throw std::runtime_error("wx_regrid_apply: batch must be >= 1");
    RegridVars a;
    std::memset(&a, 0, sizeof(a));
    a.n_vars = n_vars;
    int64_t groups = 0;
    for (int v = 0; v < n_vars; ++v) {
      if (!src[v] || !dst[v]) throw std::runtime_error("wx_regrid_apply: null tensor pointer");
      if (ppi[v] < 1) throw std::runtime_error("wx_regrid_apply: planes_per_item must be >= 1");
      if (batch > 1 && bstride[v] < 0) throw std::runtime_error("wx_regrid_apply: negative batch stride");
      const int64_t planes = (int64_t)batch * ppi[v];
      if (planes > kRegridLimit) throw std::runtime_error("wx_regrid_apply: batch * planes_per_item exceeds 2^31 - 1 planes");
      a.src[v] = src[v]; a.dst[v] = dst[v];
      a.bstride[v] = batch > 1 ? bstride[v] : 0;
      a.ppi[v] = ppi[v]; a.planes[v] = (int)planes;
      a.group0[v] = (int)groups;
      groups += (planes + kRegridPlanes - 1) / kRegridPlanes;
      if (groups > kRegridLimit) throw std::runtime_error("wx_regrid_apply: too many planes in one call");
    }
    for (int v = n_vars; v <= kRegridMaxVars; ++v) a.group0[v] = (int)groups;
    WX_HIP(hipSetDevice(device));
    RegridMatrix m;
    m.n_a = n_a; m.n_b = n_b;
    m.slice_base = slice_base; m.row_len = row_len; m.ell_col = ell_col; m.ell_val = ell_val;
    m.n_long = n_long; m.long_row = long_row; m.long_ptr = long_ptr; m.long_col = long_col; m.long_val = long_val;
    const dim3 block(256);
    for (int64_t g = 0; g < groups; g += kMaxGridY) {          // gridDim.y holds 65535 groups (524 280 planes): more take a further launch
      const unsigned gy = (unsigned)std::min<int64_t>(kMaxGridY, groups - g);
      hipLaunchKernelGGL(regrid_short_kernel, dim3((unsigned)((n_b + 255) / 256), gy), block, 0, stream, a, m, (int)g);
      if (n_long > 0) hipLaunchKernelGGL(regrid_long_kernel, dim3((unsigned)((n_long + 3) / 4), gy), block, 0, stream, a, m, (int)g);
    }
    WX_HIP(hipGetLastError());
  }

 private:
  static constexpr int64_t kMaxGridY = 65535;
  int64_t n_a, n_b;
  int device, n_long = 0;
  DeviceArena mem;
  int64_t* slice_base = nullptr;
  int* row_len = nullptr;
  int* ell_col = nullptr;
  float* ell_val = nullptr;
  int* long_row = nullptr;
  int64_t* long_ptr = nullptr;
  int* long_col = nullptr;
  float* long_val = nullptr;
};

}  // namespace wx

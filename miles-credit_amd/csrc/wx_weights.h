// wxengine: how the weights are laid out.  The layer tables (offsets into the two device arenas) and the host-side packer that
// fills them from a loaded ModelSpec: spectral-norm and LayerNorm folds, DynamicPositionBias tables, the K-contiguous GEMM operand
// layout and every kernel-specific repack (k-blocked, LDS-patch CrossEmbed, fused FeedForward chunks).  Host arithmetic only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "wx_attn.h"
#include "wx_ff.h"
#include "wx_gemm.h"
#include "wx_options.h"
#include "wx_spec.h"

namespace wx {

struct ConvW {          // one repacked GEMM operand in the weight arena
  int64_t wt = -1;      // element offset into the T arena
  int n = 0, cin = 0, kh = 1, kw = 1;
  int64_t bias = -1;    // float-arena offsets (-1 = absent)
  int64_t colsum = -1;
  int cin_true = 0;     // unpadded channels (flop accounting)
  double flop_frac = 1.0;   // share of the dense n x kh x kw x cin products that are the model's (merged CrossEmbed: the rest multiply padded zeros)
  int64_t wt_kb = -1;   // bf16 engine, 1x1 layers with n % 256 == 0: second copy, k-blocked [cin/32][n][32] (wx_gemm_stream.h)
};
struct AttnL { ConvW qkv, vonly, out; int64_t bias_tab = -1, bias_tb = -1; int wsz = 0, kind = 0; };
struct FFL { ConvW w1, w2; int64_t pack = -1, pack_pre = -1, pack_pp = -1; const AttnL* next = nullptr; };  // pack: fused-block chunk layout (wx_ff.h), T-arena offset; pack_pre: the same preceded by the attention's Wout blocks
struct BlockL { AttnL sa; FFL sf; AttnL la; FFL lf; };
struct PatchW { int64_t wt = -1, bias = -1, wt16 = -1; int n = 0; };   // LDS-patch CrossEmbed branch (wx_embed.h); wt16: split-bf16 mode, offset in the 16-bit patch arena
struct StageL {
  std::vector<ConvW> embed; std::vector<int> embed_k; std::vector<PatchW> patch; std::vector<BlockL> blocks;
  bool ride4 = false;                            // stage 0: the k = 4 branch rides in the LDS-patch kernel's spare accumulator rows
  int64_t patch_tab = -1, patch_bias64 = -1;     // float-arena offsets of EmbedPatchParams::slot_tab / bias64
  ConvW merged;   // launch-bound maps: every CrossEmbed branch zero-padded into the largest kernel's window, one convolution of all output channels
};
struct UpL { ConvW convt, convps, sharp, upc, c1, c2; int64_t g1 = -1, b1 = -1, g2 = -1, b2 = -1; int cin = 0, cout = 0; };
struct NoiseL { int64_t w = -1, b = -1, mod = -1, nf = -1; };

// every layer of the model as offsets into the T arena (weights) and the float arena (biases, column sums, tables)
struct LayerTables {
  StageL stages[4];
  UpL ups[3];
  ConvW up4[4];      // legacy head: the ConvTranspose k4's four parity convs
  ConvW up4c;        // upsample_v_conv variant: its up_block4 conv
  ConvW ps4, fin4;   // wxformer head: sub-pixel conv (shuffled rows) and the final 3x3 conv
  int cpad4 = 0;
  NoiseL nz[6];      // float-arena offsets of the six noise layers (slots as noise_slot_on)
};

// Lives for one Engine::finalize(): run() fills `tab` in place (FFL::next points into tab.stages[s].blocks) and the host arenas,
// which the engine uploads.
template <typename T>
struct WeightPacker {
  const ModelSpec& spec;
  const wx_config& cfg;
  LayerTables& tab;
  const Options& opt;
  const bool split_mma;
  std::vector<T> wt_host;            // T arena
  std::vector<float> f_host;         // float arena
  std::vector<uint16_t> sp16_host;   // split_mma: bf16 patch weights (make_patch)
  WeightPacker(const ModelSpec& m, LayerTables& t, const Options& o, bool split) : spec(m), cfg(m.cfg), tab(t), opt(o), split_mma(split) {}

  int64_t push_f(const std::vector<float>& v) {
    // keep every float-arena block 16-byte aligned
    while (f_host.size() % 4) f_host.push_back(0.f);
    const int64_t off = (int64_t)f_host.size();
    f_host.insert(f_host.end(), v.begin(), v.end());
    // pad every block to a multiple of 128 floats: GEMM epilogues read bias/colsum as whole float4 vectors
    // for a full 128-channel tile even when the layer has fewer channels
    while ((f_host.size() - off) % 128) f_host.push_back(0.f);
    return off;
  }
  int64_t push_w(const std::vector<double>& rows, int n, int64_t k) {
    // 16-byte blocks; split-bf16 arithmetic: whole 32-float K chunks (the split arena re-encodes the arena chunk by chunk)
    while (wt_host.size() % (split_mma ? 32 : 8)) wt_host.push_back(Elem<T>::from_f(0.f));
    const int64_t off = (int64_t)wt_host.size();
    wt_host.resize(off + (int64_t)n * k);
    for (int64_t i = 0; i < (int64_t)n * k; ++i) wt_host[off + i] = Elem<T>::from_f((float)rows[i]);
    return off;
  }
  // k-blocked copy of a 1x1 layer's ROUNDED arena weights for the persistent GEMM (same values, other order): a K = 32 stage of
  // 256 output channels is then 16 contiguous KB (full cache lines per LDS-DMA piece instead of half-used ones)
  void pack_kblocked(ConvW& cw) {
    if constexpr (sizeof(T) != 2) return;
    if (!opt.use_stream || cw.kh != 1 || cw.kw != 1 || cw.n % 128 != 0 || cw.cin % 32 != 0 || cw.cin < 512) return;
    while (wt_host.size() % 8) wt_host.push_back(Elem<T>::from_f(0.f));
    const int64_t off = (int64_t)wt_host.size();
    wt_host.resize(off + (int64_t)cw.n * cw.cin);
    for (int n = 0; n < cw.n; ++n)
      for (int k = 0; k < cw.cin; ++k)
        wt_host[off + ((int64_t)(k / 32) * cw.n + n) * 32 + k % 32] = wt_host[cw.wt + (int64_t)n * cw.cin + k];
    cw.wt_kb = off;
  }
  // Conv2d weight W[n][c][kh][kw] (rows [r0, r1)) -> [n][kh][kw][cpad]; optional LayerNorm fold (g, b per input channel)
  // row_src (optional): output row o takes reference row row_src[o] (-1 = all-zero row) instead of r0 + o
  // lead_rows / lead_scale: output rows [0, lead_rows) (weights and bias) are multiplied by lead_scale before rounding -- the
  // attention's 1/sqrt(d) (x log2 e) folded into the q rows of to_qkv, so the score MFMA needs no scaling afterwards
  ConvW make_conv(const std::string& p, int r0, int r1, int cin, int cpad, int kh, int kw, bool has_bias,
                  const float* ln_g, const float* ln_b, const std::vector<int>* row_src = nullptr, int lead_rows = 0,
                  double lead_scale = 1.0) {
    const std::vector<double> w = spec.folded(p, false);
    const int n = row_src ? (int)row_src->size() : r1 - r0;
    const int64_t k = (int64_t)kh * kw * cpad;
    std::vector<double> rows((size_t)n * k, 0.0);
    std::vector<float> bias(n, 0.f), colsum;
    const HostTensor* bt = has_bias ? &spec.need(p + ".bias") : nullptr;
    for (int o = 0; o < n; ++o) {
      double tshift = 0.0;
      const int ro = row_src ? (*row_src)[o] : r0 + o;
      if (ro < 0) continue;  // zero row (channel padding)
      for (int c = 0; c < cin; ++c)
        for (int y = 0; y < kh; ++y)
          for (int x = 0; x < kw; ++x) {
            double v = w[(((int64_t)ro * cin + c) * kh + y) * kw + x] * (o < lead_rows ? lead_scale : 1.0);
            if (ln_b) tshift += v * ln_b[c];
            if (ln_g) v *= ln_g[c];
            rows[(size_t)o * k + ((int64_t)y * kw + x) * cpad + c] = v;
          }
      bias[o] = (float)(tshift + (bt ? (double)bt->data[ro] * (o < lead_rows ? lead_scale : 1.0) : 0.0));
    }
    ConvW cw;
    cw.n = n; cw.cin = cpad; cw.cin_true = cin; cw.kh = kh; cw.kw = kw;
    cw.wt = push_w(rows, n, k);
    if (ln_g) {  // colsum over the ROUNDED weights so that acc - mean*colsum == sum((x-mean)*w) exactly
      colsum.resize(n);
      for (int o = 0; o < n; ++o) {
        double s = 0.0;
        for (int64_t i = 0; i < k; ++i) s += (double)Elem<T>::to_f(wt_host[cw.wt + (int64_t)o * k + i]);
        colsum[o] = (float)s;
      }
      cw.colsum = push_f(colsum);
    }
    if (has_bias || ln_b) cw.bias = push_f(bias);
    return cw;
  }
  // All branches of one CrossEmbed (crossformer.py:128-152: kernel k, stride s, padding (k - s) / 2 -- every branch is centred on the same
  // window) as ONE convolution with the largest kernel: branch b's taps sit at offset (kmax - k_b) / 2 inside it, zeros around them
  // (exact: the added products are 0 * x).  Output channels in the reference's concatenation order.
  ConvW make_embed_merged(int s, const std::vector<int>& ks, const std::vector<int>& cos, int cin, int cpad) {
    const int kmax = ks.back();
    int n = 0;
    for (int co : cos) n += co;
    const int64_t k = (int64_t)kmax * kmax * cpad;
    std::vector<double> rows((size_t)n * k, 0.0);
    std::vector<float> bias(n, 0.f);
    int o0 = 0;
    for (size_t b = 0; b < ks.size(); ++b) {
      const std::string bp = spec.embed_key(s, (int)b);
      const std::vector<double> w = spec.folded(bp, false);
      const HostTensor& bt = spec.need(bp + ".bias");
      const int kb = ks[b], d = (kmax - kb) / 2;
      for (int o = 0; o < cos[b]; ++o) {
        for (int c = 0; c < cin; ++c)
          for (int y = 0; y < kb; ++y)
            for (int x = 0; x < kb; ++x)
              rows[(size_t)(o0 + o) * k + ((int64_t)(y + d) * kmax + (x + d)) * cpad + c] = w[(((int64_t)o * cin + c) * kb + y) * kb + x];
        bias[o0 + o] = bt.data[o];
      }
      o0 += cos[b];
    }
    ConvW cw;
    cw.n = n; cw.cin = cpad; cw.cin_true = cin; cw.kh = kmax; cw.kw = kmax;
    double real = 0.0;
    for (size_t b = 0; b < ks.size(); ++b) real += (double)cos[b] * ks[b] * ks[b];
    cw.flop_frac = real / ((double)n * kmax * kmax);
    cw.wt = push_w(rows, n, k);
    cw.bias = push_f(bias);
    return cw;
  }
  // Stage-0 branch for embed_patch_kernel: [chunk][ky][kx/4][n-frag][tap g][out 16][CC channels]
  // `extra`: channels [x0, x0 + xn) of the smaller kernel `xkey` (size xk) as accumulator rows n .. n + xn - 1, their taps zero-padded
  // into the middle of this k x k window (same centre: crossformer.py:128-152 padding (k - stride) / 2) -- see EmbedPatchParams::slot_tab
  PatchW make_patch(const std::string& p, int n, int cin, int cpad, int k, const std::string& xkey = "", int xk = 0, int x0 = 0, int xn = 0) {
    PatchW pw;
    pw.n = n;
    if (split_mma) {
      // split-bf16 mode: the bf16 instantiation of the patch kernel over the K-concatenated operand pair -- weights [W_hi | W_hi | W_lo]
      // against planes [x_hi | x_lo | x_hi] (pack_input): 3 x cpad / 8 chunks of the bf16 layout, in their own 16-bit arena
      const std::vector<double> r8 = patch_rows(p, n, cin, cpad, k, 8, xkey, xk, x0, xn);
      while (sp16_host.size() % 8) sp16_host.push_back(0);
      pw.wt16 = (int64_t)sp16_host.size();
      sp16_host.resize(sp16_host.size() + 3 * r8.size());
      uint16_t* d = sp16_host.data() + pw.wt16;
      for (size_t i = 0; i < r8.size(); ++i) {
        const float w = (float)r8[i];
        const bf16_t hi = f2bf(w), lo = f2bf(w - bf2f(hi));
        d[i] = hi; d[r8.size() + i] = hi; d[2 * r8.size() + i] = lo;
      }
    }
    const std::vector<double> rows = patch_rows(p, n, cin, cpad, k, 16 / (int)sizeof(T), xkey, xk, x0, xn);
    pw.wt = push_w(rows, 1, (int64_t)rows.size());
    return pw;
  }
  std::vector<double> patch_rows(const std::string& p, int n, int cin, int cpad, int k, int CC, const std::string& xkey, int xk, int x0, int xn) {
    const std::vector<double> w = spec.folded(p, false);
    const int chunks = cpad / CC, k4n = k / 4, nfr = (k == 8) ? 2 : 1;  // fragment counts the kernel is built for
    std::vector<double> rows((size_t)chunks * k * k4n * nfr * 64 * CC, 0.0);
    auto at = [&](int ch, int ky, int kx, int o, int e) -> double& {
      return rows[(((((size_t)ch * k + ky) * k4n + kx / 4) * nfr + o / 16) * 64 + (kx % 4) * 16 + (o % 16)) * CC + e];
    };
    for (int ch = 0; ch < chunks; ++ch)
      for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx)
          for (int o = 0; o < n; ++o)
            for (int e = 0; e < CC; ++e) {
              const int c = ch * CC + e;
              if (c < cin) at(ch, ky, kx, o, e) = w[(((int64_t)o * cin + c) * k + ky) * k + kx];
            }
    if (xn > 0) {
      const std::vector<double> wx = spec.folded(xkey, false);
      const int d = (k - xk) / 2;
      for (int ch = 0; ch < chunks; ++ch)
        for (int ky = 0; ky < xk; ++ky)
          for (int kx = 0; kx < xk; ++kx)
            for (int o = 0; o < xn; ++o)
              for (int e = 0; e < CC; ++e) {
                const int c = ch * CC + e;
                if (c < cin) at(ch, ky + d, kx + d, n + o, e) = wx[(((int64_t)(x0 + o) * cin + c) * xk + ky) * xk + kx];
              }
    }
    return rows;
  }
  // ConvTranspose2d k2 s2: W[ci][co][dy][dx] -> rows n = (dy*2+dx)*cout + co, K = ci; bias expanded x4
  ConvW make_convt2(const std::string& p, int cin, int cout) {
    const std::vector<double> w = spec.folded(p, true);
    std::vector<double> rows((size_t)4 * cout * cin);
    for (int ci = 0; ci < cin; ++ci)
      for (int co = 0; co < cout; ++co)
        for (int q = 0; q < 4; ++q) rows[((size_t)q * cout + co) * cin + ci] = w[((int64_t)ci * cout + co) * 4 + q];
    const HostTensor& b = spec.need(p + ".bias");
    std::vector<float> bias(4 * cout);
    for (int q = 0; q < 4; ++q)
      for (int co = 0; co < cout; ++co) bias[q * cout + co] = b.data[co];
    ConvW cw;
    cw.n = 4 * cout; cw.cin = cin; cw.cin_true = cin;
    cw.wt = push_w(rows, 4 * cout, cin);
    cw.bias = push_f(bias);
    return cw;
  }
  // ConvTranspose2d k4 s2 p1 as four 2x2-tap parity convs: out(2y+py, 2x+px) = sum_{ty,tx} in(y-1+py+ty, x-1+px+tx) W[ci][co][3-py-2ty][3-px-2tx]
  void make_convt4(const std::string& p, int cin, int cout) {
    const std::vector<double> w = spec.folded(p, true);
    const HostTensor& b = spec.need(p + ".bias");
    for (int py = 0; py < 2; ++py)
      for (int px = 0; px < 2; ++px) {
        std::vector<double> rows((size_t)cout * 4 * cin);
        for (int co = 0; co < cout; ++co)
          for (int ty = 0; ty < 2; ++ty)
            for (int tx = 0; tx < 2; ++tx)
              for (int ci = 0; ci < cin; ++ci)
                rows[((size_t)co * 4 + ty * 2 + tx) * cin + ci] =
                    w[(((int64_t)ci * cout + co) * 4 + (3 - py - 2 * ty)) * 4 + (3 - px - 2 * tx)];
        ConvW cw;
        cw.n = cout; cw.cin = cin; cw.cin_true = cin; cw.kh = 2; cw.kw = 2;
        cw.wt = push_w(rows, cout, (int64_t)4 * cin);
        cw.bias = push_f(std::vector<float>(b.data.begin(), b.data.end()));
        tab.up4[py * 2 + px] = cw;
      }
  }
  // DynamicPositionBias (crossformer.py:158-176) evaluated on the (2w+1)^2 offsets, gathered with the
  // reference's stride-(2w-1) indices (crossformer.py:238-245, :284), padded to [NP][NP].
  int64_t make_bias_table(const std::string& p, int wsz, int dq, int64_t* tb_off = nullptr) {
    const int side = 2 * wsz + 1, npos = side * side;
    std::vector<double> w0 = spec.folded(p + ".layers.0", false), w3 = spec.folded(p + ".layers.3", false),
                        w6 = spec.folded(p + ".layers.6", false), w9 = spec.folded(p + ".layers.9", false);
    const HostTensor &b0 = spec.need(p + ".layers.0.bias"), &b3 = spec.need(p + ".layers.3.bias"), &b6 = spec.need(p + ".layers.6.bias"),
                     &b9 = spec.need(p + ".layers.9.bias");
    const HostTensor* lnw[3] = {&spec.need(p + ".layers.1.weight"), &spec.need(p + ".layers.4.weight"), &spec.need(p + ".layers.7.weight")};
    const HostTensor* lnb[3] = {&spec.need(p + ".layers.1.bias"), &spec.need(p + ".layers.4.bias"), &spec.need(p + ".layers.7.bias")};
    std::vector<double> table(npos);
    std::vector<double> h(dq), h2(dq);
    auto ln_relu = [&](std::vector<double>& v, int i) {
      double m = 0, q = 0;
      for (double x : v) m += x;
      m /= dq;
      for (double x : v) q += (x - m) * (x - m);
      q /= dq;
      const double r = 1.0 / std::sqrt(q + 1e-5);
      for (int k = 0; k < dq; ++k) {
        const double y = (v[k] - m) * r * lnw[i]->data[k] + lnb[i]->data[k];
        v[k] = y > 0 ? y : 0;
      }
    };
    for (int a = 0; a < side; ++a)
      for (int b = 0; b < side; ++b) {
        const double pr = a - wsz, pc = b - wsz;
        for (int k = 0; k < dq; ++k) h[k] = w0[2 * k] * pr + w0[2 * k + 1] * pc + b0.data[k];
        ln_relu(h, 0);
        for (int k = 0; k < dq; ++k) { double s = b3.data[k]; for (int j = 0; j < dq; ++j) s += w3[(size_t)k * dq + j] * h[j]; h2[k] = s; }
        ln_relu(h2, 1);
        for (int k = 0; k < dq; ++k) { double s = b6.data[k]; for (int j = 0; j < dq; ++j) s += w6[(size_t)k * dq + j] * h2[j]; h[k] = s; }
        ln_relu(h, 2);
        double s = b9.data[0];
        for (int j = 0; j < dq; ++j) s += w9[j] * h[j];
        table[a * side + b] = s;
      }
    // [NP][NP] table the kernel adds to the scores: padded keys (and, for packed tiles, keys of another window) get
    // -1e30; the bf16 engine exponentiates with v_exp_f32 (2^x), so its table carries the log2(e) factor
    const int N1 = wsz * wsz, G = attn_pack(wsz), N = N1 * G, NP = attn_nkf(wsz) * 16;
    const double pre = sizeof(T) == 2 ? 1.4426950408889634 : 1.0;
    std::vector<float> padded((size_t)NP * NP, 0.f);
    for (int i = 0; i < NP; ++i)
      for (int j = 0; j < NP; ++j) {
        float v;
        if (j >= N) v = -1.0e30f;
        else if (i >= N) v = 0.f;
        else if (i / N1 != j / N1) v = -1.0e30f;
        else {
          const int il = i % N1, jl = j % N1;
          const int dr = il / wsz - jl / wsz + wsz - 1, dc = il % wsz - jl % wsz + wsz - 1;
          v = (float)(pre * table[dr * (2 * wsz - 1) + dc]);
        }
        padded[(size_t)i * NP + j] = v;
      }
    if (tb_off) {  // the generating table itself (flat, first (2w-1)^2 entries are the ones the reference's indices reach)
      std::vector<float> tb((size_t)(2 * wsz - 1) * (2 * wsz - 1));
      for (size_t i = 0; i < tb.size(); ++i) tb[i] = (float)(pre * table[i]);
      *tb_off = push_f(tb);
    }
    return push_f(padded);
  }
  AttnL make_attn(const std::string& p, int c, int wsz, int kind) {
    AttnL a;
    a.wsz = wsz; a.kind = kind;
    const HostTensor &g = spec.need(p + ".norm.g"), &b = spec.need(p + ".norm.b");
    if (wsz == 1) {
      // one token per window: softmax == 1, attention output == v (crossformer.py:286-295) -> only the v rows
      a.vonly = make_conv(p + ".to_qkv", 2 * c, 3 * c, c, c, 1, 1, false, g.data.data(), b.data.data());
      pack_kblocked(a.vonly);
    } else {
      // bf16 engine: softmax scale (and the log2 e of its exp2) lives in the q rows; the fp32 engine multiplies the scores instead
      a.qkv = make_conv(p + ".to_qkv", 0, 3 * c, c, c, 1, 1, false, g.data.data(), b.data.data(), nullptr,
                        sizeof(T) == 2 ? c : 0, 1.4426950408889634 / std::sqrt((double)cfg.dim_head));
      pack_kblocked(a.qkv);
      a.bias_tab = make_bias_table(p + ".dpb", wsz, c / 4, &a.bias_tb);
    }
    a.out = make_conv(p + ".to_out", 0, c, c, c, 1, 1, true, nullptr, nullptr);
    pack_kblocked(a.out);
    return a;
  }
  // chunk blocks for ff_fused_kernel, built from the ROUNDED arena weights of w1 / w2 (same values as the unfused path)
  int64_t pack_ff(const FFL& f, int c, int hidden, const ConvW* wout = nullptr, const ConvW* wqkv = nullptr) {
    while (wt_host.size() % 8) wt_host.push_back(Elem<T>::from_f(0.f));
    const int64_t off = (int64_t)wt_host.size();
    const int nch = hidden / 32, npre = wout ? c / 64 : 0, npost = wqkv ? 3 * c / 64 : 0;
    const int64_t cb = 64 * (int64_t)c;  // elements per chunk block (128*C bytes of bf16)
    wt_host.resize(off + (npre + nch + npost) * cb);
    for (int i = 0; i < npost; ++i)      // Wqkv' rows [64 i, 64 i + 64), k order permuted like W1 (the input sits in accumulator layout)
      for (int r = 0; r < 64; ++r)
        for (int sl = 0; sl < c / 8; ++sl)
          for (int j = 0; j < 8; ++j)
            wt_host[off + (npre + nch + i) * cb + (int64_t)r * c + (sl ^ (r & 15)) * 8 + j] =
                wt_host[wqkv->wt + (int64_t)(i * 64 + r) * c + 32 * (sl / 4) + ff_perm(sl % 4, j)];
    for (int i = 0; i < npre; ++i)       // Wout rows [64 i, 64 i + 64), natural k order, 16-byte slots XOR-swizzled by row
      for (int r = 0; r < 64; ++r)
        for (int sl = 0; sl < c / 8; ++sl)
          for (int j = 0; j < 8; ++j)
            wt_host[off + i * cb + (int64_t)r * c + (sl ^ (r & 15)) * 8 + j] = wt_host[wout->wt + (int64_t)(i * 64 + r) * c + sl * 8 + j];
    for (int ch = 0; ch < nch; ++ch) {
      const int64_t base = off + (npre + ch) * cb;
      for (int r = 0; r < 32; ++r)
        for (int sl = 0; sl < c / 8; ++sl) {
          const int ks = sl / 4, g = sl % 4, phys = sl ^ (r & (c / 8 < 16 ? c / 8 - 1 : 15));   // (C = 64: 8 slots per row)
          for (int j = 0; j < 8; ++j)
            wt_host[base + (int64_t)r * c + phys * 8 + j] = wt_host[f.w1.wt + (int64_t)(ch * 32 + r) * c + 32 * ks + ff_perm(g, j)];
        }
      for (int o = 0; o < c; ++o)
        for (int g = 0; g < 4; ++g)
          for (int j = 0; j < 8; ++j)
          {
            const T wv = wt_host[f.w2.wt + (int64_t)o * hidden + ch * 32 + ff_perm(g, j)];
            // WX_FF_F16: the kernel's GEMM2 runs on f16 operands (hidden activations in f16): the SAME rounded bf16 weight, re-encoded
            // (exact: 8 significand bits into 11; only magnitudes below 6e-8 are lost)
            T enc = wv;
            if constexpr (sizeof(T) == 2) { if (WX_FF_F16) enc = (T)f2h_bits(Elem<T>::to_f(wv)); }
            wt_host[base + 32 * (int64_t)c + (int64_t)o * 32 + ff_w2_slot(o, g) * 8 + j] = enc;
          }
    }
    return off;
  }
  FFL make_ff(const std::string& p, int c, const AttnL* prev = nullptr) {
    FFL f;
    const HostTensor &g = spec.need(p + ".layers.0.g"), &b = spec.need(p + ".layers.0.b");
    f.w1 = make_conv(p + ".layers.1", 0, 4 * c, c, c, 1, 1, true, g.data.data(), b.data.data());
    pack_kblocked(f.w1);
    f.w2 = make_conv(p + ".layers.4", 0, c, 4 * c, 4 * c, 1, 1, true, nullptr, nullptr);
    pack_kblocked(f.w2);
    if constexpr (sizeof(T) == 2) {
      if (ff_fused_supported(c, 4 * c)) {
        f.pack = pack_ff(f, c, 4 * c);
        if (prev) f.pack_pre = pack_ff(f, c, 4 * c, &prev->out);
      } else if (ff_plain_supported(c, 4 * c)) {
        f.pack = pack_ff(f, c, 4 * c);
      }
    }
    return f;
  }

  void run() {
    int dims[5] = {spec.C_in_model, cfg.dim[0], cfg.dim[1], cfg.dim[2], cfg.dim[3]};
    for (int s = 0; s < 4; ++s) {
      StageL st;
      std::vector<int> ks(cfg.embed_kernels[s], cfg.embed_kernels[s] + cfg.n_embed_kernels[s]);
      std::sort(ks.begin(), ks.end());
      const int cin = dims[s], cout = dims[s + 1];
      const int cpad = s == 0 ? spec.cpad0 : cin;
      int acc = 0;
      std::vector<int> cos;
      for (size_t b = 0; b < ks.size(); ++b) {
        const int co = (b + 1 < ks.size()) ? (int)(cout / (1 << (b + 1))) : cout - acc;
        acc += co;
        cos.push_back(co);
      }
      // stage 0 on the LDS-patch kernel (wx_embed.h): branches k = 32 / 16 / 8 in its accumulator row [16 | 16 | 32]; the k = 4 branch
      // rides in the rows they leave empty when it fits (1-degree model: 8 + 8 + 16 spare rows = its 32 channels)
      std::vector<bool> pok(ks.size(), false);
      int cap[3] = {16, 16, 32}, used[3] = {0, 0, 0}, bidx[3] = {-1, -1, -1}, b4 = -1;
      for (size_t b = 0; b < ks.size(); ++b) {
        pok[b] = s == 0 && cfg.embed_strides[0] == 2 && cos[b] % 4 == 0 && ks.back() == 32 &&
                 ((ks[b] == 32 && cos[b] <= 16) || (ks[b] == 16 && cos[b] <= 16) || (ks[b] == 8 && cos[b] <= 32));
        if (pok[b]) { const int j = ks[b] == 32 ? 0 : ks[b] == 16 ? 1 : 2; used[j] = cos[b]; bidx[j] = (int)b; }
        if (ks[b] == 4) b4 = (int)b;
      }
      int ride[3] = {0, 0, 0}, ride0[3] = {0, 0, 0};   // k = 4 channels [ride0, ride0 + ride) in the spare rows of branch j
      if (s == 0 && opt.embed_ride4 && b4 >= 0 && cos[b4] % 4 == 0 && bidx[0] >= 0 && bidx[1] >= 0 && bidx[2] >= 0 &&
          (cap[0] - used[0]) + (cap[1] - used[1]) + (cap[2] - used[2]) >= cos[b4]) {
        int left = cos[b4], at4 = 0;
        for (int j = 0; j < 3; ++j) {
          ride[j] = std::min(left, cap[j] - used[j]); ride0[j] = at4;
          at4 += ride[j]; left -= ride[j];
        }
        st.ride4 = true;
      }
      std::vector<int> choffs;
      { int o = 0; for (int co : cos) { choffs.push_back(o); o += co; } }
      for (size_t b = 0; b < ks.size(); ++b) {
        const std::string bp = spec.embed_key(s, (int)b);
        const int j = ks[b] == 32 ? 0 : ks[b] == 16 ? 1 : 2;
        if (pok[b] && st.ride4 && ride[j] > 0) st.patch.push_back(make_patch(bp, cos[b], cin, cpad, ks[b], spec.embed_key(s, b4), 4, ride0[j], ride[j]));
        else st.patch.push_back(pok[b] ? make_patch(bp, cos[b], cin, cpad, ks[b]) : PatchW());
        st.embed.push_back(make_conv(bp, 0, cos[b], cin, cpad, ks[b], ks[b], true, nullptr, nullptr));
        st.embed_k.push_back(ks[b]);
      }
      if (s == 0 && bidx[0] >= 0) {   // slot table + bias row of the patch kernel's 64-wide accumulator row
        std::vector<float> tab(16, -1.f), bias64(64, 0.f);
        const int row0[3] = {0, 16, 32};
        for (int j = 0; j < 3; ++j) {
          if (bidx[j] < 0) continue;
          const HostTensor& bt = spec.need(spec.embed_key(s, bidx[j]) + ".bias");
          for (int r = 0; r < used[j]; ++r) {
            bias64[row0[j] + r] = bt.data[r];
            if (r % 4 == 0) tab[(row0[j] + r) / 4] = (float)(choffs[bidx[j]] + r);
          }
          if (st.ride4) {
            const HostTensor& b4t = spec.need(spec.embed_key(s, b4) + ".bias");
            for (int r = 0; r < ride[j]; ++r) {
              bias64[row0[j] + used[j] + r] = b4t.data[ride0[j] + r];
              if (r % 4 == 0) tab[(row0[j] + used[j] + r) / 4] = (float)(choffs[b4] + ride0[j] + r);
            }
          }
        }
        st.patch_tab = push_f(tab);
        st.patch_bias64 = push_f(bias64);
      }
      {   // one launch for the whole CrossEmbed where launches, not FLOPs, are the cost (stages 1-3 of the 1-degree grid)
        bool same_parity = ks.size() >= 2 && opt.embed_merge && s >= 1;
        for (int kk : ks) same_parity = same_parity && ((ks.back() - kk) % 2 == 0) && kk >= cfg.embed_strides[s];
        // launch-bound = the merged GEMM itself is tiny (1-degree grid: 0.75 G products per stage); the 0.25-degree stages 2-3 pass the
        // token test but are 42 G products each, where the padding costs more than the launch (107 / 123 us against 96 / 100 for the pair)
        const double products = (double)spec.sh[s] * spec.sw[s] * cout * ks.back() * ks.back() * cin;
        if (same_parity && spec.small_map_tokens(s) && products <= 4e9 && spec.sh[s] > 0) st.merged = make_embed_merged(s, ks, cos, cin, cpad);
      }
      for (int d = 0; d < cfg.depth[s]; ++d) {
        const std::string p = "layers." + std::to_string(s) + ".1.layers." + std::to_string(d);
        BlockL bl;
        bl.sa = make_attn(p + ".0", cout, cfg.local_window_size[s], 0);
        bl.sf = make_ff(p + ".1", cout, &bl.sa);
        bl.la = make_attn(p + ".2", cout, cfg.global_window_size[s], 1);
        bl.lf = make_ff(p + ".3", cout, &bl.la);
        st.blocks.push_back(bl);
      }
      tab.stages[s] = std::move(st);
      // second pass (block addresses are final now): feed-forward kernels that also run the NEXT attention's to_qkv
      if constexpr (sizeof(T) == 2) {
        std::vector<BlockL>& bs = tab.stages[s].blocks;
        const int c = cfg.dim[s];
        for (size_t d = 0; d < bs.size(); ++d) {
          FFL* ffs[2] = {&bs[d].sf, &bs[d].lf};
          const AttnL* prev[2] = {&bs[d].sa, &bs[d].la};
          const AttnL* next[2] = {&bs[d].la, d + 1 < bs.size() ? &bs[d + 1].sa : nullptr};
          for (int k = 0; k < 2; ++k)
            if (ffs[k]->pack_pre >= 0 && next[k] && next[k]->wsz > 1) {
              ffs[k]->next = next[k];
              ffs[k]->pack_pp = pack_ff(*ffs[k], c, 4 * c, &prev[k]->out, &next[k]->qkv);
            }
        }
      } else {   // fp32 storage: the split-bf16 one-launch FeedForward's to_qkv tail (wx_ff_split.h POST) reads the next attention's weights in place
        std::vector<BlockL>& bs = tab.stages[s].blocks;
        for (size_t d = 0; d < bs.size(); ++d) {
          if (bs[d].la.wsz > 1) bs[d].sf.next = &bs[d].la;
          if (d + 1 < bs.size() && bs[d + 1].sa.wsz > 1) bs[d].lf.next = &bs[d + 1].sa;
        }
      }
    }
    const int last = cfg.dim[3];
    const int upc[3][2] = {{last, last / 2}, {2 * (last / 2), last / 4}, {2 * (last / 4), last / 8}};
    for (int i = 0; i < 3; ++i) {
      const std::string p = "up_block" + std::to_string(i + 1);
      UpL u;
      u.cin = upc[i][0]; u.cout = upc[i][1];
      if (u.cout % 32) throw StateError("decoder: a width ModelSpec::derive() should have refused");
      if (spec.ps_decoder()) {
        // sub-pixel conv: reference channel c*4+q feeds sub-pixel q of channel c (PixelShuffle); rows reordered
        // to q*cout + c so the ConvT-style scatter epilogue (out_mode 1) performs the shuffle
        std::vector<int> src(4 * u.cout);
        for (int q = 0; q < 4; ++q)
          for (int c = 0; c < u.cout; ++c) src[q * u.cout + c] = c * 4 + q;
        u.convps = make_conv(p + ".conv", 0, 0, u.cin, u.cin, 3, 3, true, nullptr, nullptr, &src);
        u.sharp = make_conv(p + ".sharp", 0, u.cout, u.cout, u.cout, 3, 3, true, nullptr, nullptr);
      } else if (cfg.arch == WX_ARCH_CROSSFORMER_UPCONV) {
        u.upc = make_conv(p + ".conv", 0, u.cout, u.cin, u.cin, 3, 3, true, nullptr, nullptr);
      } else {
        u.convt = make_convt2(p + ".conv", u.cin, u.cout);
      }
      u.c1 = make_conv(p + ".b.0", 0, u.cout, u.cout, u.cout, 3, 3, true, nullptr, nullptr);
      u.c2 = make_conv(p + ".b.3", 0, u.cout, u.cout, u.cout, 3, 3, true, nullptr, nullptr);
      u.g1 = push_f(spec.need(p + ".b.1.weight").data); u.b1 = push_f(spec.need(p + ".b.1.bias").data);
      u.g2 = push_f(spec.need(p + ".b.4.weight").data); u.b2 = push_f(spec.need(p + ".b.4.bias").data);
      tab.ups[i] = u;
    }
    if (spec.ps_decoder()) {
      tab.cpad4 = ((spec.C_out + 31) / 32) * 32;  // padded channel count of the shuffled map (zero rows / zero input weights)
      std::vector<int> src(4 * tab.cpad4, -1);
      for (int q = 0; q < 4; ++q)
        for (int c = 0; c < spec.C_out; ++c) src[q * tab.cpad4 + c] = c * 4 + q;
      tab.ps4 = make_conv("up_block4.0", 0, 0, 2 * (last / 8), 2 * (last / 8), 3, 3, true, nullptr, nullptr, &src);
      tab.fin4 = make_conv("up_block4.2", 0, spec.C_out, spec.C_out, tab.cpad4, 3, 3, true, nullptr, nullptr);
    } else if (cfg.arch == WX_ARCH_CROSSFORMER_UPCONV) {
      tab.up4c = make_conv("up_block4.1", 0, spec.C_out, 2 * (last / 8), 2 * (last / 8), 3, 3, true, nullptr, nullptr);
    } else {
      make_convt4("up_block4", 2 * (last / 8), spec.C_out);
    }

    for (int l = 0; l < 6; ++l) {
      tab.nz[l] = NoiseL{};
      if (!spec.noise_slot_on(l)) continue;
      const std::string p = spec.noise_prefix(l);
      tab.nz[l].w = push_f(spec.need(p + ".noise_transform.weight").data);
      tab.nz[l].b = push_f(spec.need(p + ".noise_transform.bias").data);
      tab.nz[l].mod = push_f(spec.need(p + ".modulation").data);
      tab.nz[l].nf = push_f(spec.need(p + ".noise_factor").data);
    }
  }
};

}  // namespace wx

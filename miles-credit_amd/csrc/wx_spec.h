// wxengine: what the model is -- the validated wx_config, the geometry derived from it and the reference-layout state dict
// (key list, loaded host tensors, the spectral-norm fold).  Host only: nothing here depends on the storage type or calls HIP,
// so the lat-band planner (wx_band_plan_create) builds a ModelSpec without an engine or a GPU.
#pragma once
#include "../../include/wxengine.h"

#include <algorithm>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "wx_attn.h"   // attn_nkf(): the window sizes the attention kernels take
#include "wx_band.h"   // BandModel

namespace wx {

struct ConfigError : std::runtime_error { using std::runtime_error::runtime_error; };
struct StateError : std::runtime_error { using std::runtime_error::runtime_error; };
struct MissingError : std::runtime_error { using std::runtime_error::runtime_error; };
struct ShapeError : std::runtime_error { using std::runtime_error::runtime_error; };

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
  bool loaded = false;
  int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};

// ------------------------------------------------------------------ shape limits of the kernels, known from the config alone
// `elem`: bytes per stored activation element (4: WX_PREC_FP32 / WX_PREC_FP32_SPLIT, 2: WX_PREC_BF16).  ModelSpec::derive() refuses a
// config that misses one of them, so wx_create returns either an engine whose forward runs or WX_ERR_INVALID with the reason.
// LayerNorm (ln_stats_kernel, wx_elem.h): min(64, pieces) lanes share a row of C / (16 / elem) 16-byte pieces -- a power of two of
// them (the butterfly reduction), every lane the same number of pieces, at most four
inline bool ln_width_ok(int c, int elem) {
  const int vec = 16 / elem;
  if (c < vec || c % vec) return false;
  const int pieces = c / vec, lpt = pieces >= 64 ? 64 : pieces;
  return !(lpt & (lpt - 1)) && pieces % lpt == 0 && pieces / lpt <= 4;
}
// GroupNorm (gn_stats_kernel): one thread per 16-byte piece of a row, 256 threads
inline bool gn_width_ok(int c, int elem) { return c / (16 / elem) <= 256; }
// tail kernel: a [C_out][65] fp32 tile in 160 KB of LDS
inline bool tail_channels_ok(int c_out) { return (size_t)c_out * 65 * sizeof(float) <= (size_t)160 * 1024; }

struct ModelSpec {
  explicit ModelSpec(const wx_config& c) : cfg(c) {
    derive();
    build_spec();
  }

  // ------------------------------------------------------------------ config
  wx_config cfg;
  int C_in = 0, C_out = 0, Hp = 0, Wp = 0, halo = 0, cpad0 = 0;
  // C_in: planes of the caller's input tensor (and of the PostBlock's x), frames included.  C_in_model: channels of the first conv =
  // of the packed stage-0 input (cpad0 pads it).  They differ for WX_ARCH_CAMULATOR at frames == 2 only, whose entry averages the frames
  int C_in_model = 0;
  // the two halves an arch pairs: the CrossEmbed form (ZeroPad2d-wrapped branches or bare convs) and the decoder
  bool ps_decoder() const { return cfg.arch == WX_ARCH_WXFORMER || cfg.arch == WX_ARCH_CAMULATOR; }
  bool zeropad_embed() const { return cfg.arch == WX_ARCH_WXFORMER; }
  bool avg_frames() const { return cfg.arch == WX_ARCH_CAMULATOR && cfg.frames == 2; }
  int sh[4], sw[4];           // stage maps
  int Hd = 0, Wd = 0, Hu = 0, Wu = 0, Ho = 0, Wo = 0, ld_dec = 0;

  void derive() {
    if (cfg.abi_version != WX_ABI_VERSION) throw ConfigError("wx_config.abi_version mismatch");
    if (cfg.frames < 1 || cfg.output_frames < 1) throw ConfigError("frames/output_frames must be >= 1");
    // dim_head (crossformer.py:372-401, a constructor kwarg; every YAML of the reference leaves the default 32): 32 runs the tuned kernels;
    // 64 / 128 run the general-head-dimension attention kernel of the Swin mode (launch_window_attn_any) between the plain GEMMs --
    // the attention block kernel and the fused FeedForward's to_out / to_qkv variants are built around 32-wide heads and stay off
    if (cfg.dim_head == 96)   // a width with LayerNorm's power-of-two pieces (32, 64, 128, ...) is never a multiple of 96
      throw ConfigError("dim_head 96 is for wx_winattn_create / wx_swin_create only: no stage width the LayerNorm kernels take is a multiple of 96");
    if (cfg.dim_head != 32 && cfg.dim_head != 64 && cfg.dim_head != 128)
      throw ConfigError("dim_head must be 32, 64 or 128");
    for (int s = 0; s < 4; ++s)
      if (cfg.dim[s] % cfg.dim_head) throw ConfigError("every stage width must be a multiple of dim_head");
    if (cfg.dim_head != 32)   // launch_window_attn_dh: windows of at most 128 tokens
      for (int s = 0; s < 4; ++s)
        if (cfg.local_window_size[s] * cfg.local_window_size[s] > 128 || cfg.global_window_size[s] * cfg.global_window_size[s] > 128)
          throw ConfigError("dim_head != 32 needs windows of at most 128 tokens (the general attention kernel's limit)");
    if (cfg.arch != WX_ARCH_CROSSFORMER && cfg.arch != WX_ARCH_WXFORMER && cfg.arch != WX_ARCH_CROSSFORMER_UPCONV &&
        cfg.arch != WX_ARCH_CAMULATOR)
      throw ConfigError("unknown wx_config.arch");
    if (cfg.noise_latent_dim < 0 || cfg.noise_latent_dim > 4096) throw ConfigError("noise_latent_dim must be in 0 .. 4096");
    if (cfg.noise_latent_dim > 0 && cfg.arch == WX_ARCH_WXFORMER)
      throw ConfigError("noise layers belong to crossformer-ensemble (a legacy CrossFormer subclass): not with the wxformer decoder");
    if (cfg.arch == WX_ARCH_CAMULATOR) {
      if (cfg.noise_latent_dim > 0) throw ConfigError("camulator: noise layers belong to crossformer-ensemble, the Camulator class has none");
      // camulator.py:587-588 F.avg_pool3d(x, (2, 1, 1)).squeeze(2): frames 0 and 1 are averaged, a third is dropped without a word, four fail
      if (cfg.frames > 2) throw ConfigError("camulator: frames must be 1 or 2 (the entry averages frames 0 and 1; the reference drops a third and fails on four)");
      if (cfg.output_frames != 1) throw ConfigError("camulator: output_frames must be 1 (the class has no such argument)");
    }
    C_in_model = cfg.channels * cfg.levels + cfg.surface_channels + cfg.input_only_channels;
    C_in = C_in_model * cfg.frames;
    if (cfg.arch != WX_ARCH_CAMULATOR) C_in_model = C_in;   // every other class reshapes the frames into channels (c * t)
    C_out = (cfg.channels * cfg.levels + cfg.surface_channels + cfg.output_only_channels) * cfg.output_frames;
    Hp = cfg.image_height + (cfg.pad_activate ? cfg.pad_lat[0] + cfg.pad_lat[1] : 0);
    Wp = cfg.image_width + (cfg.pad_activate ? cfg.pad_lon[0] + cfg.pad_lon[1] : 0);
    if (cfg.pad_activate && cfg.pad_lat[0] > 0 && cfg.pad_lat[1] == 0)
      throw ConfigError("pad_lat=[p,0] hits a slicing quirk of the reference (boundary_padding.py:66); unsupported");
    if (cfg.pad_activate && (cfg.pad_lat[0] > cfg.image_height || cfg.pad_lat[1] > cfg.image_height))
      throw ConfigError("pad_lat larger than the image");
    if (cfg.pad_activate == 2 && (cfg.pad_lat[0] >= cfg.image_height || cfg.pad_lat[1] >= cfg.image_height))
      throw ConfigError("padding mode mirror: pad_lat must be smaller than the image height (reflection without the edge row)");
    int h = Hp, w = Wp;
    for (int s = 0; s < 4; ++s) {
      const int st = cfg.embed_strides[s];
      if (cfg.n_embed_kernels[s] < 1 || cfg.n_embed_kernels[s] > 4) throw ConfigError("1..4 cross-embed kernels per stage");
      int oh = -1, ow = -1;
      for (int b = 0; b < cfg.n_embed_kernels[s]; ++b) {
        const int k = cfg.embed_kernels[s][b];
        if (k < st) throw ConfigError("cross-embed kernel smaller than stride");
        const int pd = (k - st) / 2;
        // legacy: symmetric padding pd; wxformer: ZeroPad2d(lo = (k-s)/2, hi = (k-s) - lo) then an un-padded conv
        const int pad_total = zeropad_embed() ? (k - st) : 2 * pd;
        const int h2 = (h + pad_total - k) / st + 1, w2 = (w + pad_total - k) / st + 1;
        if (oh >= 0 && (h2 != oh || w2 != ow)) throw ConfigError("cross-embed branches disagree on output size");
        oh = h2; ow = w2;
        if (s == 0) halo = std::max(halo, pad_total - pd);
      }
      sh[s] = h = oh; sw[s] = w = ow;
      if (cfg.dim[s] % 32) throw ConfigError("dim must be a multiple of 32");
      for (int wsz : {cfg.local_window_size[s], cfg.global_window_size[s]}) {
        if (wsz < 1 || h % wsz || w % wsz) throw ConfigError("stage map not divisible by window size");
        if (attn_nkf(wsz) < 0) throw ConfigError("window size > 16 (more than 256 tokens) unsupported");
      }
    }
    for (int s = 0; s < 3; ++s) {
      if (sh[s] != 2 * sh[s + 1] || sw[s] != 2 * sw[s + 1]) throw ConfigError("stage maps must halve (decoder skip concat)");
      if (cfg.dim[s + 1] != 2 * cfg.dim[s]) throw ConfigError("dim must double per stage (decoder skip widths)");
    }
    // the widths the kernels take (thrown by the first forward / by finalize before: LayerNorm, GroupNorm, decoder, tail)
    const int elem = cfg.precision == WX_PREC_BF16 ? 2 : 4;
    for (int s = 0; s < 4; ++s)
      if (!ln_width_ok(cfg.dim[s], elem)) throw ConfigError("LayerNorm width unsupported (need power-of-two pieces, C <= 1024 fp32)");
    for (int i = 1; i <= 3; ++i) {   // up block i: dim[3] / 2^i output channels
      const int c = cfg.dim[3] >> i;
      if (c % 32) throw ConfigError("decoder widths must be multiples of 32");
      if (!gn_width_ok(c, elem)) throw ConfigError("GroupNorm width unsupported");
    }
    if (!tail_channels_ok(C_out)) throw ConfigError("too many output channels for the tail kernel");
    for (int s = 0; s < 4; ++s)
      for (int wsz : {cfg.local_window_size[s], cfg.global_window_size[s]})
        if (wsz > 1 && !window_attn_lds_ok(elem, attn_nkf(wsz), cfg.dim_head, false))
          throw ConfigError("window attention: dim_head x window size exceeds the kernel's 160 KB of LDS (fp32 storage: dim_head 128 takes windows of at most 64 tokens)");
    cpad0 = ((C_in_model + 31) / 32) * 32;
    Hd = sh[3] * 16; Wd = sw[3] * 16;
    Hu = Hd - (cfg.pad_activate ? cfg.pad_lat[0] + cfg.pad_lat[1] : 0);
    Wu = Wd - (cfg.pad_activate ? cfg.pad_lon[0] + cfg.pad_lon[1] : 0);
    if (Hu < 1 || Wu < 1) throw ConfigError("decoder output smaller than the padding");
    Ho = cfg.interp ? cfg.image_height : Hu;
    Wo = cfg.interp ? cfg.image_width : Wu;
    ld_dec = ((C_out + 7) / 8) * 8;
    if (cfg.max_batch < 1) cfg.max_batch = 1;
  }

  // ------------------------------------------------------------------ state dict
  std::vector<std::string> keys;
  std::map<std::string, HostTensor> tensors;

  void add_key(const std::string& k, std::vector<int64_t> shape) {
    keys.push_back(k);
    HostTensor t;
    t.shape = std::move(shape);
    tensors[k] = std::move(t);
  }
  // sn = false: a conv the class leaves out of apply_spectral_norm (camulator.py:22-28 skips every module named "sharp")
  void add_conv(const std::string& p, std::vector<int64_t> shape, bool bias, bool transposed = false, bool sn = true) {
    const int64_t nb = transposed ? shape[1] : shape[0];
    if (cfg.use_spectral_norm && sn) {
      if (bias) add_key(p + ".bias", {nb});
      add_key(p + ".weight_orig", shape);
      int64_t rest = 1;
      if (transposed) {
        rest = shape[0];
        for (size_t i = 2; i < shape.size(); ++i) rest *= shape[i];
        add_key(p + ".weight_u", {shape[1]});
      } else {
        for (size_t i = 1; i < shape.size(); ++i) rest *= shape[i];
        add_key(p + ".weight_u", {shape[0]});
      }
      add_key(p + ".weight_v", {rest});
    } else {
      add_key(p + ".weight", shape);
      if (bias) add_key(p + ".bias", {nb});
    }
  }
  void build_spec() {
    int dims[5] = {C_in_model, cfg.dim[0], cfg.dim[1], cfg.dim[2], cfg.dim[3]};
    for (int s = 0; s < 4; ++s) {
      const int cin = dims[s], cout = dims[s + 1];
      std::vector<int> ks(cfg.embed_kernels[s], cfg.embed_kernels[s] + cfg.n_embed_kernels[s]);
      std::sort(ks.begin(), ks.end());
      std::vector<int> sc;
      int acc = 0;
      for (size_t i = 1; i < ks.size(); ++i) { sc.push_back((int)(cout / (1 << i))); acc += sc.back(); }
      sc.push_back(cout - acc);
      for (size_t b = 0; b < ks.size(); ++b)
        add_conv(embed_key(s, (int)b), {sc[b], cin, ks[b], ks[b]}, true);
      const int dq = cout / 4;
      for (int d = 0; d < cfg.depth[s]; ++d) {
        for (int j = 0; j < 4; ++j) {
          const std::string p = "layers." + std::to_string(s) + ".1.layers." + std::to_string(d) + "." + std::to_string(j);
          if (j == 0 || j == 2) {
            add_key(p + ".norm.g", {1, cout, 1, 1});
            add_key(p + ".norm.b", {1, cout, 1, 1});
            add_conv(p + ".to_qkv", {3 * cout, cout, 1, 1}, false);
            add_conv(p + ".to_out", {cout, cout, 1, 1}, true);
            add_conv(p + ".dpb.layers.0", {dq, 2}, true);
            add_key(p + ".dpb.layers.1.weight", {dq});
            add_key(p + ".dpb.layers.1.bias", {dq});
            add_conv(p + ".dpb.layers.3", {dq, dq}, true);
            add_key(p + ".dpb.layers.4.weight", {dq});
            add_key(p + ".dpb.layers.4.bias", {dq});
            add_conv(p + ".dpb.layers.6", {dq, dq}, true);
            add_key(p + ".dpb.layers.7.weight", {dq});
            add_key(p + ".dpb.layers.7.bias", {dq});
            add_conv(p + ".dpb.layers.9", {1, dq}, true);
          } else {
            add_key(p + ".layers.0.g", {1, cout, 1, 1});
            add_key(p + ".layers.0.b", {1, cout, 1, 1});
            add_conv(p + ".layers.1", {4 * cout, cout, 1, 1}, true);
            add_conv(p + ".layers.4", {cout, 4 * cout, 1, 1}, true);
          }
        }
      }
    }
    const int last = cfg.dim[3];
    const int ups[3][2] = {{last, last / 2}, {2 * (last / 2), last / 4}, {2 * (last / 4), last / 8}};
    for (int i = 0; i < 3; ++i) {
      const std::string p = "up_block" + std::to_string(i + 1);
      if (ps_decoder()) {  // UpBlockPS (wxformer/crossformer.py:137-162, camulator.py:102-127)
        add_conv(p + ".conv", {4 * ups[i][1], ups[i][0], 3, 3}, true);
        add_conv(p + ".sharp", {ups[i][1], ups[i][1], 3, 3}, true, false, cfg.arch != WX_ARCH_CAMULATOR);
      } else if (cfg.arch == WX_ARCH_CROSSFORMER_UPCONV) {  // nn.Upsample + Conv2d 3x3 (crossformer.py:87-89)
        add_conv(p + ".conv", {ups[i][1], ups[i][0], 3, 3}, true);
      } else {
        add_conv(p + ".conv", {ups[i][0], ups[i][1], 2, 2}, true, true);
      }
      for (int j : {0, 3}) {
        add_conv(p + ".b." + std::to_string(j), {ups[i][1], ups[i][1], 3, 3}, true);
        add_key(p + ".b." + std::to_string(j + 1) + ".weight", {ups[i][1]});
        add_key(p + ".b." + std::to_string(j + 1) + ".bias", {ups[i][1]});
      }
    }
    if (ps_decoder()) {  // Sequential(conv3x3 -> PixelShuffle -> conv3x3) (wxformer/crossformer.py:817-830, camulator.py:546-557)
      add_conv("up_block4.0", {4 * C_out, 2 * (last / 8), 3, 3}, true);
      add_conv("up_block4.2", {C_out, C_out, 3, 3}, true);
    } else if (cfg.arch == WX_ARCH_CROSSFORMER_UPCONV) {  // Sequential(Upsample, Conv2d) (crossformer.py:560-570)
      add_conv("up_block4.1", {C_out, 2 * (last / 8), 3, 3}, true);
    } else {
      add_conv("up_block4", {2 * (last / 8), C_out, 4, 4}, true, true);
    }
    // CrossFormerWithNoise (crossformer_ensemble.py): created after apply_spectral_norm, so noise_transform keeps a plain `weight`
    for (int l = 0; l < 6; ++l) {
      if (!noise_slot_on(l)) continue;
      const std::string p = noise_prefix(l);
      const int c = noise_channels(l);
      add_key(p + ".modulation", {1, c, 1, 1});
      add_key(p + ".noise_factor", {1});
      add_key(p + ".noise_transform.weight", {c, cfg.noise_latent_dim});
      add_key(p + ".noise_transform.bias", {c});
    }
  }
  // noise slots: 0 - 2 encoder_noise_layers.{0,1,2} (after stage k, width dim[k]); 3 - 5 noise_inject{1,2,3} (after up_block n, width dim[3 - n])
  bool noise_slot_on(int l) const { return cfg.noise_latent_dim > 0 && (l >= 3 || cfg.encoder_noise); }
  std::string noise_prefix(int l) const {
    return l < 3 ? "encoder_noise_layers." + std::to_string(l) : "noise_inject" + std::to_string(l - 2);
  }
  int noise_channels(int l) const { return l < 3 ? cfg.dim[l] : cfg.dim[5 - l]; }
  std::string embed_key(int s, int b) const {
    return "layers." + std::to_string(s) + ".0.convs." + std::to_string(b) + (zeropad_embed() ? ".1" : "");
  }

  void load_tensor(const char* key, const float* data, int ndim, const int64_t* shape) {
    auto it = tensors.find(key);
    if (it == tensors.end() && cfg.arch == WX_ARCH_WXFORMER) {
      // pre-ZeroPad2d checkpoints keep CrossEmbed parameters at convs.<i>.<suffix>; the reference migrates them
      // to convs.<i>.1.<suffix> on load (wxformer/crossformer.py:247-283) -- do the same
      const std::string k(key);
      const size_t pos = k.find(".0.convs.");
      if (k.rfind("layers.", 0) == 0 && pos != std::string::npos) {
        const size_t dot = k.find('.', pos + 9);
        if (dot != std::string::npos && !(k.size() > dot + 2 && isdigit((unsigned char)k[dot + 1]) && k[dot + 2] == '.'))
          it = tensors.find(k.substr(0, dot) + ".1" + k.substr(dot));
      }
    }
    if (it == tensors.end()) {
      // reference semantics: load_state_dict(strict=False) ignores unexpected keys (base_model.py:77-80)
      return;
    }
    HostTensor& t = it->second;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= shape[i];
    // torch semantics: the shapes must agree.  Only singleton dimensions may differ ((1, C, 1, 1) vs (C,)): the same
    // element count in another layout ([128, 256, 2, 2] for a [256, 128, 2, 2] ConvTranspose weight) would load scrambled.
    std::vector<int64_t> got, want;
    for (int i = 0; i < ndim; ++i) if (shape[i] != 1) got.push_back(shape[i]);
    for (int64_t d : t.shape) if (d != 1) want.push_back(d);
    if (n != t.numel() || got != want) {
      auto fmt = [](const int64_t* d, size_t k) { std::string r = "("; for (size_t i = 0; i < k; ++i) r += (i ? ", " : "") + std::to_string(d[i]); return r + ")"; };
      throw ShapeError(std::string("size mismatch for ") + key + ": checkpoint " + fmt(shape, (size_t)ndim) + " vs model " +
                       fmt(t.shape.data(), t.shape.size()));
    }
    t.data.assign(data, data + n);
    t.loaded = true;
  }
  int num_tensors() { return (int)keys.size(); }
  void tensor_info(int i, const char** key, int* ndim, int64_t shape[8]) {
    if (i < 0 || i >= (int)keys.size()) throw ConfigError("tensor index out of range");
    const HostTensor& t = tensors[keys[i]];
    *key = keys[i].c_str();
    *ndim = (int)t.shape.size();
    for (size_t d = 0; d < t.shape.size() && d < 8; ++d) shape[d] = t.shape[d];
  }
  const HostTensor& need(const std::string& k) const {
    auto it = tensors.find(k);
    if (it == tensors.end() || !it->second.loaded) throw MissingError("state-dict tensor '" + k + "' was not loaded");
    return it->second;
  }

  // eval-mode spectral norm: W / (u . (W_mat v)); W_mat rows = dim 0 (dim 1 for ConvTranspose2d)
  std::vector<double> folded(const std::string& p, bool transposed) const {
    if (!cfg.use_spectral_norm || !tensors.count(p + ".weight_orig")) {   // the spec lists `weight` for a conv without spectral norm
      const HostTensor& w = need(p + ".weight");
      return std::vector<double>(w.data.begin(), w.data.end());
    }
    const HostTensor& w = need(p + ".weight_orig");
    const HostTensor& u = need(p + ".weight_u");
    const HostTensor& v = need(p + ".weight_v");
    const int64_t d0 = w.shape[0], d1 = w.shape.size() > 1 ? w.shape[1] : 1;
    int64_t rest = 1;
    for (size_t i = 2; i < w.shape.size(); ++i) rest *= w.shape[i];
    double sigma = 0.0;
    if (!transposed) {
      const int64_t cols = d1 * rest;
      for (int64_t r = 0; r < d0; ++r) {
        double acc = 0.0;
        const float* row = w.data.data() + r * cols;
        for (int64_t c = 0; c < cols; ++c) acc += (double)row[c] * v.data[c];
        sigma += acc * u.data[r];
      }
    } else {
      // W_mat[o][i*rest + k] = W[i][o][k]
      for (int64_t o = 0; o < d1; ++o) {
        double acc = 0.0;
        for (int64_t i = 0; i < d0; ++i)
          for (int64_t k = 0; k < rest; ++k) acc += (double)w.data[(i * d1 + o) * rest + k] * v.data[i * rest + k];
        sigma += acc * u.data[o];
      }
    }
    std::vector<double> out(w.data.size());
    for (size_t i = 0; i < out.size(); ++i) out[i] = (double)w.data[i] / sigma;
    return out;
  }

  bool small_map_tokens(int s) const { return (int64_t)sh[s] * sw[s] <= 32768; }
};

// ------------------------------------------------------------------ what the lat-band planner needs of a model (wx_band.h)
// elem: bytes per activation element; n_fix: conservation fixers of the attached post block
inline BandModel band_model(const ModelSpec& e, int n, int elem, int n_fix) {
  BandModel m;
  m.n = n; m.C_in = e.C_in; m.H = e.cfg.image_height; m.W = e.cfg.image_width;
  m.p0 = e.cfg.pad_activate ? e.cfg.pad_lat[0] : 0; m.p1 = e.cfg.pad_activate ? e.cfg.pad_lat[1] : 0;
  m.Hp = e.Hp; m.halo = e.halo;
  for (int s = 0; s < 4; ++s) {
    m.stride[s] = e.cfg.embed_strides[s];
    m.sh[s] = e.sh[s]; m.sw[s] = e.sw[s];
    m.wl[s] = e.cfg.local_window_size[s]; m.wg[s] = e.cfg.global_window_size[s];
    m.depth[s] = e.cfg.depth[s]; m.dim[s] = e.cfg.dim[s];
    int lo = 0, hi = 0;
    for (int b = 0; b < e.cfg.n_embed_kernels[s]; ++b) {
      const int k = e.cfg.embed_kernels[s][b], pd = (k - m.stride[s]) / 2;
      lo = std::max(lo, pd);
      hi = std::max(hi, k - m.stride[s] - pd);
    }
    m.emb_lo[s] = lo; m.emb_hi[s] = hi;
  }
  m.elem = elem;
  for (int i = 0; i < 3; ++i) m.up_cout[i] = e.cfg.dim[2 - i];
  m.Hd = e.Hd; m.Wd = e.Wd; m.Hu = e.Hu; m.Ho = e.Ho; m.off_y = e.cfg.pad_activate ? e.cfg.pad_lat[0] : 0;
  m.interp = e.cfg.interp; m.ld_dec = e.ld_dec;
  m.wxformer = e.cfg.arch == WX_ARCH_WXFORMER; m.cpad4 = ((e.C_out + 31) / 32) * 32;
  m.n_fix = n_fix;
  return m;
}
inline void band_check_supported(const ModelSpec& e) {
  if (e.cfg.arch == WX_ARCH_CAMULATOR)
    throw ConfigError("lat-band mode: the camulator arch is not wired (crossformer and wxformer are)");
  if (e.cfg.arch != WX_ARCH_CROSSFORMER && e.cfg.arch != WX_ARCH_WXFORMER)
    throw ConfigError("lat-band mode: the upsample_v_conv decoder variant is not wired (crossformer and wxformer are)");
  if (e.cfg.frames != 1 || e.cfg.output_frames != 1) throw ConfigError("lat-band mode needs frames == output_frames == 1");
  if (e.cfg.dim_head != 32) throw ConfigError("lat-band mode needs dim_head == 32");
  if (e.cfg.noise_latent_dim > 0) throw ConfigError("lat-band mode: the noise-injection ensemble (noise_latent_dim > 0) is not supported");
}

}  // namespace wx

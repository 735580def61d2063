// wxengine: MI355X-native CrossFormer/WXFormer forecast step behind the C ABI of include/wxengine.h.
//
// This file: Engine<T>, the object that runs a step -- it owns every activation buffer in HBM (token-major H x W x C) and issues
// the kernels of wx_gemm.h / wx_attn.h / wx_elem.h on the caller's HIP stream.  The host side around it:
//   wx_spec.h     what the model is: wx_config checks, derived geometry, the reference-layout state dict, the spectral-norm fold
//   wx_weights.h  how the weights are laid out: the layer tables and the packer that folds the state dict into the two arenas
//   wx_rccl.h     RCCL bound at run time for the lat-band transport
//   wx_abi.h      the extern "C" wrappers of include/wxengine.h
#include "../../include/wxengine.h"
#include "../../include/wxengine_sht.h"
#include "../../include/wxengine_polefilter.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "wx_attn.h"
#include "wx_ff.h"
#include "wx_common.h"
#include "wx_elem.h"
#include "wx_embed.h"
#include "wx_band.h"
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: the library is bound with dlopen when a communicator is requested
#include "wx_gemm.h"
#include "wx_gemm_stream.h"
#include "wx_gemm_wreg.h"
#include "wx_gemm8p.h"
#include "wx_ff_split.h"
#include "wx_attn_block.h"
#include "wx_swin.h"
#include "wx_fuxi.h"
#include "wx_post.h"
#include "wx_pre.h"
#include "wx_unxform.h"
#include "wx_diag.h"
#include "wx_wind.h"
#include "wx_advect.h"
#include "wx_hybrid.h"
#include "wx_regrid.h"
#include "wx_tisr.h"
#include "wx_dft.h"
#include "wx_perturb.h"
#include "wx_spectrum.h"
#include "wx_sht.h"
#include "wx_polefilter.h"
#include "wx_metrics.h"
#include "wx_ensemble.h"
#include "wx_noise.h"
#include "wx_options.h"
#include "wx_spec.h"
#include "wx_rccl.h"
#include "wx_weights.h"

namespace wx {

struct KernelStatAcc { int64_t launches = 0; double ms = 0, flops = 0, bytes = 0; };

class EngineBase {
 public:
  virtual ~EngineBase() {}
  virtual void load_tensor(const char* key, const float* data, int ndim, const int64_t* shape) = 0;
  virtual void finalize() = 0;
  virtual void forward(const float* x, float* y, int batch, hipStream_t s) = 0;
  virtual void step(const float* x, const float* frc, float* y, float* y_phys, float* x_next, hipStream_t s) = 0;
  virtual void rollout(const float* x0, const float* const* frc, int n_steps, float* const* y_phys, float* x_final, hipStream_t s) = 0;
  virtual void set_denorm(const float* mean, const float* stdv, int n) = 0;
  virtual void set_tracer(const int32_t* inds, const float* thres, const float* thres_max, int n, int denorm) = 0;
  virtual void set_layout(int n_prog, int n_static, int n_dyn) = 0;
  virtual void set_layout_groups(int n, const int32_t* kind, const int32_t* x_start, const int32_t* src_start, const int32_t* count) = 0;
  virtual int num_tensors() = 0;
  virtual void tensor_info(int i, const char** key, int* ndim, int64_t shape[8]) = 0;
  virtual void set_debug(int on) = 0;
  virtual void debug_read(const char* name, float* out, int64_t cap, int64_t shape[3]) = 0;
  virtual void profile(int on) = 0;
  virtual void profile_reset() = 0;
  virtual int profile_read(wx_kernel_stat* out, int cap) = 0;
  virtual void attach_post(PostBlock* p) = 0;
  virtual bool query(const std::string& key, int64_t* v) = 0;
  virtual void band_enable(int rank, int nranks) = 0;
  virtual void band_info(int* own_row0, int* own_rows, int64_t* send_bytes, int64_t* recv_bytes, int* n_exchanges) = 0;
  virtual void band_set_staging(void* send, int64_t send_bytes, void* recv, int64_t recv_bytes) = 0;
  virtual int band_messages_of(int xid, wx_band_msg* sends, int cap_s, int* n_s, wx_band_msg* recvs, int cap_r, int* n_r) = 0;
  virtual int band_begin(const float* x_own, const float* frc_own, float* y, float* y_phys, float* x_next, hipStream_t s) = 0;
  virtual int band_resume() = 0;
  virtual void* band_comm_stream(void* adopt) = 0;
  virtual void band_rccl_init(const ncclUniqueId& id) = 0;
  virtual void band_step_rccl(const float* x_own, const float* frc_own, float* y, float* y_phys, float* x_next, hipStream_t s) = 0;
  virtual void set_noise(uint64_t seed, int member0, int step) = 0;
  virtual void set_noise_tape(const float* const* draws, int n) = 0;
  int device = 0;
};

template <typename T>
class Engine : public EngineBase, public ModelSpec, public LayerTables {
 public:
  // split_mma (T = float only; wx_config.precision WX_PREC_FP32_SPLIT): fp32 storage, LayerNorm / softmax statistics / GroupNorm as the
  // exact-f32 engine, but every implicit GEMM (wx_gemm.h SPLIT), the stage-0 CrossEmbed (the bf16 patch kernel over K-concatenated
  // (hi, lo) planes, wx_embed.h) and the attention's Q.K^T / P.V (wx_attn.h M3) run split-bf16 arithmetic on the 2.5 PF pipe --
  // x = x_hi + x_lo, W = W_hi + W_lo (split once at load), three bf16 MFMAs per product with fp32 accumulation.  Measured error against
  // the reference's fp32 forward: ~1e-5 of max|y| (base weights), 5-7e-5 on the stress families -- inside the stated 1e-4 tolerance.
  bool split_mma = false;
  const Options opt;   // the run-time switches, read once by wx_create (wx_options.h)
  Engine(const wx_config& c, int dev, const Options& o, bool split = false) : ModelSpec(c), split_mma(split && sizeof(T) == 4), opt(o), mem(dev) {
    device = dev;
  }
  ~Engine() override {
    (void)hipSetDevice(device);
    if (b_comm) (void)RcclApi::get().CommDestroy(b_comm);
    if (b_cstream_own && b_cstream) (void)hipStreamDestroy(b_cstream);
    if (b_ev_pack) { (void)hipEventDestroy(b_ev_pack); (void)hipEventDestroy(b_ev_done); }
    roll_invalidate();
    if (roll_stream) { (void)hipStreamDestroy(roll_stream); (void)hipEventDestroy(roll_ev_in); (void)hipEventDestroy(roll_ev_out); }
    for (auto& e : ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  }

  // ------------------------------------------------------------------ state dict (wx_spec.h) and weights (wx_weights.h)
  bool finalized = false;
  void load_tensor(const char* key, const float* data, int ndim, const int64_t* shape) override {
    ModelSpec::load_tensor(key, data, ndim, shape);
    finalized = false;
  }
  int num_tensors() override { return (int)keys.size(); }
  void tensor_info(int i, const char** key, int* ndim, int64_t shape[8]) override { ModelSpec::tensor_info(i, key, ndim, shape); }
  T* wt_dev = nullptr;
  float* f_dev = nullptr;
  NoiseState* d_noise = nullptr;   // seed / member0 / step (device: advanced inside captured graphs)
  float* d_style = nullptr;        // [6][dim[3]] styles of the batch row being computed
  std::vector<const float*> noise_tape;   // wx_set_noise_tape: device pointers in the reference's draw order (empty: generator)
  int cur_row = 0;                 // batch row of the forward item being computed
  T* ps4_buf = nullptr;
  uint16_t* sp16_dev = nullptr;

  void finalize() override {
    WX_HIP(hipSetDevice(device));
    for (const auto& k : keys) need(k);
    WeightPacker<T> pk(*this, *this, opt, split_mma);
    pk.run();
    // upload
    mem.release(wt_dev);
    mem.release(f_dev);
    wt_dev = (T*)mem.alloc(pk.wt_host.size() * sizeof(T) + 256);
    f_dev = (float*)mem.alloc(pk.f_host.size() * sizeof(float) + 256);
    WX_HIP(hipMemcpy(wt_dev, pk.wt_host.data(), pk.wt_host.size() * sizeof(T), hipMemcpyHostToDevice));
    WX_HIP(hipMemcpy(f_dev, pk.f_host.data(), pk.f_host.size() * sizeof(float), hipMemcpyHostToDevice));
    if constexpr (sizeof(T) == 4) {
      if (split_mma) {
        // the split arena: same offsets, same bytes per 32-float chunk -- [hi fragments g = 0..3 | lo fragments g = 0..3], fragment g =
        // the eight k values {4 g .. 4 g + 3, 16 + 4 g .. 16 + 4 g + 3} a lane of k-group g feeds to v_mfma_f32_16x16x32_bf16
        // (the same two 16-byte slots of the fp32 activation row the exact-f32 path reads in its two sub-steps).  Every weight row of
        // a layer with cin % 32 == 0 is a whole number of chunks from a chunk-aligned start (push_w); other layers keep the f32 MFMA.
        while (pk.wt_host.size() % 32) pk.wt_host.push_back(0.f);
        std::vector<uint16_t> sp(pk.wt_host.size() * 2);
        split_encode_chunks(pk.wt_host.data(), pk.wt_host.size(), sp.data());
        mem.release(ws_dev);
        ws_dev = (T*)mem.alloc(sp.size() * sizeof(uint16_t) + 256);
        WX_HIP(hipMemcpy(ws_dev, sp.data(), sp.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        if (!pk.sp16_host.empty()) {
          mem.release(sp16_dev);   // a second wx_finalize_weights: no leak
          sp16_dev = (uint16_t*)mem.alloc(pk.sp16_host.size() * sizeof(uint16_t) + 256);
          WX_HIP(hipMemcpy(sp16_dev, pk.sp16_host.data(), pk.sp16_host.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        }
      }
    }
    alloc_activations();
    finalized = true;
  }

  // ------------------------------------------------------------------ buffers
  DeviceArena mem;   // every device buffer below; freed after ~Engine's body has destroyed the communicator, streams, graphs and events
  T* ws_dev = nullptr;       // split_mma: the weight arena re-encoded as bf16 (hi, lo) fragments, same offsets as wt_dev
  char* xs_planes = nullptr; // split_mma: the packed input as bf16 planes [x_hi | x_lo] (PackParams::split_planar); the patch kernel's third
                             // chunk group wraps around to x_hi (EmbedPatchParams::plane_wrap)
  T* xin = nullptr;          // packed, halo'd input
  T* xin_planar = nullptr;   // chunk-planar copy for the LDS-patch CrossEmbed kernel (wx_embed.h)
  T* cat[3] = {nullptr, nullptr, nullptr};   // [HW_s][2*C_s]: [up-block output | encoder stream]
  T* x3 = nullptr;           // stage-3 stream
  T* scratch = nullptr;      // qkv / FF hidden
  T* attn_o = nullptr;       // attention output before to_out
  T* dtmp[4] = {nullptr, nullptr, nullptr, nullptr};  // decoder temporaries
  T* upbuf = nullptr;        // upsample_v_conv variant: 2x bilinear up-sampled map feeding the 3x3 conv
  T* dec = nullptr;          // up_block4 output [Hd][Wd][ld_dec]
  float2* rowstat = nullptr;
  char* zero_page = nullptr;
  float* embed_tail = nullptr;
  size_t embed_tail_bytes = 0;
  float* splitk_buf = nullptr;   // fp32 partial sums of every split-K form (plain, skinny, hidden-split FeedForward): ONE buffer, sized in
  size_t splitk_bytes = 0;       // alloc_activations from the split rules' own bounds -- the forward never allocates (hipMalloc inside a
                                 // forward would also be illegal under the opt-in graph capture)
  size_t splitk_bound(bool band = false) const {   // band: the wider skinny rule of lat-band ranks (reserved by band_enable only)
    const size_t tile = (size_t)128 * 128 * sizeof(float);
    size_t b = (size_t)512 * tile;                                                               // plain rule: S * tiles <= 512
    b = std::max(b, (size_t)std::max(band ? std::max(opt.skinny_tiles, opt.skinny_tiles_band) : opt.skinny_tiles, 1) * (size_t)std::max(opt.skinny_max, 1) * tile); // skinny rule: tiles <= skinny_tiles, S <= skinny_max
    b = std::max(b, (size_t)std::max(opt.ff_split_tiles, 1) * 128 * 256 * (size_t)std::max(opt.ff_split_max, 1) * sizeof(float));   // <= ff_split_tiles pixel tiles of <= 128 px, C <= 256
    return b;
  }
  float* splitk_scratch(size_t need) {
    if (need > splitk_bytes) throw StateError("split-K scratch: a launch asks for " + std::to_string(need) + " bytes, " + std::to_string(splitk_bytes) + " were reserved (the split rules and splitk_bound() disagree)");
    return splitk_buf;
  }
  float* embed_partial = nullptr;
  size_t embed_partial_bytes = 0;
  int64_t n_gemm8p = 0;              // launches of the last forward that took it
  int64_t n_splitk = 0;              // plain split-K launches (K ranges + finish kernel) of the last forward
  char* stream_sink = nullptr;
  float2* statpart = nullptr;   // [rows][slots] LayerNorm partials written by the producing GEMM epilogue (slots <= 8, or C / 32)
  int64_t statpart_elems = 0;
  float2* stat_dst(int64_t rows, int slots) const {
    if (rows * slots > statpart_elems)
      throw StateError("LayerNorm partials: " + std::to_string(rows) + " rows x " + std::to_string(slots) + " slots exceed the " +
                       std::to_string(statpart_elems) + " reserved");
    return statpart;
  }
  float2* gnpart = nullptr;     // [m_tiles][C] GroupNorm partials written by the 3x3 conv epilogue
  int64_t gnpart_elems = 0;
  int64_t n_attn_blk = 0;       // attention sub-blocks of the last forward that ran on the k-blocked layouts
  int stat_tiles_ready = 0;     // > 0: `statpart` holds partials of the current stream contents (that many per row)
  double* gn_acc = nullptr;
  float *d_mean = nullptr, *d_std = nullptr, *d_lo = nullptr, *d_hi = nullptr;
  bool have_denorm = false, have_tracer = false;
  int tracer_denorm = 0, n_prog = -1, n_static = 0, n_dyn = 0;
  bool acts_ready = false;

  void alloc_activations() {
    if (acts_ready) return;
    const int64_t xin_elems = (int64_t)(Hp + 2 * halo + 2) * (Wp + 2 * halo + 2) * cpad0;
    xin = (T*)mem.alloc(xin_elems * sizeof(T));
    WX_HIP(hipMemset(xin, 0, xin_elems * sizeof(T)));
    if (split_mma && opt.use_patch && sp16_dev) {   // the patch kernel reads the bf16 (hi, lo) planes: no fp32 planar copy in this mode
      xs_planes = (char*)mem.alloc((size_t)xin_elems * 2 * 2);
      WX_HIP(hipMemset(xs_planes, 0, (size_t)xin_elems * 2 * 2));
    } else if (opt.use_patch && opt.planar_xin) {
      xin_planar = (T*)mem.alloc(xin_elems * sizeof(T));
      WX_HIP(hipMemset(xin_planar, 0, xin_elems * sizeof(T)));
    }
    int64_t max_sc = 0, max_ao = 0, max_hw = 0;
    for (int s = 0; s < 4; ++s) {
      const int64_t hw = (int64_t)sh[s] * sw[s];
      if (s < 3) cat[s] = (T*)mem.alloc(hw * 2 * cfg.dim[s] * sizeof(T));
      else x3 = (T*)mem.alloc(hw * cfg.dim[s] * sizeof(T));
      max_sc = std::max(max_sc, hw * 4 * cfg.dim[s]);
      max_ao = std::max(max_ao, hw * cfg.dim[s]);
      max_hw = std::max(max_hw, hw);
    }
    scratch = (T*)mem.alloc(max_sc * sizeof(T));
    attn_o = (T*)mem.alloc(max_ao * sizeof(T));
    int64_t max_dt = 0;
    for (int i = 0; i < 3; ++i) max_dt = std::max(max_dt, (int64_t)sh[2 - i] * sw[2 - i] * ups[i].cout);
    for (int i = 0; i < 4; ++i) dtmp[i] = (T*)mem.alloc(max_dt * sizeof(T));
    if (ps_decoder()) ps4_buf = (T*)mem.alloc((int64_t)Hd * Wd * cpad4 * sizeof(T));
    if (cfg.arch == WX_ARCH_CROSSFORMER_UPCONV) {  // bilinearly up-sampled conv input: largest is up_block4's (Hd x Wd x 2 dim0)
      int64_t m = (int64_t)Hd * Wd * 2 * cfg.dim[0];
      for (int i = 0; i < 3; ++i) m = std::max(m, (int64_t)sh[2 - i] * sw[2 - i] * ups[i].cin);
      upbuf = (T*)mem.alloc(m * sizeof(T));
    }
    dec = (T*)mem.alloc((int64_t)Hd * Wd * ld_dec * sizeof(T));
    WX_HIP(hipMemset(dec, 0, (int64_t)Hd * Wd * ld_dec * sizeof(T)));
    rowstat = (float2*)mem.alloc(max_hw * sizeof(float2));
    // LayerNorm partials: most producers leave <= 8 per row; the weight-stationary GEMM and the attention block kernel leave C / 32
    // (16 at C = 512) -- sized from the largest rows x slots product any stage can ask for, and checked at every producer (stat_dst)
    statpart_elems = max_hw * 8;
    for (int s = 0; s < 4; ++s) statpart_elems = std::max(statpart_elems, (int64_t)sh[s] * sw[s] * std::max(8, cfg.dim[s] / 32));
    statpart = (float2*)mem.alloc(statpart_elems * sizeof(float2));
    gnpart_elems = (int64_t)cdiv(max_hw, 128) * cfg.dim[3];
    gnpart = (float2*)mem.alloc(gnpart_elems * sizeof(float2));
    zero_page = (char*)mem.alloc(256);
    WX_HIP(hipMemset(zero_page, 0, 256));
    stream_sink = (char*)mem.alloc(8192);   // 16 bytes per thread of the widest workgroup (512: wx_gemm8p.h)
    splitk_bytes = splitk_bound();
    splitk_buf = (float*)mem.alloc(splitk_bytes);
    const int cmax = cfg.dim[3];
    gn_acc = (double*)mem.alloc(2 * cmax * sizeof(double));
    d_mean = (float*)mem.alloc(C_out * sizeof(float));
    d_std = (float*)mem.alloc(C_out * sizeof(float));
    d_lo = (float*)mem.alloc(C_out * sizeof(float));
    d_hi = (float*)mem.alloc(C_out * sizeof(float));
    if (cfg.noise_latent_dim > 0) {
      d_noise = (NoiseState*)mem.alloc(sizeof(NoiseState));
      WX_HIP(hipMemset(d_noise, 0, sizeof(NoiseState)));
      d_style = (float*)mem.alloc((size_t)6 * cfg.dim[3] * sizeof(float));
    }
    acts_ready = true;
  }

  // one stage's token stream as a sub-block sees it: the whole map, or in lat-band mode the rows this rank holds in one layout
  struct StageView { int s; T* x; int64_t ld; int h, w; int attn_kind = -1; };   // attn_kind >= 0 replaces AttnL::kind
  StageView whole(int s) const { return {s, s < 3 ? cat[s] + cfg.dim[s] : x3, s < 3 ? 2 * cfg.dim[s] : cfg.dim[s], sh[s], sw[s]}; }
  // lat-band mode: the long layout has its own buffer; the short one sits behind 1 halo row of the concat buffer
  StageView band_view(int s, bool is_long) const {
    if (is_long) return {s, blong[s], cfg.dim[s], bplan.g.rows_long(s, b_rank), sw[s], 2};
    StageView v = whole(s);
    v.x = s < 3 ? bcat[s] + (int64_t)sw[s] * 2 * cfg.dim[s] + cfg.dim[s] : bx3;
    v.h = bplan.g.rows_short(s, b_rank);
    return v;
  }

  // ------------------------------------------------------------------ step glue state
  void set_denorm(const float* mean, const float* stdv, int n) override {
    if (n != C_out) throw ShapeError("wx_set_denorm: n must equal the number of output channels");
    WX_HIP(hipSetDevice(device));
    roll_invalidate();
    need_finalized();
    WX_HIP(hipMemcpy(d_mean, mean, n * sizeof(float), hipMemcpyHostToDevice));
    WX_HIP(hipMemcpy(d_std, stdv, n * sizeof(float), hipMemcpyHostToDevice));
    have_denorm = true;
  }
  void set_tracer(const int32_t* inds, const float* thres, const float* thres_max, int n, int denorm) override {
    WX_HIP(hipSetDevice(device));
    roll_invalidate();
    need_finalized();
    if (n == 0) { have_tracer = false; return; }
    std::vector<float> lo(C_out, -3.4e38f), hi(C_out, 3.4e38f);
    for (int i = 0; i < n; ++i) {
      if (inds[i] < 0 || inds[i] >= C_out) throw ConfigError("tracer index out of range");
      lo[inds[i]] = thres[i];
      if (thres_max) hi[inds[i]] = thres_max[i];
    }
    if (denorm && !have_denorm) throw StateError("wx_set_tracer_fixer(denorm=1) needs wx_set_denorm first");
    WX_HIP(hipMemcpy(d_lo, lo.data(), C_out * sizeof(float), hipMemcpyHostToDevice));
    WX_HIP(hipMemcpy(d_hi, hi.data(), C_out * sizeof(float), hipMemcpyHostToDevice));
    have_tracer = true;
    tracer_denorm = denorm;
  }
  // a14: which input channels the next step takes from y (prognostic), from the forcing tensor (dynamic_forcing) or keeps
  // (static), as explicit groups -- channel_utils.py:140-250 build_channel_layout: with several data sources a field type's
  // channels are contiguous only within a source
  struct LGroup { int kind, x0, src0, n; };   // kind 0 prognostic, 1 dynamic_forcing, 2 fixed
  std::vector<LGroup> lgroups;
  int* d_xmap = nullptr;                       // [C_out] -> input channel, or -1
  void set_layout(int np, int ns, int nd) override {
    if (np < 0 || ns < 0 || nd < 0 || np + ns + nd != C_in / cfg.frames || np > C_out)
      throw ConfigError("wx_set_layout: n_prog + n_static + n_dyn must equal the input channels");
    const int32_t kind[3] = {0, 2, 1}, x0[3] = {0, np, np + ns}, s0[3] = {0, 0, 0}, cnt[3] = {np, ns, nd};
    set_layout_groups(3, kind, x0, s0, cnt);
  }
  void set_layout_groups(int n, const int32_t* kind, const int32_t* x_start, const int32_t* src_start, const int32_t* count) override {
    if (!acts_ready) throw StateError("call wx_finalize_weights before wx_set_layout");
    WX_HIP(hipSetDevice(device));
    roll_invalidate();
    if (n < 0 || (n > 0 && (!kind || !x_start || !src_start || !count))) throw ConfigError("wx_set_layout_groups: null argument");
    const int cx = C_in / cfg.frames;
    std::vector<int> owner(cx, -1), xmap(C_out, -1);
    std::vector<LGroup> gs;
    int np = 0, ns = 0, nd = 0;
    for (int i = 0; i < n; ++i) {
      const LGroup g{kind[i], x_start[i], src_start[i], count[i]};
      if (g.n == 0) continue;
      if (g.kind < 0 || g.kind > 2 || g.n < 0 || g.x0 < 0 || g.x0 + g.n > cx) throw ConfigError("wx_set_layout_groups: group outside the input channels");
      for (int c = g.x0; c < g.x0 + g.n; ++c) {
        if (owner[c] >= 0) throw ConfigError("wx_set_layout_groups: input channel claimed by two groups");
        owner[c] = i;
      }
      if (g.kind == 0) {
        if (g.src0 < 0 || g.src0 + g.n > C_out) throw ConfigError("wx_set_layout_groups: prognostic source outside the output channels");
        for (int k = 0; k < g.n; ++k) {
          if (xmap[g.src0 + k] >= 0) throw ConfigError("wx_set_layout_groups: output channel feeds two input channels");
          xmap[g.src0 + k] = g.x0 + k;
        }
        np += g.n;
      } else if (g.kind == 1) {
        if (g.src0 < 0) throw ConfigError("wx_set_layout_groups: negative forcing offset");
        nd = std::max(nd, g.src0 + g.n);
      } else {
        ns += g.n;
      }
      gs.push_back(g);
    }
    for (int c = 0; c < cx; ++c)
      if (owner[c] < 0) throw ConfigError("wx_set_layout_groups: the groups must cover every input channel");
    if (!d_xmap) d_xmap = (int*)mem.alloc((size_t)C_out * sizeof(int));
    WX_HIP(hipMemcpy(d_xmap, xmap.data(), (size_t)C_out * sizeof(int), hipMemcpyHostToDevice));
    lgroups = gs;
    n_prog = np; n_static = ns; n_dyn = nd;   // n_dyn = channels of the forcing tensor
  }
  // the channels of x_next that do not come from y: fixed groups from x, dynamic-forcing groups from frc (planes of `plane` floats)
  // with_static = false: x_next already holds the fixed planes (the rollout's ping-pong buffers keep them from two steps earlier)
  void copy_layout_groups(const float* x, const float* frc, float* x_next, int64_t plane, hipStream_t s, bool with_static = true) {
    for (const LGroup& g : lgroups) {
      if (g.kind == 2 && !with_static) continue;
      if (g.kind == 2)
        WX_HIP(hipMemcpyAsync(x_next + g.x0 * plane, x + g.x0 * plane, g.n * plane * sizeof(float), hipMemcpyDeviceToDevice, s));
      else if (g.kind == 1)
        WX_HIP(hipMemcpyAsync(x_next + g.x0 * plane, frc + g.src0 * plane, g.n * plane * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
  }
  void need_finalized() const {
    if (!acts_ready) throw StateError("call wx_finalize_weights before configuring the step glue");
  }

  // ------------------------------------------------------------------ profiling + debug
  bool prof_on = false, detail_on = false, family_on = false;
  const char* cur_family = nullptr;   // kernel family of the launch being timed (profile mode 3 appends "@family")
  struct Pending { std::string name; double flops, bytes; int ev; };
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  std::vector<Pending> pending;
  std::map<std::string, KernelStatAcc> stats;
  hipStream_t cur_stream = nullptr;
  int cur_stage = -1;   // appended to kernel-class names while profiling ("gemm_ff1.s2")

  void profile(int on) override { prof_on = on != 0; detail_on = on > 1; family_on = on > 2; }
  int64_t n_split_gemms = 0;         // GEMM launches of the last forward that ran split-bf16 arithmetic
  int64_t n_ff_split_pre = 0;        // ... of which with the out-projection in front (three GEMMs)
  int64_t n_ff_split_post = 0;       // ... of which also with the next to_qkv behind (four GEMMs)
  int64_t n_ff_split_fused = 0;      // ... of which FeedForward sub-blocks in one launch (wx_ff_split.h; counted as two GEMMs above)
  int64_t n_launches = 0;            // timed() calls of the last forward (one per kernel launch or launch + finish pair)
  int64_t attn_nkf_mask = 0;         // bit n: the last forward launched window_attn_kernel with NKF == n key fragments
  int64_t attn_block_nkf_mask = 0;   // ... attn_block_kernel with NKF == n
  bool query(const std::string& key, int64_t* v) override {
    if (key == "launches") { *v = n_launches; return true; }
    if (key == "precision") { *v = sizeof(T) == 2 ? WX_PREC_BF16 : (split_mma ? WX_PREC_FP32_SPLIT : WX_PREC_FP32); return true; }
    if (key == "split_gemms") { *v = n_split_gemms; return true; }
    if (key == "gemm8p_launches") { *v = n_gemm8p; return true; }
    if (key == "splitk_gemms") { *v = n_splitk; return true; }
    if (key == "attn_blk") { *v = n_attn_blk; return true; }
    if (key == "attn_nkf_mask") { *v = attn_nkf_mask; return true; }
    if (key == "attn_block_nkf_mask") { *v = attn_block_nkf_mask; return true; }
    if (key == "ff_split_fused") { *v = n_ff_split_fused; return true; }
    if (key == "ff_split_pre") { *v = n_ff_split_pre; return true; }
    if (key == "ff_split_post") { *v = n_ff_split_post; return true; }
    return false;
  }
  void profile_reset() override { drain(); stats.clear(); }
  void drain() {
    if (pending.empty()) return;
    WX_HIP(hipSetDevice(device));
    for (auto& pd : pending) {
      WX_HIP(hipEventSynchronize(ev_pool[pd.ev].second));
      float ms = 0.f;
      WX_HIP(hipEventElapsedTime(&ms, ev_pool[pd.ev].first, ev_pool[pd.ev].second));
      auto& st = stats[pd.name];
      st.launches += 1; st.ms += ms; st.flops += pd.flops; st.bytes += pd.bytes;
    }
    pending.clear();
  }
  int profile_read(wx_kernel_stat* out, int cap) override {
    drain();
    int i = 0;
    for (auto& kv : stats) {
      if (i >= cap) break;
      std::memset(&out[i], 0, sizeof(wx_kernel_stat));
      std::strncpy(out[i].name, kv.first.c_str(), sizeof(out[i].name) - 1);
      out[i].launches = kv.second.launches; out[i].ms = kv.second.ms;
      out[i].flops = kv.second.flops; out[i].bytes = kv.second.bytes;
      ++i;
    }
    return i;
  }
  template <typename F>
  void timed(const char* name, double flops, double bytes, F&& fn) {
    ++n_launches;
    if (!prof_on) { cur_family = nullptr; fn(); return; }
    const int idx = (int)pending.size();
    while ((int)ev_pool.size() <= idx) {
      hipEvent_t a, b;
      WX_HIP(hipEventCreate(&a)); WX_HIP(hipEventCreate(&b));
      ev_pool.push_back({a, b});
    }
    WX_HIP(hipEventRecord(ev_pool[idx].first, cur_stream));
    fn();
    WX_HIP(hipEventRecord(ev_pool[idx].second, cur_stream));
    std::string nm(name);
    if (detail_on && cur_stage >= 0) nm += ".s" + std::to_string(cur_stage);
    if (family_on && cur_family) nm += std::string("@") + cur_family;
    cur_family = nullptr;
    pending.push_back({nm, flops, bytes, idx});
  }

  PostBlock* post = nullptr;    // not owned
  float* y_internal = nullptr;  // scratch for the normalised output when the caller does not ask for it
  void attach_post(PostBlock* p) override {
    if (band_on) throw StateError("wx_attach_postblock: attach the post block before wx_band_enable");
    if (p && (p->h_full != Ho || p->w != Wo || p->cout != C_out || p->cin * p->fr != C_in || p->fr != cfg.frames))
      throw ConfigError("wx_attach_postblock: post block geometry does not match the model");
    roll_invalidate();
    post = p;
  }
  // forward tail + optional post block + (y_phys, x_next) of one batch item
  void finish_item(const float* x_item, float* y, float* y_phys, float* x_next) {
    if (!post) { tail(y, y_phys, x_next); return; }
    if (!y) {
      if (!y_internal) y_internal = (float*)mem.alloc((size_t)C_out * Ho * Wo * sizeof(float));
      y = y_internal;
    }
    tail(y, nullptr, nullptr);
    timed("post_block", 0.0, 0.0, [&] { post->apply(x_item, y, cur_stream); });
    if (y_phys || x_next) launch_finish(y, (int64_t)Ho * Wo, y_phys, x_next);
  }
  // after the post block: y_phys and the prognostic channels of x_next from the corrected y (planes of `plane` floats)
  void launch_finish(float* y, int64_t plane, float* y_phys, float* x_next) {
    hipLaunchKernelGGL(finish_kernel, dim3(2048), dim3(256), 0, cur_stream, y, plane, C_out, have_denorm ? d_mean : nullptr,
                       have_denorm ? d_std : nullptr, y_phys, x_next, n_prog < 0 ? 0 : n_prog, d_xmap);
    WX_HIP(hipGetLastError());
  }
  // capture level (wx_set_debug): 1 = every activation the reference names, so the routes whose intermediates never reach memory
  // (PRE / POST FeedForward forms, the k-blocked attention chain) step aside; 2 = whatever the default routes leave in memory, the
  // routes themselves untouched
  bool dbg_on = false, dbg_unfuse = false;   // any level; level 1
  struct DbgT { int64_t c, h, w; std::vector<float> data; };
  std::map<std::string, DbgT> dbg;
  void set_debug(int on) override {
    const bool unfuse = on != 0 && on != 2;
    if (on == 0 || unfuse != dbg_unfuse) dbg.clear();   // a level's forward must not answer with another level's captures
    dbg_on = on != 0; dbg_unfuse = unfuse;
  }
  void capture(const std::string& name, const T* base, int h, int w, int c, int64_t ld, int64_t row_pitch_px) {
    if (!dbg_on) return;
    WX_HIP(hipStreamSynchronize(cur_stream));
    std::vector<T> raw((size_t)h * row_pitch_px * ld);
    const size_t used = ((size_t)(h - 1) * row_pitch_px + (w - 1)) * ld + c;  // do not run past a strided view
    WX_HIP(hipMemcpy(raw.data(), base, used * sizeof(T), hipMemcpyDeviceToHost));
    DbgT d;
    d.c = c; d.h = h; d.w = w;
    d.data.resize((size_t)c * h * w);
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x)
        for (int k = 0; k < c; ++k)
          d.data[((size_t)k * h + y) * w + x] = Elem<T>::to_f(raw[((size_t)y * row_pitch_px + x) * ld + k]);
    dbg[name] = std::move(d);
  }
  void debug_read(const char* name, float* out, int64_t cap, int64_t shape[3]) override {
    auto it = dbg.find(name);
    if (it == dbg.end()) throw StateError(std::string("no debug capture named '") + name + "'");
    shape[0] = it->second.c; shape[1] = it->second.h; shape[2] = it->second.w;
    if (out) {
      if (cap < (int64_t)it->second.data.size()) throw ShapeError("debug_read: output buffer too small");
      std::memcpy(out, it->second.data.data(), it->second.data.size() * sizeof(float));
    }
  }

  // ------------------------------------------------------------------ launch helpers
  // K ranges of the plain split-K rule (gemm() below) for a bias-only convolution of `rows` output pixels; 1 = not split
  int plain_split_ways(const ConvW& w, int64_t rows) const {
    if (!opt.split_k || !opt.use_dma || w.n % 128 != 0 || (w.cin * (int)sizeof(T)) % 128 != 0) return 1;
    const int64_t tiles = cdiv(rows, (int64_t)128) * (w.n / 128);
    const int nk = w.kh * w.kw * (w.cin * (int)sizeof(T) / 128);
    int S = (int)std::min<int64_t>(8, 512 / std::max<int64_t>(tiles, 1));
    S = std::min(S, nk / 16);   // at least 16 K steps per range
    return (tiles <= 200 && S >= 2) ? S : 1;
  }
  // One gemm() call: `in` convolved with a layer's weights into `out`.  The defaults are a stride-1 "same" convolution with a bias-only
  // epilogue, so a call names only what differs from that.
  static constexpr int same_pad = INT_MIN;   // pad_y / pad_x: (k - 1) / 2
  // k-blocked [K/32][M][32] exchange of a sub-block chain (bf16, persistent GEMMs): the LayerNorm-folded producer writes its output
  // k-blocked and the residual layer behind it reads its operand k-blocked -- full cache lines per LDS-DMA piece.
  //   hidden: the FeedForward hidden tensor [4C/32][M][32] (ff2 47.9 -> 45.0 us, ff1 56.6 -> 53.8 us)
  //   attn:   q|k|v and the attention output [C/32][M][32] = [head][token][32] at dim_head 32 (to_qkv's stores, the attention's loads and
  //           stores and to_out's operand DMA move full cache lines; row-major: 64-byte halves of lines 3C x 2 bytes apart)
  enum class KBlk { none, hidden, attn };
  struct GemmReq {
    const T* in = nullptr; int in_h = 0, in_w = 0; int64_t in_ld = 0;
    T* out = nullptr; int64_t out_ld = 0;
    int stride = 1, pad_y = same_pad, pad_x = same_pad;
    int out_h = -1, out_w = -1;                   // -1: in_h, in_w
    const float2* rs = nullptr;                   // LayerNorm-folded layer: the statistics of the input rows (stream_stats)
    int act = 0;                                  // 1: GELU
    const T* res = nullptr; int64_t res_ld = 0;   // residual added by the epilogue
    int out_mode = 0, cout = 0;                   // 1: PixelShuffle / ConvTranspose k2 scatter of cout channels; 2: a ConvTranspose k4 ...
    const ConvW* par = nullptr;                   // ... whose four parity weight sets gemm() runs (in one launch when it can) ...
    int py = 0, px = 0;                           // ... each as one parity (py, px) of the output
    KBlk blk = KBlk::none;
    bool want_stats = false;                      // LayerNorm partials of the output rows into `statpart` ...
    int stat_stride = 0, stat_slot0 = 0;          // ... as slots stat_slot0.. of rows of stat_stride slots that several launches share (0: own rows)
    bool want_gn = false;                         // GroupNorm tile partials into `gnpart` ...
    int gn_off = 0;                               // ... after the gn_off tiles earlier launches of the same conv wrote
  };
  struct GemmOut {
    int stat_slots = 0;   // LayerNorm partial slots per row it wrote (0: none)
    int gn_tiles = 0;     // GroupNorm tiles it wrote (0: none)
  };
  enum class Route { gemm8p_conv, gemm8p_convt2, wreg, stream_res, stream_res_lc, stream_ln, conv128 };
  // the kernel a (normalised) request runs on; conv128 is the 128 x 128 implicit-GEMM kernel, every shape's fall-back
  Route gemm_route(const ConvW& w, const GemmReq& r) const {
    if (sizeof(T) != 2 || !opt.use_dma || opt.dbg_flags) return Route::conv128;
    const int64_t rows = (int64_t)r.out_h * r.out_w;
    const bool same_map = r.stride == 1 && r.in_h == r.out_h && r.in_w == r.out_w;
    const bool one = w.kh == 1 && w.kw == 1 && same_map && r.pad_y == 0 && r.pad_x == 0;
    // stride-1 k x k convolutions with a deep K and >= 256 output channels on large maps (the two 3x3 convs of the decoder's first two
    // UpBlocks at 0.25 degrees: K = 4608 / 2304): the eight-phase kernel's conv form (wx_gemm8p.h) -- 127.7 -> 90.1 us and 112.6 -> 102.0 us
    // against the 128 x 128 kernel (tools/gemm8p_probe, profiles/r06_gemm8p_probe_b_conv_form.txt); bitwise the same outputs where the two
    // walk K in the same order.  GroupNorm partials: one per (160-row tile, wave row) = 80 output rows, folded like the 128-row ones.
    if (opt.use_gemm8p && !band_on && w.kh == w.kw && w.kh > 1 && w.kh * w.kw <= 32 && same_map && r.pad_y == (w.kh - 1) / 2 &&
        r.pad_x == (w.kw - 1) / 2 && !r.rs && r.act == 0 && r.out_mode == 0 && !r.want_stats && w.n % 256 == 0 && w.cin % 64 == 0 &&
        (w.kh * w.kw * w.cin) % 128 == 0 && rows >= opt.gemm8p_min_rows && rows * r.in_ld * 2 < (int64_t)0x7fffff00 && gemm8p_fits(rows, w.n, 2, 5, true) &&
        (!r.want_gn || (opt.fuse_ln && (int64_t)(r.gn_off + gemm8p_conv_gn_tiles(rows, w.n)) * w.n <= gnpart_elems)))
      return Route::gemm8p_conv;
    // ConvTranspose k2 s2 (a 1x1 GEMM with N = 4 cout whose epilogue scatters 2 x 2 pixels; the decoder's three UpBlocks): the same
    // kernel's 1x1 form with the scatter in its epilogue -- 33.4 -> 24.6, 59.3 -> 41.9, 63.1 -> 47.3 us at 0.25 degrees, bitwise equal
    if (opt.use_gemm8p && !band_on && one && !r.rs && !r.res && r.act == 0 && r.out_mode == 1 && !r.want_stats && !r.want_gn &&
        r.cout > 0 && w.n == 4 * r.cout && r.cout % 64 == 0 && w.cin % 128 == 0 && rows >= opt.gemm8p_min_rows / 4 && gemm8p_fits(rows, w.n, 2, 5, true))
      return Route::gemm8p_convt2;
    // K = 512 layers on maps of a few thousand rows (a lat-band rank's share of the 0.25-degree stage 2: 2 000 - 4 000 tokens): the
    // weight-stationary kernel (wx_gemm_wreg.h: the wave's weight slice in registers, activations streamed tile by tile, one barrier
    // per tile).  tools/gemm_wreg_probe, M = 2500: to_qkv 11.5 us against 16.1 (persistent kernel) -- at M = 20 000 the two tie, so the
    // unsharded model keeps the persistent kernel.  Bitwise the same outputs; row partials in N / 32 slots instead of N / 128.
    const bool ln_v = r.rs && !r.res && !r.want_stats && w.colsum >= 0, res_v = !r.rs && r.res && r.want_stats && opt.fuse_ln && r.act == 0;
    if (opt.use_wreg && w.wt_kb >= 0 && one && w.cin == 512 && w.n % WREG_BN == 0 && w.bias >= 0 && r.out_mode == 0 && !r.want_gn && r.blk == KBlk::none &&
        rows >= opt.wreg_min_rows && rows < opt.wreg_max_rows && (ln_v || (res_v && w.n / 32 <= WREG_MAXT)) &&
        wreg_gemm_ok(rows, w.n, w.cin, r.rs ? stat_tiles_ready : 0, ln_v))
      return Route::wreg;
    // residual layers with N = 512 / 1024 (to_out, FeedForward layer 2 of stages 2 and 3): the persistent kernel on 160 x 128 tiles, two
    // workgroups per CU (47.9 vs 58.3 us on layer 2, 21.0 vs 23.2 us on to_out; bitwise equal to the 128 x 128 kernel's output) -- with at
    // most one tile per CU and a deep K (stage 3 of the 0.25-degree model) in its loader / consumer form
    if (opt.use_stream && w.wt_kb >= 0 && one && !r.rs && r.res && r.act == 0 && r.out_mode == 0 && r.want_stats && opt.fuse_ln && !r.want_gn &&
        (w.n == 512 || w.n == 1024) && w.bias >= 0 && rows >= opt.stream_min_rows && stream_gemm_ok(rows, w.n, w.cin, 128))
      return opt.use_stream_lc && stream_gemm_lc_pays(rows, w.n, w.cin, 5) ? Route::stream_res_lc : Route::stream_res;
    // LayerNorm-folded 1x1 layers with many rows and K >= 512 (to_qkv, FeedForward layer 1 of stages 2-3): the persistent
    // 128 x 256-tile kernel; measured per shape against the 128 x 128 kernel in tools/gemm_stream_probe
    if (opt.use_stream && w.wt_kb >= 0 && w.n % 256 == 0 && one && r.rs && !r.res && r.out_mode == 0 && !r.want_stats && !r.want_gn &&
        rows >= opt.stream_min_rows && stream_gemm_ok(rows, w.n, w.cin))
      return Route::stream_ln;
    return Route::conv128;
  }
  GemmOut gemm(const char* cls, const ConvW& w, GemmReq r) {
    if (r.out_h < 0) r.out_h = r.in_h;
    if (r.out_w < 0) r.out_w = r.in_w;
    if (r.pad_y == same_pad) r.pad_y = (w.kh - 1) / 2;
    if (r.pad_x == same_pad) r.pad_x = (w.kw - 1) / 2;
    ConvGemmParams p;
    std::memset(&p, 0, sizeof(p));
    p.in = r.in; p.in_h = r.in_h; p.in_w = r.in_w; p.in_ld = r.in_ld; p.cin = w.cin;
    p.kh = w.kh; p.kw = w.kw; p.stride = r.stride; p.pad_y = r.pad_y; p.pad_x = r.pad_x;
    p.out_h = r.out_h; p.out_w = r.out_w;
    p.wt = wt_dev + w.wt; p.n = w.n; p.n_alloc = w.n;
    p.bias = w.bias >= 0 ? f_dev + w.bias : nullptr;
    p.rowstat = r.rs; p.colsum = (r.rs && w.colsum >= 0) ? f_dev + w.colsum : nullptr;
    p.stat_tiles = r.rs ? stat_tiles_ready : 0; p.stat_inv_c = 1.0f / (float)w.cin_true;
    if (r.rs && w.colsum < 0) throw StateError("LayerNorm-folded GEMM without column sums");
    p.act = r.act; p.res = r.res; p.res_ld = r.res_ld; p.out = r.out; p.out_ld = r.out_ld;
    p.out_mode = r.out_mode; p.cout = r.cout; p.py = r.py; p.px = r.px; p.dbg = opt.dbg_flags;
    const bool dma = conv_gemm_is_dma<T>(p, opt.use_dma ? zero_page : nullptr);
    const int64_t rows = (int64_t)r.out_h * r.out_w;
    const double m = (double)rows;
    if constexpr (sizeof(T) == 4) {
      if (split_mma && w.cin % 32 == 0 && !opt.dbg_flags && dma) {
        p.split = 1;
        p.wt = ws_dev + w.wt;
        if (!r.par) ++n_split_gemms;   // a ConvTranspose's outer call only dispatches: its launches are counted where they happen
      }
    }
    const double flops = 2.0 * m * w.n * w.kh * w.kw * w.cin_true * w.flop_frac;
    const double bytes = (m * w.n * (r.res ? 2.0 : 1.0) + (double)r.in_h * r.in_w * w.cin_true + (double)w.n * w.kh * w.kw * w.cin) * sizeof(T);
    const Route route = gemm_route(w, r);
    if constexpr (sizeof(T) == 2) {
      if (route == Route::gemm8p_conv || route == Route::gemm8p_convt2) {
        Gemm8pParams q;
        std::memset(&q, 0, sizeof(q));
        q.a = reinterpret_cast<const bf16_t*>(r.in); q.lda = r.in_ld; q.w = reinterpret_cast<const bf16_t*>(wt_dev + w.wt);
        q.M = (int)rows; q.N = w.n; q.K = w.kh * w.kw * w.cin; q.bias = p.bias;
        q.res = reinterpret_cast<const bf16_t*>(r.res); q.res_ld = r.res_ld;
        q.out = reinterpret_cast<bf16_t*>(r.out); q.out_ld = r.out_ld; q.sink = stream_sink; q.xcd_part = 1;
        cur_family = "gemm8p";
        ++n_gemm8p;
        if (route == Route::gemm8p_convt2) {
          q.scat_w = r.out_w; q.cout = r.cout;
          timed(cls, flops, bytes, [&] { launch_gemm8p_convt2<5>(q, cur_stream); });
          return {};
        }
        q.in_h = r.in_h; q.in_w = r.in_w; q.cin = w.cin; q.kh = w.kh; q.kw = w.kw; q.pad_y = r.pad_y; q.pad_x = r.pad_x;
        q.gn_out = r.want_gn ? gnpart + (int64_t)r.gn_off * w.n : nullptr;
        timed(cls, flops, bytes, [&] { launch_gemm8p_conv(q, cur_stream); });
        return {0, r.want_gn ? gemm8p_conv_gn_tiles(rows, w.n) : 0};
      }
      if (route != Route::conv128) {   // the persistent and weight-stationary kernels: 1x1 layers on the k-blocked weight copy
        StreamGemmParams q;
        std::memset(&q, 0, sizeof(q));
        q.a = reinterpret_cast<const bf16_t*>(r.in); q.lda = r.in_ld; q.w = reinterpret_cast<const bf16_t*>(wt_dev + w.wt_kb);
        q.M = (int)rows; q.N = w.n; q.K = w.cin; q.bias = p.bias; q.colsum = p.colsum;
        q.rowstat = r.rs; q.stat_tiles = p.stat_tiles; q.stat_inv_c = p.stat_inv_c;
        q.res = reinterpret_cast<const bf16_t*>(r.res); q.res_ld = r.res_ld;
        q.out = reinterpret_cast<bf16_t*>(r.out); q.out_ld = r.out_ld; q.sink = stream_sink;
        if (route == Route::wreg) {   // its residual form, or its LayerNorm-folded one
          q.stat_slots = w.n / 32;
          q.stat_out = r.res ? stat_dst(rows, q.stat_slots) : nullptr;
          cur_family = "wreg";
          timed(cls, flops, bytes, [&] { launch_gemm_wreg(q, r.res ? 3 : (r.act == 1 ? 2 : 1), cur_stream); });
          return {r.res ? q.stat_slots : 0, 0};
        }
        if (route == Route::stream_ln) {
          q.o_blk = r.blk != KBlk::none ? 1 : 0; q.o_rows = q.M;
          // tile per epilogue (tools/gemm_stream_probe, MI355X): with GELU the 160-row tile on a 2-stage ring (256 VGPRs, 2 x 54 KB of
          // LDS) wins -- 54.6 / 46.8 us on the stage-2 / stage-3 FeedForward shapes against 56.4 / 58.5 -- without it the 128-row tile
          // on 3 stages does (39.8 vs 46.4 us on to_qkv)
          cur_family = "stream";
          timed(cls, flops, bytes, [&] {
            if (r.act == 1) launch_gemm_stream<5, 2>(q, 2, cur_stream);
            else launch_gemm_stream<4, 3>(q, 1, cur_stream);
          });
          return {};
        }
        q.stat_slots = w.n / 64;
        q.stat_out = stat_dst(rows, q.stat_slots);
        q.a_blk = r.blk != KBlk::none ? 1 : 0; q.a_rows = q.M;
        const bool lc = route == Route::stream_res_lc;
        cur_family = lc ? "stream_lc" : "stream";
        timed(cls, flops, bytes, [&] {
          if (lc) launch_gemm_stream_n128_lc<5, 8>(q, cur_stream);
          else launch_gemm_stream_n128<5, 3, 2>(q, cur_stream);
        });
        return {q.stat_slots, 0};
      }
    }
    if (r.blk == KBlk::hidden) throw StateError("k-blocked hidden tensor requested but the GEMM fell back to the row-major kernel");
    if (r.blk == KBlk::attn) throw StateError("k-blocked q|k|v / attention output requested but the GEMM fell back to the row-major kernel");
    if (r.par) {   // the four parity convs of a ConvTranspose k4 s2 p1 (out_mode 2): one launch when the fast path takes it
      if (opt.merge_parity && dma && !opt.dbg_flags && w.n <= 128) {
        p.n_par = 4;
        for (int q = 0; q < 4; ++q) p.wt_par[q] = (p.split ? ws_dev : wt_dev) + r.par[q].wt;
        const double fl4 = 4.0 * 2.0 * m * w.n * w.kh * w.kw * w.cin_true;
        const double by4 = (4.0 * m * w.n + (double)r.in_h * r.in_w * w.cin_true + 4.0 * w.n * w.kh * w.kw * w.cin) * sizeof(T);
        if (p.split) ++n_split_gemms;   // the merged launch
        timed(cls, fl4, by4, [&] { launch_conv_gemm<T>(p, zero_page, cur_stream, opt.gemm_cfg); });
        return {};
      }
      for (int q = 0; q < 4; ++q) {
        GemmReq rq = r;
        rq.par = nullptr; rq.pad_y = r.pad_y - (q >> 1); rq.pad_x = r.pad_x - (q & 1); rq.py = q >> 1; rq.px = q & 1;
        gemm(cls, r.par[q], rq);
      }
      return {};
    }
    GemmOut o;
    if (r.want_stats && opt.fuse_ln && dma) {
      p.stat_out = statpart;
      p.stat_stride = r.stat_stride; p.stat_slot0 = r.stat_slot0;
    }
    if (r.want_gn && opt.fuse_ln && dma) {
      p.gn_out = gnpart + (int64_t)r.gn_off * w.n;
      o.gn_tiles = (int)cdiv(rows, (int64_t)128);
    }
    // split-K for plain deep-K launches that cannot fill the chip (stage-3 CrossEmbed k = 4: 160 tiles walking K = 8192; every
    // CrossEmbed GEMM of the 1-degree grid): 128 x 128 tiles x S K-ranges, fp32 partial sums, fixed-order finish kernel
    if (!r.rs && !r.res && r.act == 0 && r.out_mode == 0 && !p.gn_out && dma) {
      const int S = plain_split_ways(w, rows);
      if (S >= 2) {
        p.partial = splitk_scratch((size_t)S * rows * w.n * sizeof(float));
        p.k_splits = S;
        ++n_splitk;
      }
    }
    // ... and for the deep-K 1 x 1 layers of the transformer blocks on maps of a few hundred pixels (1-degree grid, stages 2 - 3:
    // 4 - 12 tiles, each walking 16 - 32 K steps alone on its CU at 0.57 us per step): K ranges of >= skinny_steps steps over up to
    // skinny_max workgroups per tile; the finish kernel applies the whole epilogue (LayerNorm fold, GELU, residual, LN partials)
    if (opt.split_k && opt.skinny_max >= 2 && !p.partial && r.out_mode == 0 && !p.gn_out && w.kh == 1 && w.kw == 1 && r.stride == 1 &&
        w.n % 64 == 0 && (w.cin * (int)sizeof(T)) % 128 == 0 && dma && !opt.dbg_flags) {
      const int64_t tiles = (int64_t)cdiv(rows, (int64_t)128) * conv_gemm_n_tiles(w.n);
      const int nk = w.cin * (int)sizeof(T) / 128;
      // (the tiles the wider lat-band rule adds -- more than skinny_tiles of them -- take at most skinny_max_band K ranges: with 8 the fp32
      // partial sums of a rank's stage-2 FeedForward 2, 8 x 2 600 x 512 floats written and read back, cost more than the shorter K walk
      // saves: slowest of 8 ranks 4.51 -> 4.32 ms with 4, 4.42 with 2)
      const int S = std::min((band_on && tiles > opt.skinny_tiles) ? std::min(opt.skinny_max, opt.skinny_max_band) : opt.skinny_max, nk / opt.skinny_steps);
      // lat-band ranks: a rank's share of the 0.25-degree stage 2 is ~80 tiles walking K = 2048 alone (FeedForward layer 2: 40 us) -- the
      // rule tuned on the 1-degree model (<= 32 tiles) is widened there (slowest of 8 ranks 4.62 -> 4.53 ms)
      if (tiles <= (band_on ? std::max(opt.skinny_tiles, opt.skinny_tiles_band) : opt.skinny_tiles) && nk >= opt.skinny_min_nk && S >= 2) {
        p.partial = splitk_scratch((size_t)S * rows * w.n * sizeof(float));
        p.k_splits = S;
      }
    }
    if constexpr (sizeof(T) == 4) {
      // fp32 storage (both arithmetic modes), residual 1 x 1 layers whose 128 x 128 tiles fill the last round of the 512 workgroup slots badly (0.25-degree stage 2:
      // N = 512 -> 628 tiles = 1.23 rounds): 128 x 64 tiles (1 256 of them: 2.45 half-length rounds; three workgroups per CU)
      // (measured, C3: FeedForward 2 of stage 2 2.74 -> 2.36 ms, to_out 1.03 -> 0.88; 64-column tiles EVERYWHERE lose -- to_qkv 1.82 -> 1.99,
      // FeedForward 1 2.59 -> 2.84: half the MFMAs per split activation fragment)
      if (!p.partial && opt.split_bn64 && dma && w.n >= 96 && w.n % 64 == 0 && (w.n <= 512 || !p.stat_out) && r.stat_stride == 0) {
        const int64_t tiles = cdiv(rows, (int64_t)128) * cdiv(w.n, 128);
        const double rounds = (double)tiles / 512.0;
        if (tiles > 512 && rounds < 1.5) p.bn64 = 1;
      }
    }
    timed(cls, flops, bytes, [&] { launch_conv_gemm<T>(p, opt.use_dma ? zero_page : nullptr, cur_stream, opt.gemm_cfg); });
    if (p.stat_out) o.stat_slots = p.partial ? conv_gemm_finish_slots(w.n) : (p.bn64 ? cdiv(w.n, 64) : conv_gemm_n_tiles(w.n));
    return o;
  }
  void upsample2x(const T* in, int h, int w, int64_t in_ld, int c) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int64_t total = (int64_t)4 * h * w * (c / VEC);
    timed("upsample2x", 0.0, (double)5 * h * w * c * sizeof(T), [&] {
      hipLaunchKernelGGL(upsample2x_kernel<T>, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, cur_stream, in, h, w, in_ld, c, upbuf);
      WX_HIP(hipGetLastError());
    });
  }
  void ln_stats(const T* x, int64_t ld, int c, int m) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int pieces = c / VEC;
    const int lpt = pieces >= 64 ? 64 : pieces;
    if (!ln_width_ok(c, (int)sizeof(T))) throw StateError("ln_stats: a width ModelSpec::derive() should have refused");
    const int pix_per_block = 4 * (64 / lpt);
    timed("ln_stats", 0.0, (double)m * c * sizeof(T), [&] {
      hipLaunchKernelGGL(ln_stats_kernel<T>, dim3(cdiv(m, pix_per_block)), dim3(256), 0, cur_stream, x, ld, c, m, 1e-5f, rowstat);
      WX_HIP(hipGetLastError());
    });
  }
  // LayerNorm statistics of the stream: either the partials the last producing GEMM left (stat_tiles_ready > 0)
  // or a fresh two-pass ln_stats launch (stage entry, slow-path producers).
  const float2* stream_stats(const T* x, int64_t ld, int c, int m) {
    if (stat_tiles_ready > 0) return statpart;
    ln_stats(x, ld, c, m);
    return rowstat;
  }
  // ------------------------------------------------------------------ the route of one (attention, FeedForward) pair
  // The fused feed-forward kernel gives every workgroup 128 (C = 128) or 64 (C = 256) pixels: below one workgroup per CU the
  // plain GEMM chain fills the chip better (1-degree model: 45 and 22 workgroups; 507 -> 527 steps/s without the fusion)
  bool ff_big_enough(const StageView& v) const {
    const int64_t m = (int64_t)v.h * v.w;
    // C = 128 on a launch-bound map (1-degree grid stage 1: 45 workgroups): one launch instead of two wins from 40 workgroups on
    // (724 -> 729 steps/s); C = 256 at 23 workgroups loses (710)
    if (cfg.dim[v.s] == 128 || cfg.dim[v.s] == 64) return cdiv(m, 128) >= std::min(opt.ff_min_wgs, 40);
    return cdiv(m, 64) >= opt.ff_min_wgs;
  }
  // split-bf16 precision: the one-launch FeedForward (wx_ff_split.h) of this layer
  bool ff_split_fused_ok(const FFL& f, int c) const {
    return sizeof(T) == 4 && split_mma && opt.ff_split_fused && !opt.dbg_flags && ws_dev && ff_split_supported(c, f.w1.n) && (c == 128 || opt.ff_split_256) && f.w1.cin == c &&
           f.w2.cin == 4 * c && f.w1.kh == 1 && f.w2.kh == 1 && f.w1.bias >= 0 && f.w2.bias >= 0 && f.w1.colsum >= 0;
  }
  // the form of a FeedForward (feedforward() below):
  //   fused       bf16: the one-launch block (wx_ff.h), in its plain, PRE (with the attention's to_out in front) or POST (and the next
  //               attention's LayerNorm + to_qkv behind) form
  //   split       bf16, launch-bound maps: the fused block with its hidden dimension split, and the split-K finish kernel
  //   split_bf16  split-bf16 precision, C = 128 / 256: both layers in one launch (wx_ff_split.h), plain / PRE / POST
  //   chain       ff1 + ff2 on gemm()
  enum class FFForm { fused, split, split_bf16, chain };
  // what attention() and feedforward() run for one pair; plan_pair() is the only place that decides it
  struct PairPlan {
    enum class Attn { vonly, block, chain } attn = Attn::chain;   // wsz == 1: V-only GEMM; wx_attn_block.h; to_qkv -> window_attn -> to_out
    bool qkv_ready = false;     // q|k|v already lie in `scratch` (the previous pair's POST form wrote them)
    bool attn_kblk = false;     // chain on the k-blocked layouts (KBlk::attn)
    FFForm ff = FFForm::chain;
    bool pre = false;           // the attention leaves its output in attn_o; the FeedForward applies to_out + residual itself ...
    bool post = false;          // ... and the next attention's LayerNorm + to_qkv (the next pair's qkv_ready)
    bool hidden_kblk = false;   // chain: hidden tensor k-blocked (KBlk::hidden)
  };
  // A pure function of the layer tables, the view, opt / cfg / precision, band_on and the capture level -- of nothing a launch changes
  // (stat_tiles_ready: the decisions that need it stay where they execute).  Resolved in the order block, pre, form, post, attn_kblk,
  // hidden_kblk: each may use the ones before it (the bf16 `split` form needs `pre` known).
  PairPlan plan_pair(const AttnL& a, const FFL& f, const StageView& v, bool qkv_ready) const {
    const int s = v.s, c = cfg.dim[s];
    const int64_t m = (int64_t)v.h * v.w;
    // the whole attention sub-block in one launch?  (bf16 engine, C = 128 / 256, unsharded maps; q|k|v and the attention output never
    // exist in memory on this path: a debug run captures the sub-block's output only)
    auto block = [&](const AttnL& a) {   // (also asked of the NEXT attention, f.next, by `post`)
      if (sizeof(T) != 2 || !opt.attn_block || band_on || a.bias_tb < 0 || cfg.dim_head != 32) return false;
      if (opt.attn_block == 2) {
        const bool big_s0 = cfg.dim[s] == 128 && attn_nkf(a.wsz) == 7 && (int64_t)(v.h / a.wsz) * (v.w / a.wsz) >= 2048;
        const bool small_map = small_map_tokens(s);   // launch-bound maps (1-degree model): one launch instead of three
        if (!big_s0 && !small_map) return false;
      }
      // 2 x 2 windows: one 16-token fragment per window loses even on launch-bound maps (37 us against 26 for the three launches); four
      // windows per fragment (AttnBlockParams::pack) win there
      if (a.wsz == 2 && !(opt.attn_pack2 && small_map_tokens(s) && ((v.h / 2) * (v.w / 2)) % 4 == 0)) return false;
      return a.wsz > 1 && attn_block_supported(cfg.dim[s], a.wsz, true) &&
             (a.kind == 0 || a.kind == 1) && a.qkv.cin == cfg.dim[s] && a.out.cin == cfg.dim[s];
    };
    PairPlan p;
    p.qkv_ready = qkv_ready;
    p.attn = block(a) ? PairPlan::Attn::block : a.wsz == 1 ? PairPlan::Attn::vonly : PairPlan::Attn::chain;
    if constexpr (sizeof(T) == 2) {
      p.pre = opt.fuse_ff && opt.fuse_out && f.pack_pre >= 0 && !dbg_unfuse && ff_big_enough(v) && cfg.dim_head == 32 && p.attn != PairPlan::Attn::block;
      if (opt.ff_split_max >= 2 && !p.pre && f.pack >= 0 && opt.fuse_ff && opt.fuse_ln && !band_on && !opt.dbg_flags &&
          ff_fused_supported(c, 4 * c) && small_map_tokens(s) && cdiv(m, (int64_t)(c == 128 ? 128 : 64)) <= opt.ff_split_tiles && f.w2.bias >= 0 && f.w1.colsum >= 0)
        p.ff = FFForm::split;
      else if (f.pack >= 0 && opt.fuse_ff && ff_big_enough(v)) p.ff = FFForm::fused;
      p.post = p.pre && opt.fuse_qkv && f.pack_pp >= 0 && !band_on && !(f.next && block(*f.next));
    } else {
      // split-bf16 precision: the one-launch form, whether it also applies the attention's out-projection + residual in front (its PRE
      // form: to_out's launch, the write of x1 by one kernel and its read by the next are gone), and the to_qkv tail (its POST form)
      const bool one = ff_split_fused_ok(f, c);
      if (one) p.ff = FFForm::split_bf16;
      p.pre = one && opt.ff_split_pre && opt.fuse_ln && !dbg_unfuse && !band_on && a.out.cin == c && a.out.n == c && a.out.kh == 1 && a.out.kw == 1 && a.out.bias >= 0;
      if (p.pre && f.next) {
        const ConvW& q = f.next->qkv;
        p.post = one && opt.ff_split_pre && opt.ff_split_post && opt.fuse_ln && !dbg_unfuse && !band_on && f.next->wsz > 1 && q.wt >= 0 && q.cin == c &&
                 q.n == 3 * c && q.kh == 1 && q.kw == 1 && q.bias >= 0 && q.colsum >= 0;
      }
    }
    // C >= 512 on large maps (stages 2 - 3 of the 0.25-degree model): the three launches exchange q|k|v and the attention output
    // k-blocked (see KBlk); outputs bitwise the row-major chain's
    p.attn_kblk = p.attn == PairPlan::Attn::chain && sizeof(T) == 2 && opt.attn_blk_on && opt.use_stream && opt.use_dma && opt.fuse_ln && !opt.dbg_flags && !dbg_unfuse &&
                  !band_on && cfg.dim_head == 32 && !p.qkv_ready && !p.pre && a.qkv.wt_kb >= 0 && a.out.wt_kb >= 0 && (c == 512 || c == 1024) &&
                  m >= opt.stream_min_rows && a.out.bias >= 0 && a.qkv.colsum >= 0 && a.qkv.n % 256 == 0;
    // both layers on the persistent GEMM (stage 2 of the 0.25-degree model): the hidden tensor between them goes k-blocked
    p.hidden_kblk = p.ff == FFForm::chain && sizeof(T) == 2 && opt.use_stream && opt.use_dma && opt.fuse_ln && !opt.dbg_flags && f.w1.wt_kb >= 0 && f.w2.wt_kb >= 0 &&
                    c == 512 && m >= opt.stream_min_rows && f.w2.bias >= 0;
    return p;
  }
  void attention(const AttnL& a, const StageView& v, const std::string& dbg_name, const PairPlan& pl) {
    const int c = cfg.dim[v.s], h = v.h, w = v.w, m = h * w;
    const int64_t ld = v.ld;
    T* x = v.x;
    if constexpr (sizeof(T) == 2) {
      if (pl.attn == PairPlan::Attn::block) {
        AttnBlockParams bp;
        bp.x = reinterpret_cast<bf16_t*>(x); bp.ld = ld;
        bp.wqkv = reinterpret_cast<const bf16_t*>(wt_dev + a.qkv.wt); bp.csq = f_dev + a.qkv.colsum; bp.bq = f_dev + a.qkv.bias;
        bp.wout = reinterpret_cast<const bf16_t*>(wt_dev + a.out.wt); bp.bo = f_dev + a.out.bias;
        bp.tb = f_dev + a.bias_tb; bp.H = h; bp.W = w; bp.wsz = a.wsz; bp.kind = a.kind;
        bp.pack = a.wsz == 2 ? 4 : 1;
        const double n = (double)a.wsz * a.wsz;
        bp.stat_out = opt.fuse_ln && !opt.dbg_flags ? stat_dst(m, c / 32) : nullptr;
        attn_block_nkf_mask |= (int64_t)1 << attn_nkf_tokens(a.wsz * a.wsz * bp.pack);
        timed("attn_block", 8.0 * m * c * c + 4.0 * m * n * c, 2.0 * m * c * sizeof(T), [&] { launch_attn_block(c, bp, cur_stream); });
        stat_tiles_ready = bp.stat_out ? c / 32 : 0;
        capture(dbg_name, x, h, w, c, ld, w);
        return;
      }
    }
    const float2* rs = pl.qkv_ready ? nullptr : stream_stats(x, ld, c, m);
    const KBlk blk = pl.attn_kblk ? KBlk::attn : KBlk::none;
    if (pl.attn == PairPlan::Attn::vonly) {
      gemm("gemm_qkv", a.vonly, {.in = x, .in_h = h, .in_w = w, .in_ld = ld, .out = attn_o, .out_ld = c, .rs = rs});
    } else {
      if (pl.attn_kblk) ++n_attn_blk;
      if (!pl.qkv_ready) gemm("gemm_qkv", a.qkv, {.in = x, .in_h = h, .in_w = w, .in_ld = ld, .out = scratch, .out_ld = 3 * c, .rs = rs, .blk = blk});
      AttnParams p;
      p.trace = nullptr;
      p.qkv = scratch; p.ld_qkv = 3 * c; p.out = attn_o; p.ld_out = c; p.bias = f_dev + a.bias_tab; p.tb = a.bias_tb >= 0 ? f_dev + a.bias_tb : nullptr;
      p.H = h; p.W = w; p.C = c; p.heads = c / cfg.dim_head; p.wsz = a.wsz; p.kind = v.attn_kind >= 0 ? v.attn_kind : a.kind;
      p.scale = (float)(1.0 / std::sqrt((double)cfg.dim_head));   // fp32 engine only: the bf16 engine's q already carries scale * log2(e)
      p.pack = attn_pack(a.wsz);
      p.mma3 = split_mma ? 1 : 0;
      p.blk = blk == KBlk::attn ? 1 : 0;
      const double n = (double)a.wsz * a.wsz;
      attn_nkf_mask |= (int64_t)1 << attn_nkf_tokens(a.wsz * a.wsz * p.pack);
      timed("window_attn", 4.0 * m * n * c, 4.0 * m * c * sizeof(T), [&] {
        if (cfg.dim_head == 32) launch_window_attn<T>(p, cur_stream, opt.attn_split, opt.attn_no_b2);
        else launch_window_attn_any<T>(p, cfg.dim_head, cur_stream);   // [NP][NP] bias table shared by the heads (bias_head_stride 0)
      });
      if (blk != KBlk::attn) capture(dbg_name + ".qkv", scratch, h, w, 3 * c, 3 * c, w);   // (k-blocked: not a [tokens][3C] map)
    }
    if (blk != KBlk::attn) capture(dbg_name + ".attn", attn_o, h, w, c, c, w);
    if (pl.pre) return;   // attn_o stays for the FeedForward
    stat_tiles_ready = gemm("gemm_out", a.out, {.in = attn_o, .in_h = h, .in_w = w, .in_ld = c, .out = x, .out_ld = ld, .res = x, .res_ld = ld,
                                                .blk = blk, .want_stats = true}).stat_slots;
    capture(dbg_name, x, h, w, c, ld, w);
  }
  void feedforward(const AttnL& a, const FFL& f, const StageView& v, const std::string& dbg_name, const PairPlan& pl) {   // a: the pair's attention (PRE form: its to_out)
    const int c = cfg.dim[v.s], h = v.h, w = v.w, m = h * w;
    const int64_t ld = v.ld;
    T* x = v.x;
    const FFForm form = pl.ff;
    const bool pre = pl.pre, post = pl.post;
    if constexpr (sizeof(T) == 2) {
      auto block_params = [&](int64_t pack) {   // the one-launch block's operands
        FFParams fp{};
        fp.x = reinterpret_cast<const bf16_t*>(x); fp.ld = ld; fp.out = reinterpret_cast<bf16_t*>(x); fp.out_ld = ld;
        fp.M = m; fp.hidden = 4 * c; fp.wpack = reinterpret_cast<const char*>(wt_dev + pack);
        fp.cs1 = f_dev + f.w1.colsum; fp.b1 = f_dev + f.w1.bias; fp.b2 = f_dev + f.w2.bias;
        return fp;
      };
      // the fused block with the hidden dimension cut into S ranges over blockIdx.y -- every workgroup streams 1/S of W1 | W2 instead of
      // all of it -- and the split-K finish kernel behind it (+ b2 + residual, rounding, LayerNorm partials): two launches instead of
      // ff1 + ff2 (+ finish)
      auto hidden_split = [&](int64_t pack, int S) {
        const int nch = 4 * c / 32, ch_per = cdiv(nch, S), S_eff = cdiv(nch, ch_per);
        splitk_scratch((size_t)S_eff * m * c * sizeof(float));
        FFParams fp = block_params(pack);
        fp.partial = splitk_buf; fp.ch_per = ch_per;
        ConvGemmParams q;
        std::memset(&q, 0, sizeof(q));
        q.out_h = h; q.out_w = w; q.n = c; q.partial = splitk_buf; q.k_splits = S_eff;
        q.bias = f_dev + f.w2.bias; q.res = x; q.res_ld = ld; q.out = x; q.out_ld = ld; q.stat_out = statpart;
        timed("ff_fused_split", 16.0 * m * c * c, 2.0 * m * c * sizeof(T) + 16.0 * c * c, [&] {
          launch_ff_fused_split(c, fp, zero_page, cur_stream);
          const int64_t waves = (int64_t)m * conv_gemm_finish_slots(c);
          hipLaunchKernelGGL(conv_gemm_finish_kernel<T>, dim3((unsigned)cdiv(waves, (int64_t)4)), dim3(256), 0, cur_stream, q);
          WX_HIP(hipGetLastError());
        });
        stat_tiles_ready = conv_gemm_finish_slots(c);
      };
      if (form == FFForm::fused) {
        FFParams fp = block_params(post ? f.pack_pp : pre ? f.pack_pre : f.pack);
        fp.qkv = post ? reinterpret_cast<bf16_t*>(scratch) : nullptr; fp.ld_qkv = 3 * c;
        fp.csq = post ? f_dev + f.next->qkv.colsum : nullptr; fp.bq = post ? f_dev + f.next->qkv.bias : nullptr;
        fp.o = pre ? reinterpret_cast<const bf16_t*>(attn_o) : nullptr; fp.ld_o = c; fp.bo = pre ? f_dev + a.out.bias : nullptr;
        fp.stat_out = opt.fuse_ln ? statpart : nullptr; fp.dbg = 0;
        timed(post ? "out_ff_qkv_fused" : pre ? "out_ff_fused" : "ff_fused", (post ? 24.0 : pre ? 18.0 : 16.0) * m * c * c, 2.0 * m * c * sizeof(T) + 16.0 * c * c, [&] { launch_ff_fused(c, fp, zero_page, cur_stream, /*px64=*/c == 128 && !pre && opt.ff_small_px64 && cdiv(m, 128) < 128); });
        stat_tiles_ready = opt.fuse_ln ? 1 : 0;
      } else if (form == FFForm::split) {   // launch-bound maps (1-degree grid, C = 128 / 256 stages of 23 - 45 pixel tiles)
        hidden_split(f.pack, std::min(opt.ff_split_max, 4 * c / 32 / 4));
      }
    }
    if constexpr (sizeof(T) == 4) {
      if (form == FFForm::split_bf16) {   // the hidden tensor stays in registers
        const float2* rs = pre ? nullptr : stream_stats(x, ld, c, m);   // the PRE form takes the statistics of x1 itself
        FFSplitParams q{};
        q.x = reinterpret_cast<float*>(x); q.ld = ld; q.M = m; q.hidden = 4 * c;
        q.w1s = reinterpret_cast<const float*>(ws_dev + f.w1.wt); q.b1 = f_dev + f.w1.bias;
        q.w2s = reinterpret_cast<const float*>(ws_dev + f.w2.wt); q.b2 = f_dev + f.w2.bias;
        q.rowstat = rs; q.stat_tiles = pre ? 0 : stat_tiles_ready; q.stat_inv_c = 1.0f / (float)c;
        q.stat_out = opt.fuse_ln ? stat_dst(m, 1) : nullptr;
        if (!pre && q.stat_out && stat_tiles_ready > 1) {
          // the launch would read `statpart` as [M][stat_tiles_ready] in its prologue and write it as [M][1] in its epilogue: workgroup 2j's
          // stores land on the entries workgroup j still has to read, and nothing orders the two (lat-band ranks, WX_NO_FF_SPLIT_PRE,
          // debug captures: the producer was a stand-alone to_out with 2 - 4 slots).  Final statistics through `rowstat` instead.
          ln_stats(x, ld, c, m);
          q.rowstat = rowstat; q.stat_tiles = 0;
        }
        if (pre) {
          q.o = reinterpret_cast<const float*>(attn_o); q.ld_o = c;
          q.wos = reinterpret_cast<const float*>(ws_dev + a.out.wt); q.bo = f_dev + a.out.bias;
          ++n_split_gemms;
          ++n_ff_split_pre;
        }
        if (post) {
          q.qkv = reinterpret_cast<float*>(scratch); q.ld_qkv = 3 * c;
          q.wqs = reinterpret_cast<const float*>(ws_dev + f.next->qkv.wt); q.bq = f_dev + f.next->qkv.bias;
          ++n_split_gemms;
          ++n_ff_split_post;
        }
        n_split_gemms += 2;
        ++n_ff_split_fused;
        timed(post ? "out_ff_qkv_split_fused" : pre ? "out_ff_split_fused" : "ff_split_fused", (post ? 24.0 : pre ? 18.0 : 16.0) * m * c * c,
              (post ? 6.0 : pre ? 3.0 : 2.0) * m * c * sizeof(T) + (post ? 12.0 : pre ? 9.0 : 8.0) * c * c * sizeof(T), [&] { launch_ff_split(c, q, cur_stream, opt.ff_split_tw ? opt.ff_split_tw : (cdiv(m, 128) >= 512 ? 2 : 1)); });
        stat_tiles_ready = q.stat_out ? 1 : 0;
      }
    }
    if (form == FFForm::chain) {
      const float2* rs = stream_stats(x, ld, c, m);
      const KBlk blk = pl.hidden_kblk ? KBlk::hidden : KBlk::none;
      gemm("gemm_ff1", f.w1, {.in = x, .in_h = h, .in_w = w, .in_ld = ld, .out = scratch, .out_ld = 4 * c, .rs = rs, .act = 1, .blk = blk});
      stat_tiles_ready = gemm("gemm_ff2", f.w2, {.in = scratch, .in_h = h, .in_w = w, .in_ld = 4 * c, .out = x, .out_ld = ld, .res = x, .res_ld = ld,
                                                 .blk = blk, .want_stats = true}).stat_slots;
    }
    capture(dbg_name, x, h, w, c, ld, w);
  }
  // -> gn_acc[2c] (sum, sum sq) in fp64; tiles > 0: the producing conv's epilogue left that many per-tile (sum, sum sq) in gnpart
  void gn_local_stats(const T* x, int c, int64_t m, int tiles) {
    constexpr int VEC = 16 / (int)sizeof(T);
    if (!gn_width_ok(c, (int)sizeof(T))) throw StateError("gn_stats: a width ModelSpec::derive() should have refused");
    if (tiles > 0) {  // just fold them
      timed("gn_stats", 0.0, (double)tiles * c * 8.0, [&] {
        hipLaunchKernelGGL(gn_fold_partials_kernel, dim3(c), dim3(256), 0, cur_stream, gnpart, tiles, c, gn_acc);
        WX_HIP(hipGetLastError());
      });
    } else {
      WX_HIP(hipMemsetAsync(gn_acc, 0, 2 * c * sizeof(double), cur_stream));
      const int rows_per_block = 256 / (c / VEC);
      int blocks = (int)std::min<int64_t>(2048, (m + rows_per_block - 1) / rows_per_block);
      timed("gn_stats", 0.0, (double)m * c * sizeof(T), [&] {
        hipLaunchKernelGGL(gn_stats_kernel<T>, dim3(blocks), dim3(256), 2 * c * sizeof(double), cur_stream, x, (int64_t)c, c, m, gn_acc);
        WX_HIP(hipGetLastError());
      });
    }
  }
  // gn_acc over m_count pixels (the whole map) -> per-channel affine; applied to the m rows at x
  void gn_finalize_apply(const T* x, int c, int64_t m, int64_t m_count, int64_t g_off, int64_t b_off, const T* res, int64_t res_ld, T* out,
                         int64_t out_ld, int fold_tiles = 0) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int64_t total = m * (c / VEC);
    int ablocks = (int)std::min<int64_t>(2048, (total + 255) / 256);   // one resident round: every workgroup derives the affine once
    if (fold_tiles > 0) ablocks = std::min(ablocks, 256);              // ... and, folding the partials itself, reads tiles x C x 8 bytes first
    const size_t lds = 2 * c * sizeof(float) + (fold_tiles > 0 ? 2 * c * sizeof(double) : 0);
    timed("gn_apply", 0.0, (double)m * c * sizeof(T) * (res ? 3.0 : 2.0), [&] {
      hipLaunchKernelGGL(gn_apply_kernel<T>, dim3(ablocks), dim3(256), lds, cur_stream, x, (int64_t)c, c, m, gn_acc, f_dev + g_off,
                         f_dev + b_off, cfg.dim[0], (double)m_count, 1e-5f, res, res_ld, out, out_ld, fold_tiles > 0 ? gnpart : nullptr, fold_tiles);
      WX_HIP(hipGetLastError());
    });
  }
  void group_norm_silu(const T* x, int c, int64_t m, int64_t g_off, int64_t b_off, const T* res, int64_t res_ld, T* out,
                       int64_t out_ld, int tiles) {   // tiles: the producing conv's GroupNorm partials (gn_local_stats)
    if (tiles > 0 && tiles <= opt.gn_fold_max_tiles) {   // few tiles: the apply kernel folds the partials itself (one launch instead of two)
      gn_finalize_apply(x, c, m, m, g_off, b_off, res, res_ld, out, out_ld, tiles);
      return;
    }
    gn_local_stats(x, c, m, tiles);
    gn_finalize_apply(x, c, m, m, g_off, b_off, res, res_ld, out, out_ld);
  }

  // ------------------------------------------------------------------ forward
  // a1: padded rows [row0, row0 + nrows) of the earth-padded grid -> buffer rows dst_row.. of `dst` (Hb buffer rows);
  // `x` holds input rows [src_row0, src_row0 + src_rows) of every channel (the whole grid outside lat-band mode)
  void pack_input(const float* x, T* dst, T* dst_planar, int Hb, int row0, int nrows, int dst_row, int src_row0, int src_rows) {
    PackParams p;
    p.x = x; p.dst = dst; p.C = C_in_model; p.H = cfg.image_height; p.W = cfg.image_width;
    p.p0 = cfg.pad_activate ? cfg.pad_lat[0] : 0; p.p1 = cfg.pad_activate ? cfg.pad_lat[1] : 0;
    p.pl = cfg.pad_activate ? cfg.pad_lon[0] : 0; p.pr = cfg.pad_activate ? cfg.pad_lon[1] : 0;
    p.halo = halo; p.cpad = cpad0; p.dst_planar = dst_planar; p.Hb = Hb;
    p.row0 = row0; p.src_row0 = src_row0; p.src_rows = src_rows; p.dst_row = dst_row;
    p.mirror = cfg.pad_activate == 2;
    p.split_planar = (split_mma && dst == xin && xs_planes) ? xs_planes : nullptr;
    if (nrows <= 0) return;
    // channel group = all of cpad0 while its [cg][65] fp32 tile stays under 64 KB of LDS; block origin shifted so that the 256-byte source
    // runs of the interior rows are line-aligned (wx_elem.h)
    const int cg = std::min(cpad0, 224);
    const int xshift = opt.pack_align ? (64 - p.pl % 64) % 64 : 0;
    timed("pack_input", 0.0, (double)C_in * nrows * cfg.image_width * 4.0 + (double)nrows * Wp * cpad0 * sizeof(T), [&] {
      // camulator at frames == 2: the same launch reads both frames of x [C_in_model][2][H][W] and packs their mean
      if (avg_frames()) hipLaunchKernelGGL((pack_input_kernel<T, true>), dim3(cdiv(Wp + xshift, 64), nrows), dim3(256), (size_t)cg * 65 * sizeof(float), cur_stream, p, cg, xshift);
      else hipLaunchKernelGGL(pack_input_kernel<T>, dim3(cdiv(Wp + xshift, 64), nrows), dim3(256), (size_t)cg * 65 * sizeof(float), cur_stream, p, cg, xshift);
      WX_HIP(hipGetLastError());
    });
  }
  // a2: the CrossEmbed of stage s.  `in` = stage-0: packed input buffer of Hb rows (xin layout); later stages: rows of the
  // previous stream, in_h of them, whose first row is row `in_row0` relative to stride*first-output-row (0 for the whole map,
  // -emb_lo in lat-band mode where the conv halo is materialised).
  void cross_embed(const StageView& v, const T* in, const T* in_planar, int in_h, int in_row0, int64_t in_ld_s) {
    const int s = v.s;
    const StageL& st = stages[s];
    T* x = v.x;
    const int64_t ld = v.ld;
    if (v.h <= 0) return;
    int choff = 0;
    if (s >= 1 && st.merged.wt >= 0 && opt.embed_merge && !band_on) {
      const int k = st.embed_k.back(), stv = cfg.embed_strides[s], pd = (k - stv) / 2;
      // ... which also leaves the LayerNorm partials of its rows for the stage's first sub-block
      stat_tiles_ready = gemm("gemm_embed", st.merged, {.in = in, .in_h = in_h, .in_w = sw[s - 1], .in_ld = in_ld_s, .out = x, .out_ld = ld, .stride = stv,
                                                        .pad_y = pd + in_row0, .pad_x = pd, .out_h = v.h, .out_w = v.w, .want_stats = true}).stat_slots;
      return;
    }
    // stages 1-3: every branch's epilogue (or split-K finish) leaves the LayerNorm partials of ITS channel range in the shared row of
    // `statpart` -- the stage's first sub-block then needs no ln_stats launch (slot counts are predicted here and checked after each launch)
    int slots[8] = {0}, total_slots = 0;
    bool share = s >= 1 && opt.fuse_ln && opt.use_dma && !band_on && !opt.dbg_flags && opt.stat_share && st.embed.size() <= 8;
    for (size_t b = 0; share && b < st.embed.size(); ++b) {
      const ConvW& w = st.embed[b];
      slots[b] = plain_split_ways(w, (int64_t)v.h * v.w) > 1 ? conv_gemm_finish_slots(w.n) : conv_gemm_n_tiles(w.n);
      total_slots += slots[b];
    }
    share = share && total_slots <= 8;
    bool all_made = share;
    int slot_at = 0;
    for (size_t b = 0; b < st.embed.size(); ++b) {
      const int k = st.embed_k[b], stv = cfg.embed_strides[s], pd = (k - stv) / 2;
      const bool patch_on = s == 0 && opt.use_patch && st.embed_k.back() == 32 && st.patch.back().wt >= 0 && st.patch_tab >= 0;
      if (patch_on && k == 4 && st.ride4) { choff += st.embed[b].n; continue; }   // computed by the patch kernel's spare accumulator rows
      if (patch_on && st.patch[b].wt >= 0) {
        if (k != 32) { choff += st.embed[b].n; continue; }  // rides along in the fused launch issued with k = 32
        EmbedPatchParams ep;
        std::memset(&ep, 0, sizeof(ep));
        ep.xin = in; ep.xin_planar = in_planar; ep.Hb = in_h; ep.Wb = Wp + 2 * halo; ep.cpad = cpad0; ep.org = halo - 15;
        ep.out_ld = ld; ep.out_h = v.h; ep.out_w = v.w; ep.dbg = opt.dbg_flags;
        ep.slot_tab = f_dev + st.patch_tab; ep.bias64 = f_dev + st.patch_bias64; ep.out_row = x;
        double fl = 0.0;
        int off = 0;
        for (size_t j = 0; j < st.embed.size(); ++j) {
          const PatchW& pw = st.patch[j];
          const int kj = st.embed_k[j];
          if (pw.wt >= 0) {
            fl += 2.0 * v.h * v.w * pw.n * kj * kj * C_in_model;
            if (kj == 32) ep.wt32 = wt_dev + pw.wt;
            if (kj == 16) ep.wt16 = wt_dev + pw.wt;
            if (kj == 8) ep.wt8 = wt_dev + pw.wt;
          } else if (kj == 4 && st.ride4) {
            fl += 2.0 * v.h * v.w * st.embed[j].n * kj * kj * C_in_model;
          }
          off += st.embed[j].n;
        }
        // small maps (1-degree grid, lat-band ranks): the serial walk over the channel chunks bounds the launch -> split it four
        // ways over blockIdx.y, fp32 partial sums, fixed-order finish kernel
        const int chunks0 = cpad0 / (16 / (int)sizeof(T));
        if (opt.embed_split && embed_patch_small_map(v.h, v.w, opt.dbg_flags) && chunks0 >= 8) {
          const int n_split = opt.embed_split_ways;
          const size_t need = (size_t)n_split * v.h * v.w * 64 * sizeof(float);
          if (need > embed_partial_bytes) {
            embed_partial = (float*)mem.alloc(need);   // grows at most a few times (batch / band geometry); the arena frees the older ones at destroy
            embed_partial_bytes = need;
          }
          ep.partial = embed_partial;
          ep.chunk_per = cdiv(chunks0, n_split);
        } else if (opt.embed_tail_split && !opt.dbg_flags) {
          // big maps: the partly filled last round of tiles (0.25 degrees: 125 of 625) runs as ONE round of half-chunk workgroups
          const int tail = embed_patch_tail_rows(v.h, v.w, chunks0);
          if (tail > 0) {
            const size_t need = (size_t)2 * tail * v.w * 64 * sizeof(float);
            if (need > embed_tail_bytes) { embed_tail = (float*)mem.alloc(need); embed_tail_bytes = need; }
            ep.tail_partial = embed_tail;
          }
        }
        const bool split_patch = split_mma && xs_planes && in == xin && !opt.dbg_flags;
        if (split_patch) {   // the bf16 kernel over the K-concatenated (hi, lo) operands, fp32 out
          ep.xin = nullptr; ep.xin_planar = xs_planes; ep.cpad = 3 * cpad0; ep.plane_wrap = 2 * cpad0 / 8;   // chunks [2n, 3n) re-read the x_hi planes
          ep.wt32 = ep.wt16 = ep.wt8 = nullptr;
          for (size_t j = 0; j < st.embed.size(); ++j) {
            const PatchW& pw = st.patch[j];
            if (pw.wt16 < 0) continue;
            if (st.embed_k[j] == 32) ep.wt32 = sp16_dev + pw.wt16;
            if (st.embed_k[j] == 16) ep.wt16 = sp16_dev + pw.wt16;
            if (st.embed_k[j] == 8) ep.wt8 = sp16_dev + pw.wt16;
          }
          if (ep.chunk_per) ep.chunk_per = cdiv(3 * cpad0 / 8, opt.embed_split_ways);
          ++n_split_gemms;
        }
        timed("embed_patch", fl, (double)(in_h * Wp) * cpad0 * sizeof(T) + (double)v.h * v.w * 64 * sizeof(T), [&] {
          if constexpr (sizeof(T) == 4) {
            if (split_patch) { launch_embed_patch<bf16_t, float>(ep, zero_page, cur_stream); return; }
          }
          launch_embed_patch<T>(ep, zero_page, cur_stream);
        });
      } else if (s == 0) {
        // the branch that does not ride in the patch kernel (k = 4 of the 0.25-degree model: 64 channels, its own implicit GEMM)
        gemm("gemm_embed", st.embed[b], {.in = in, .in_h = in_h, .in_w = Wp + 2 * halo, .in_ld = cpad0, .out = x + choff, .out_ld = ld, .stride = stv,
                                         .pad_y = pd - halo, .pad_x = pd - halo, .out_h = v.h, .out_w = v.w});
      } else {
        const int made = gemm("gemm_embed", st.embed[b], {.in = in, .in_h = in_h, .in_w = sw[s - 1], .in_ld = in_ld_s, .out = x + choff, .out_ld = ld,
                                                          .stride = stv, .pad_y = pd + in_row0, .pad_x = pd, .out_h = v.h, .out_w = v.w, .want_stats = share,
                                                          .stat_stride = share ? total_slots : 0, .stat_slot0 = share ? slot_at : 0}).stat_slots;
        if (share && made && made != slots[b]) throw StateError("cross_embed: LayerNorm partial slots of a branch differ from the prediction");
        all_made = all_made && made > 0;
        slot_at += slots[b];
      }
      choff += st.embed[b].n;
    }
    if (share) stat_tiles_ready = all_made ? total_slots : 0;
  }
  // a4-a7: the transformer blocks of stage s on the rows the stream currently holds
  void stage_blocks(int s) {
    const StageL& st = stages[s];
    const StageView v = whole(s);
    const std::string sp = "layers." + std::to_string(s);
    bool qkv_made = false;  // the previous fused kernel already produced this attention's q|k|v
    for (size_t d = 0; d < st.blocks.size(); ++d) {
      const std::string bp = sp + ".1.layers." + std::to_string(d);
      const BlockL& bl = st.blocks[d];
      const PairPlan p = plan_pair(bl.sa, bl.sf, v, qkv_made);
      attention(bl.sa, v, bp + ".0", p);
      feedforward(bl.sa, bl.sf, v, bp + ".1", p);
      const PairPlan q = plan_pair(bl.la, bl.lf, v, p.post);
      attention(bl.la, v, bp + ".2", q);
      feedforward(bl.la, bl.lf, v, bp + ".3", q);
      qkv_made = q.post;
    }
  }
  void block_half(const StageView& v, int d, bool long_half) {   // lat-band mode: one (attention, feed-forward) pair
    if (v.h <= 0) return;
    const BlockL& bl = stages[v.s].blocks[d];
    const AttnL& a = long_half ? bl.la : bl.sa;
    const FFL& f = long_half ? bl.lf : bl.sf;
    const PairPlan p = plan_pair(a, f, v, false);
    attention(a, v, "", p);
    feedforward(a, f, v, "", p);
  }
  // ------------------------------------------------------------------ ensemble noise (wx_noise.h)
  // tape entries of slot l in the reference's draw order: per active layer (latent, pixel), or one latent first when correlated
  int tape_index(int l, bool latent) const {
    int e = 0;
    for (int k = 0; k < l; ++k) e += noise_slot_on(k);
    if (cfg.noise_correlated) return latent ? 0 : 1 + e;
    return 2 * e + (latent ? 0 : 1);
  }
  int tape_count() const {
    int e = 0;
    for (int k = 0; k < 6; ++k) e += noise_slot_on(k);
    return cfg.noise_correlated ? 1 + e : 2 * e;
  }
  void noise_styles() {
    NoiseStyleParams p{};
    for (int l = 0; l < 6; ++l) {
      if (!noise_slot_on(l)) continue;
      p.w[l] = f_dev + nz[l].w;
      p.bias[l] = f_dev + nz[l].b;
      p.C[l] = noise_channels(l);
      if (!noise_tape.empty()) p.tape_z[l] = noise_tape[tape_index(l, true)] + (int64_t)cur_row * cfg.noise_latent_dim;
    }
    p.style = d_style; p.cstride = cfg.dim[3]; p.Dn = cfg.noise_latent_dim; p.correlated = cfg.noise_correlated; p.row = cur_row;
    p.st = d_noise;
    const size_t lds = (size_t)((cfg.noise_latent_dim + 3) / 4) * 4 * sizeof(float);
    timed("noise_style", 2.0 * cfg.noise_latent_dim * (2 * cfg.dim[0] + 2 * cfg.dim[1] + 2 * cfg.dim[2]), 0.0, [&] {
      hipLaunchKernelGGL(noise_style_kernel, dim3(6), dim3(256), lds, cur_stream, p);
      WX_HIP(hipGetLastError());
    });
  }
  void noise_inject(int l, T* x, int64_t ld, int h, int w) {
    const int c = noise_channels(l);
    constexpr int VEC = 16 / (int)sizeof(T);
    if (c % VEC || ld % VEC) throw ConfigError("noise layer width must be a multiple of the 16-byte vector");
    if ((int64_t)c * h * w >= (int64_t)1 << 34) throw ConfigError("noise layer larger than 2^34 elements (32-bit quad counter)");
    NoiseInjectParams<T> p{};
    p.x = x; p.ld = ld; p.HW = h * w; p.C = c;
    p.style = d_style + l * cfg.dim[3]; p.nf = f_dev + nz[l].nf; p.mod = f_dev + nz[l].mod;
    p.tape = noise_tape.empty() ? nullptr : noise_tape[tape_index(l, false)] + (int64_t)cur_row * c * h * w;
    p.st = d_noise; p.slot = l; p.row = cur_row;
    const int64_t total = (int64_t)cdiv((int64_t)h * w, 4) * (c / VEC);
    const int blocks = (int)std::min<int64_t>(cdiv(total, 256), 8192);
    timed("noise_inject", 0.0, 2.0 * (double)h * w * c * sizeof(T), [&] {
      hipLaunchKernelGGL(noise_inject_kernel<T>, dim3(blocks), dim3(256), 0, cur_stream, p);
      WX_HIP(hipGetLastError());
    });
  }
  void noise_next_step() {   // after every forward / step: the next one draws new noise (a captured graph replays this too)
    if (cfg.noise_latent_dim <= 0) return;
    timed("noise_step", 0.0, 0.0, [&] {
      hipLaunchKernelGGL(noise_step_kernel, dim3(1), dim3(64), 0, cur_stream, d_noise);
      WX_HIP(hipGetLastError());
    });
  }
  void set_noise(uint64_t seed, int member0, int step) override {
    if (cfg.noise_latent_dim <= 0) throw ConfigError("wx_set_noise: the model has no noise layers (noise_latent_dim = 0)");
    if (!acts_ready) throw StateError("wx_set_noise: finalize the weights first");
    if (member0 < 0 || step < 0) throw ConfigError("wx_set_noise: member0 and step must be >= 0");
    WX_HIP(hipSetDevice(device));
    const NoiseState st{(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), member0, step};
    WX_HIP(hipDeviceSynchronize());   // forwards / graph replays in flight read the state
    WX_HIP(hipMemcpy(d_noise, &st, sizeof(st), hipMemcpyHostToDevice));
  }
  void set_noise_tape(const float* const* draws, int n) override {
    if (cfg.noise_latent_dim <= 0) throw ConfigError("wx_set_noise_tape: the model has no noise layers (noise_latent_dim = 0)");
    roll_invalidate();   // captured graphs bake the draw pointers in
    if (!draws) { noise_tape.clear(); return; }
    if (n != tape_count())
      throw ConfigError("wx_set_noise_tape: expected " + std::to_string(tape_count()) + " draw tensors, got " + std::to_string(n));
    for (int i = 0; i < n; ++i)
      if (!draws[i]) throw ConfigError("wx_set_noise_tape: NULL draw pointer");
    noise_tape.assign(draws, draws + n);
  }
  void core(const float* x_item) {
    n_gemm8p = 0;
    n_splitk = 0;
    n_attn_blk = 0;
    n_split_gemms = 0;
    n_ff_split_fused = 0;
    n_ff_split_pre = 0;
    n_ff_split_post = 0;
    n_launches = 0;
    attn_nkf_mask = 0;
    attn_block_nkf_mask = 0;
    // a1: pack + earth halo
    pack_input(x_item, xin, xin_planar, Hp + 2 * halo, 0, Hp, halo, 0, cfg.image_height);
    capture("pad", xin + ((int64_t)halo * (Wp + 2 * halo) + halo) * cpad0, Hp, Wp, C_in_model, cpad0, Wp + 2 * halo);
    if (cfg.noise_latent_dim > 0) noise_styles();
    // encoder
    for (int s = 0; s < 4; ++s) {
      cur_stage = s;
      stat_tiles_ready = 0;  // the CrossEmbed output has no partials yet
      const StageView v = whole(s);
      if (s == 0) cross_embed(v, xin, xin_planar, Hp + 2 * halo, 0, 0);
      else cross_embed(v, whole(s - 1).x, nullptr, sh[s - 1], 0, whole(s - 1).ld);
      const std::string sp = "layers." + std::to_string(s);
      capture(sp + ".0", v.x, v.h, v.w, cfg.dim[s], v.ld, v.w);
      stage_blocks(s);
      capture(sp + ".1", v.x, v.h, v.w, cfg.dim[s], v.ld, v.w);
      if (s < 3 && noise_slot_on(s)) {   // in place: the noisy map is both the skip and the next stage's input
        noise_inject(s, v.x, v.ld, v.h, v.w);
        capture(noise_prefix(s), v.x, v.h, v.w, cfg.dim[s], v.ld, v.w);
      }
    }
    // decoder
    stat_tiles_ready = 0;
    for (int i = 0; i < 3; ++i) {
      cur_stage = 4 + i;
      const UpL& u = ups[i];
      const int si = 3 - i;             // input stage map
      const int so = 2 - i;             // output stage map
      const T* in = (i == 0) ? x3 : cat[si];
      const int64_t in_ld = (i == 0) ? cfg.dim[3] : 2 * cfg.dim[si];
      const int64_t mo = (int64_t)sh[so] * sw[so];
      T *scut = dtmp[0], *ta = dtmp[1], *tb = dtmp[2];
      // the block's stored intermediates, captured behind the launch that wrote them (ta is written twice); no route depends on them
      const std::string up = "up_block" + std::to_string(i + 1);
      auto cap_mid = [&](const char* what, const T* buf, int c) { capture(up + what, buf, sh[so], sw[so], c, c, sw[so]); };
      if (ps_decoder()) {
        // x = PixelShuffle(conv3x3(x)); x = x + sharp(x)   (wxformer/crossformer.py:157-158)
        gemm("gemm_convPS", u.convps, {.in = in, .in_h = sh[si], .in_w = sw[si], .in_ld = in_ld, .out = dtmp[3], .out_ld = u.cout, .out_mode = 1,
                                       .cout = u.cout});
        cap_mid(".ps", dtmp[3], u.cout);
        gemm("gemm_conv3", u.sharp, {.in = dtmp[3], .in_h = sh[so], .in_w = sw[so], .in_ld = u.cout, .out = scut, .out_ld = u.cout, .res = dtmp[3],
                                     .res_ld = u.cout});
      } else if (cfg.arch == WX_ARCH_CROSSFORMER_UPCONV) {
        upsample2x(in, sh[si], sw[si], in_ld, u.cin);
        cap_mid(".us", upbuf, u.cin);
        gemm("gemm_conv3", u.upc, {.in = upbuf, .in_h = sh[so], .in_w = sw[so], .in_ld = u.cin, .out = scut, .out_ld = u.cout});
      } else {
        gemm("gemm_convT2", u.convt, {.in = in, .in_h = sh[si], .in_w = sw[si], .in_ld = in_ld, .out = scut, .out_ld = u.cout, .out_mode = 1, .cout = u.cout});
      }
      cap_mid(".up", scut, u.cout);
      int tiles = gemm("gemm_conv3", u.c1, {.in = scut, .in_h = sh[so], .in_w = sw[so], .in_ld = u.cout, .out = ta, .out_ld = u.cout, .want_gn = true}).gn_tiles;
      cap_mid(".c1", ta, u.cout);
      group_norm_silu(ta, u.cout, mo, u.g1, u.b1, nullptr, 0, tb, u.cout, tiles);
      cap_mid(".n1", tb, u.cout);
      tiles = gemm("gemm_conv3", u.c2, {.in = tb, .in_h = sh[so], .in_w = sw[so], .in_ld = u.cout, .out = ta, .out_ld = u.cout, .want_gn = true}).gn_tiles;
      cap_mid(".c2", ta, u.cout);
      group_norm_silu(ta, u.cout, mo, u.g2, u.b2, scut, u.cout, cat[so], 2 * cfg.dim[so], tiles);
      capture(up, cat[so], sh[so], sw[so], u.cout, 2 * cfg.dim[so], sw[so]);
      if (noise_slot_on(3 + i)) {       // before the concat: the up block's half of cat[so]
        noise_inject(3 + i, cat[so], 2 * cfg.dim[so], sh[so], sw[so]);
        capture(noise_prefix(3 + i), cat[so], sh[so], sw[so], u.cout, 2 * cfg.dim[so], sw[so]);
      }
    }
    cur_stage = 7;
    if (ps_decoder()) {
      gemm("gemm_convPS", ps4, {.in = cat[0], .in_h = sh[0], .in_w = sw[0], .in_ld = 2 * cfg.dim[0], .out = ps4_buf, .out_ld = cpad4, .out_mode = 1,
                                .cout = cpad4});
      capture("up_block4.ps", ps4_buf, Hd, Wd, C_out, cpad4, Wd);
      gemm("gemm_conv3", fin4, {.in = ps4_buf, .in_h = Hd, .in_w = Wd, .in_ld = cpad4, .out = dec, .out_ld = ld_dec});
    } else if (cfg.arch == WX_ARCH_CROSSFORMER_UPCONV) {
      upsample2x(cat[0], sh[0], sw[0], 2 * cfg.dim[0], 2 * cfg.dim[0]);
      capture("up_block4.us", upbuf, Hd, Wd, 2 * cfg.dim[0], 2 * cfg.dim[0], Wd);
      gemm("gemm_conv3", up4c, {.in = upbuf, .in_h = Hd, .in_w = Wd, .in_ld = 2 * cfg.dim[0], .out = dec, .out_ld = ld_dec});
    } else {
      // pads (1 - py, 1 - px), output pixel (2 oy + py, 2 ox + px): gemm() runs the four parities (merged when it can)
      gemm("gemm_convT4", up4[0], {.in = cat[0], .in_h = sh[0], .in_w = sw[0], .in_ld = 2 * cfg.dim[0], .out = dec, .out_ld = ld_dec, .pad_y = 1,
                                   .pad_x = 1, .out_mode = 2, .par = up4});
    }
    capture("up_block4", dec, Hd, Wd, C_out, ld_dec, Wd);
  }
  void tail(float* y, float* y_phys, float* x_next) { launch_tail(dec, 0, 0, Ho, y, y_phys, x_next); }
  // output rows [oy0, oy0 + rows) from the decoder buffer `dec_buf`, whose first row is decoder row `dec_row0`
  void launch_tail(const T* dec_buf, int dec_row0, int oy0, int rows, float* y, float* y_phys, float* x_next) {
    TailParams p;
    p.dec = dec_buf; p.ld = ld_dec; p.Hd = Hd; p.Wd = Wd;
    p.off_y = cfg.pad_activate ? cfg.pad_lat[0] : 0; p.off_x = cfg.pad_activate ? cfg.pad_lon[0] : 0;
    p.Hu = Hu; p.Wu = Wu; p.H = Ho; p.W = Wo; p.C = C_out; p.interp = cfg.interp;
    p.y = y; p.y_phys = y_phys; p.x_next = x_next; p.n_prog = n_prog < 0 ? 0 : n_prog; p.xmap = d_xmap;
    p.mean = have_denorm ? d_mean : nullptr; p.stdv = have_denorm ? d_std : nullptr;
    p.thr_lo = have_tracer ? d_lo : nullptr; p.thr_hi = have_tracer ? d_hi : nullptr;
    p.tracer_denorm = tracer_denorm;
    p.oy0 = oy0; p.dec_row0 = dec_row0; p.Hloc = rows;
    const size_t lds = (size_t)C_out * 65 * sizeof(float);
    static uint64_t attr_done_mask = 0;   // hipFuncSetAttribute is per device: one bit per device id
    if (!attr_done_on_device(attr_done_mask)) {
      WX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(tail_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      attr_mark_device(attr_done_mask);
    }
    if (!tail_channels_ok(C_out)) throw StateError("tail: a channel count ModelSpec::derive() should have refused");
    const double plane = (double)rows * Wo * C_out;
    timed("tail", 0.0, plane * (2.0 * sizeof(T) + 4.0 * ((y ? 1 : 0) + (y_phys ? 1 : 0)) + (x_next ? 4.0 : 0.0)), [&] {
      hipLaunchKernelGGL(tail_kernel<T>, dim3(cdiv(Wo, 64), rows), dim3(256), lds, cur_stream, p);
      WX_HIP(hipGetLastError());
    });
  }
  // ------------------------------------------------------------------ lat-band mode (wx_band.h)
  // One forecast sharded over n ranks by latitude.  A step is a PROGRAM of ops separated by exchanges; the driver
  // (wxengine/latband.py: torch.distributed P2P over RCCL, gloo, or in-process copies between virtual ranks) calls
  // band_begin / band_resume and moves the bytes of the staging buffers in between -- the engine packs the row runs of
  // the plan into `b_send` before handing control back and unpacks `b_recv` when it is resumed.
  bool band_on = false;
  int b_rank = 0, b_n = 1;
  BandPlan bplan;
  T *bcat[3] = {nullptr, nullptr, nullptr}, *bx3 = nullptr, *blong[4] = {nullptr, nullptr, nullptr, nullptr};
  T *bps[3] = {nullptr, nullptr, nullptr}, *bps4 = nullptr;   // wxformer: pixel-shuffled maps (2 / 1 halo rows, rows beyond the map stay zero)
  T *bxin = nullptr, *bxin_planar = nullptr, *bemb_in = nullptr, *bdec_in = nullptr, *bscut = nullptr, *bta = nullptr, *btb = nullptr,
    *bdec = nullptr;
  float* bxneed = nullptr;
  double *gn_all = nullptr, *fix_all = nullptr;
  float* by_internal = nullptr;   // y band when a post block runs and the caller did not ask for y
  char *b_send = nullptr, *b_recv = nullptr;
  int64_t b_send_need = 0, b_recv_need = 0;
  std::vector<std::function<void()>> b_ops;
  std::vector<int> b_xid;              // exchange that follows op i, or -1
  std::vector<std::function<void()>> b_pre;   // op i's part that does not depend on the exchange before it (interior rows): launched
                                              // right after that exchange's pack, i.e. while its bytes are on the wire
  // overlap: the transport of an exchange runs on a second stream between two events (pack done -> bytes moved), so the compute
  // stream keeps going with b_pre[i]; credit/domain_parallel/halo_exchange.py:45-79 waits for its batch_isend_irecv in place
  hipStream_t b_cstream = nullptr;
  hipEvent_t b_ev_pack = nullptr, b_ev_done = nullptr;
  bool b_async = false, b_cstream_own = false;
  // interior / boundary split of the convolutions behind a halo exchange: OFF unless an overlapped transport asks for it (measured on
  // MI355X, profiles/r03_latband_overlap_virtual_ranks_C3_bf16.txt: the two one-row launches cost each rank more than the ~20 us exchange they would hide)
  bool b_split = opt.band_split;   // set by band_comm_stream
  void* band_comm_stream(void* adopt) override {
    band_need();
    WX_HIP(hipSetDevice(device));
    // never while an exchange is in flight: band_resume records its "done" event on b_cstream, and the unpack waits on that event --
    // swapping the stream (or destroying the one the engine owns) mid-exchange would leave the bytes in flight unordered
    if (b_pending >= 0) throw StateError("wx_band_comm_stream: a step is in flight");
    if (adopt) {
      if (b_cstream && b_cstream != (hipStream_t)adopt) WX_HIP(hipStreamSynchronize(b_cstream));
      if (b_cstream_own && b_cstream) (void)hipStreamDestroy(b_cstream);
      b_cstream = (hipStream_t)adopt; b_cstream_own = false;
    } else if (!b_cstream) {
      WX_HIP(hipStreamCreateWithFlags(&b_cstream, hipStreamNonBlocking));
      b_cstream_own = true;
    }
    if (!b_ev_pack) {
      WX_HIP(hipEventCreateWithFlags(&b_ev_pack, hipEventDisableTiming));
      WX_HIP(hipEventCreateWithFlags(&b_ev_done, hipEventDisableTiming));
    }
    b_async = true;
    if (!b_split) {   // an overlapped transport: give it something to overlap with
      b_split = true;
      band_build_program();
    }
    return (void*)b_cstream;
  }
  size_t b_pc = 0;
  int b_pending = -1;
  int b_unpack_slots = 0;   // > 0: the last band_unpack left that many LayerNorm partials per token of the layout it filled
  const float *bx_own = nullptr, *bfrc_own = nullptr;
  float *by = nullptr, *by_phys = nullptr, *bx_next = nullptr;

  int b_rows(int s) const { return bplan.g.rows_short(s, b_rank); }
  int b_own_rows() const { return bplan.g.po[b_rank + 1] - bplan.g.po[b_rank]; }


  void band_enable(int rank, int n) override {
    if (cfg.pad_activate == 2) throw ConfigError("lat-band mode supports padding mode 'earth' only (the band plan's pole rows)");
    if (!finalized) throw StateError("wx_band_enable: finalize the weights first");
    if (band_on) throw StateError("wx_band_enable: already enabled");
    if (n < 1 || rank < 0 || rank >= n) throw ConfigError("wx_band_enable: bad rank / nranks");
    band_check_supported(*this);
    WX_HIP(hipSetDevice(device));
    if (splitk_bound(true) > splitk_bytes) {   // the band ranks' split-K rule reaches more tiles than the whole-map engine's
      splitk_bytes = splitk_bound(true);
      mem.release(splitk_buf);
      splitk_buf = (float*)mem.alloc(splitk_bytes);
    }
    bplan.build(band_model(*this, n, (int)sizeof(T), post ? post->n_fixers() : 0));
    b_rank = rank; b_n = n;
    const BandGeom& g = bplan.g;
    if (g.rows_short(0, rank) <= 0) throw ConfigError("lat-band mode: more ranks than window rows at stage 0");
    if (post && (post->row0 != g.po[rank] || post->h != g.po[rank + 1] - g.po[rank]))
      throw ConfigError("lat-band mode: the attached post block must cover this rank's rows (wx_post_set_band with the rows of "
                        "wx_band_plan_partition(p, 8, ...))");
    if (post && post->h == post->h_full && n > 1) throw ConfigError("lat-band mode: the attached post block covers the whole grid");
    // ---- buffers of this band
    const int st0 = cfg.embed_strides[0];
    const int64_t xin_elems = (int64_t)(st0 * g.rows_short(0, rank) + 2 * halo + 2) * (Wp + 2 * halo + 2) * cpad0;
    bxin = (T*)mem.alloc(xin_elems * sizeof(T));
    WX_HIP(hipMemset(bxin, 0, xin_elems * sizeof(T)));
    if (opt.use_patch && opt.planar_xin) {
      bxin_planar = (T*)mem.alloc(xin_elems * sizeof(T));
      WX_HIP(hipMemset(bxin_planar, 0, xin_elems * sizeof(T)));
    }
    const int xneed = bplan.x_need_hi[rank] - bplan.x_need_lo[rank];
    bxneed = (float*)mem.alloc((size_t)std::max(1, xneed) * C_in * cfg.image_width * sizeof(float));
    int64_t emb_max = 1, dec_in_max = 1, dt_max = 1;
    for (int s = 0; s < 4; ++s) {
      const int64_t rs = g.rows_short(s, rank), rl = g.rows_long(s, rank);
      if (s < 3) {
        const int64_t el = (rs + 2) * sw[s] * 2 * cfg.dim[s];
        bcat[s] = (T*)mem.alloc(el * sizeof(T));
        WX_HIP(hipMemset(bcat[s], 0, el * sizeof(T)));
      } else {
        bx3 = (T*)mem.alloc(std::max<int64_t>(1, rs * sw[s] * cfg.dim[s]) * sizeof(T));
      }
      if (cfg.global_window_size[s] > 1) blong[s] = (T*)mem.alloc(std::max<int64_t>(1, rl * sw[s] * cfg.dim[s]) * sizeof(T));
      if (s > 0) emb_max = std::max(emb_max, (int64_t)(cfg.embed_strides[s] * rs + bplan.m.emb_lo[s] + bplan.m.emb_hi[s]) * sw[s - 1] * cfg.dim[s - 1]);
      // scratch / attn_o / rowstat / statpart of the whole-map engine are large enough for any band
    }
    for (int i = 0; i < 3; ++i) {
      const int si = 3 - i, so = 2 - i;
      const int64_t rows_in = (g.rows_short(so, rank) + 1) / 2 + 1 + (cfg.arch == WX_ARCH_WXFORMER ? 4 : 0);
      if (cfg.arch == WX_ARCH_WXFORMER) {
        const int64_t el = (int64_t)(g.rows_short(so, rank) + 4) * sw[so] * ups[i].cout;
        bps[i] = (T*)mem.alloc(el * sizeof(T));
        WX_HIP(hipMemset(bps[i], 0, el * sizeof(T)));
      }
      dec_in_max = std::max(dec_in_max, rows_in * sw[si] * (i == 0 ? cfg.dim[3] : 2 * cfg.dim[si]));
      dt_max = std::max(dt_max, (int64_t)(g.rows_short(so, rank) + 2) * sw[so] * ups[i].cout);
    }
    bemb_in = (T*)mem.alloc(emb_max * sizeof(T));
    bdec_in = (T*)mem.alloc(dec_in_max * sizeof(T));
    bscut = (T*)mem.alloc(dt_max * sizeof(T));
    bta = (T*)mem.alloc(dt_max * sizeof(T));
    btb = (T*)mem.alloc(dt_max * sizeof(T));
    WX_HIP(hipMemset(bscut, 0, dt_max * sizeof(T)));
    WX_HIP(hipMemset(btb, 0, dt_max * sizeof(T)));
    if (cfg.arch == WX_ARCH_WXFORMER) {
      const int64_t el = (int64_t)(2 * g.rows_short(0, rank) + 2) * Wd * cpad4;
      bps4 = (T*)mem.alloc(el * sizeof(T));
      WX_HIP(hipMemset(bps4, 0, el * sizeof(T)));
    }
    const int64_t dec_el = (int64_t)(2 * g.rows_short(0, rank) + 2) * Wd * ld_dec;
    bdec = (T*)mem.alloc(dec_el * sizeof(T));
    WX_HIP(hipMemset(bdec, 0, dec_el * sizeof(T)));
    gn_all = (double*)mem.alloc((size_t)n * 2 * cfg.dim[3] * sizeof(double));
    fix_all = (double*)mem.alloc((size_t)n * 4 * sizeof(double));
    if (post) by_internal = (float*)mem.alloc(std::max<size_t>(1, (size_t)C_out * (g.po[rank + 1] - g.po[rank]) * Wo) * sizeof(float));
    for (const BandExchange& x : bplan.xs) {
      b_send_need = std::max(b_send_need, band_send_bytes(x, rank));
      b_recv_need = std::max(b_recv_need, band_recv_bytes(x, rank));
    }
    band_on = true;
    band_upload_maps();
    band_build_program();
  }
  void band_info(int* own_row0, int* own_rows, int64_t* send_bytes, int64_t* recv_bytes, int* n_exchanges) override {
    band_need();
    *own_row0 = bplan.g.po[b_rank]; *own_rows = b_own_rows();
    *send_bytes = b_send_need; *recv_bytes = b_recv_need; *n_exchanges = (int)bplan.xs.size();
  }
  void band_set_staging(void* send, int64_t send_bytes, void* recv, int64_t recv_bytes) override {
    band_need();
    if (send_bytes < b_send_need || recv_bytes < b_recv_need) throw ConfigError("wx_band_set_staging: buffers smaller than wx_band_info asks for");
    if ((b_send_need && !send) || (b_recv_need && !recv)) throw ConfigError("wx_band_set_staging: null staging buffer");
    b_send = (char*)send; b_recv = (char*)recv;
  }
  int band_messages_of(int xid, wx_band_msg* sends, int cap_s, int* n_s, wx_band_msg* recvs, int cap_r, int* n_r) override {
    band_need();
    if (xid < 0 || xid >= (int)bplan.xs.size()) throw ConfigError("wx_band_exchange: no such exchange");
    std::vector<BandMsg> s, r;
    band_messages(bplan.xs[xid], b_rank, &s, &r);
    if ((int)s.size() > cap_s || (int)r.size() > cap_r) throw ConfigError("wx_band_exchange: message arrays too small (need nranks - 1)");
    for (size_t i = 0; i < s.size(); ++i) sends[i] = wx_band_msg{s[i].peer, s[i].offset, s[i].bytes};
    for (size_t i = 0; i < r.size(); ++i) recvs[i] = wx_band_msg{r[i].peer, r[i].offset, r[i].bytes};
    *n_s = (int)s.size(); *n_r = (int)r.size();
    return 0;
  }
  void band_need() const { if (!band_on) throw StateError("lat-band mode is not enabled (wx_band_enable)"); }

  // ---- buffer views: the shape of ONE row of buffer `buf` (every row of an exchange has the same shape)
  struct BRow { char* base; int64_t row_stride, pitch, width; int hpr; };
  BRow band_row(int buf, const BandExchange& x) {
    const int64_t e = sizeof(T);
    const int s = x.stage;
    auto tok = [&](T* base, int64_t ld_el, int64_t ch_el, int64_t ch_off, int w) {
      return BRow{reinterpret_cast<char*>(base + ch_off), (int64_t)w * ld_el * e, ld_el * e, ch_el * e, w};
    };
    auto chan = [&](const float* base, int rows_loc) {   // [C_in][rows][W] fp32: a "row" is one W-line of every channel
      const int64_t w4 = (int64_t)cfg.image_width * 4;
      return BRow{reinterpret_cast<char*>(const_cast<float*>(base)), w4, rows_loc * w4, w4, C_in};
    };
    switch (buf) {
      case BB_X_OWN: return chan(bx_own, b_own_rows());
      case BB_X_NEED: return chan(bxneed, bplan.x_need_hi[b_rank] - bplan.x_need_lo[b_rank]);
      case BB_STREAM_S: return s < 3 ? tok(bcat[s], 2 * cfg.dim[s], cfg.dim[s], cfg.dim[s], sw[s]) : tok(bx3, cfg.dim[3], cfg.dim[3], 0, sw[3]);
      case BB_STREAM_L: return tok(blong[s], cfg.dim[s], cfg.dim[s], 0, sw[s]);
      case BB_EMB_IN: return tok(bemb_in, cfg.dim[s], cfg.dim[s], 0, sw[s]);
      case BB_DEC_SRC: return s == 3 ? tok(bx3, cfg.dim[3], cfg.dim[3], 0, sw[3]) : tok(bcat[s], 2 * cfg.dim[s], 2 * cfg.dim[s], 0, sw[s]);
      case BB_DEC_IN: { const int64_t c = s == 3 ? cfg.dim[3] : 2 * cfg.dim[s]; return tok(bdec_in, c, c, 0, sw[s]); }
      case BB_SCUT: return tok(bscut, ups[2 - s].cout, ups[2 - s].cout, 0, sw[s]);
      case BB_TB: return tok(btb, ups[2 - s].cout, ups[2 - s].cout, 0, sw[s]);
      case BB_CAT0: return tok(bcat[0], 2 * cfg.dim[0], 2 * cfg.dim[0], 0, sw[0]);
      case BB_DEC: return tok(bdec, ld_dec, ld_dec, 0, Wd);
      case BB_GN_ACC: return BRow{reinterpret_cast<char*>(gn_acc), x.row_bytes, x.row_bytes, x.row_bytes, 1};
      case BB_GN_ALL: return BRow{reinterpret_cast<char*>(gn_all), x.row_bytes, x.row_bytes, x.row_bytes, 1};
      case BB_PS4: return tok(bps4, cpad4, cpad4, 0, Wd);
      case BB_FIX_ACC: return BRow{reinterpret_cast<char*>(post->sums), 32, 32, 32, 1};
      case BB_FIX_ALL: return BRow{reinterpret_cast<char*>(fix_all), 32, 32, 32, 1};
    }
    throw StateError("band: unknown buffer id");
  }
  BRow band_staging(char* base, const BRow& like) { return BRow{base, like.width * like.hpr, like.width, like.width, like.hpr}; }
  // row lists of every exchange, resident on the device (built once in band_enable)
  struct BandXDev {
    int2 *pack = nullptr, *merged = nullptr;   // merged: the receiving side's one row list (band_unpack_kernel: staging / own / zero rows)
    int n_pack = 0, n_unpack = 0, n_self = 0, n_zero = 0, n_merged = 0;
  };
  std::vector<BandXDev> bx_dev;
  void band_upload_maps() {
    bx_dev.assign(bplan.xs.size(), BandXDev());
    for (size_t xid = 0; xid < bplan.xs.size(); ++xid) {
      const BandExchange& x = bplan.xs[xid];
      std::vector<int2> pk, up, sf;
      std::vector<int> zr;
      int row = 0;
      for (int p = 0; p < b_n; ++p) {
        if (p == b_rank) continue;
        for (const BandSeg& sg : x.recv[p])
          if (sg.peer == b_rank)
            for (int k = 0; k < sg.nrows; ++k) pk.push_back(make_int2(sg.src_row + k, row++));
      }
      row = 0;
      for (int r = 0; r < b_n; ++r) {
        if (r == b_rank) continue;
        for (const BandSeg& sg : x.recv[b_rank])
          if (sg.peer == r)
            for (int k = 0; k < sg.nrows; ++k) up.push_back(make_int2(row++, sg.dst_row + k));
      }
      for (const BandSeg& sg : x.recv[b_rank])
        for (int k = 0; k < sg.nrows; ++k) {
          if (sg.peer == b_rank) sf.push_back(make_int2(sg.src_row + k, sg.dst_row + k));
          else if (sg.peer < 0) zr.push_back(sg.dst_row + k);
        }
      BandXDev& d = bx_dev[xid];
      auto up2 = [&](const std::vector<int2>& v, int2** dst, int* n) {
        *n = (int)v.size();
        if (v.empty()) return;
        *dst = (int2*)mem.alloc(v.size() * sizeof(int2));
        WX_HIP(hipMemcpy(*dst, v.data(), v.size() * sizeof(int2), hipMemcpyHostToDevice));
      };
      up2(pk, &d.pack, &d.n_pack);
      d.n_unpack = (int)up.size(); d.n_self = (int)sf.size(); d.n_zero = (int)zr.size();
      std::vector<int2> mg;
      for (const int2& e : up) mg.push_back(e);
      for (const int2& e : sf) mg.push_back(make_int2(-1 - e.x, e.y));
      for (int zrow : zr) mg.push_back(make_int2((int)0x80000000, zrow));
      up2(mg, &d.merged, &d.n_merged);
    }
  }
  void band_rowcopy(const BRow& d, const BRow& s, const int2* map, int n) {
    if (n <= 0) return;
    if (d.width != s.width || d.hpr != s.hpr || (d.width & 15)) throw StateError("band: row shape mismatch");
    const int64_t per_row = (int64_t)d.hpr * (d.width / 16);
    const dim3 grid((unsigned)std::min<int64_t>(64, cdiv(per_row, 256)), (unsigned)std::min(n, 16384));
    hipLaunchKernelGGL(band_rowcopy_kernel, grid, dim3(256), 0, cur_stream, d.base,
                       d.row_stride, d.pitch, s.base, s.row_stride, s.pitch, (int)(d.width / 16), d.hpr, n, map);
    WX_HIP(hipGetLastError());
  }
  void band_pack(int xid) {
    const BandExchange& x = bplan.xs[xid];
    const BandXDev& d = bx_dev[xid];
    if (d.n_pack <= 0) return;
    const BRow s = band_row(x.src_buf, x);
    if (s.width * s.hpr != x.row_bytes) throw StateError("band: row size mismatch in " + x.name);
    band_rowcopy(band_staging(b_send, s), s, d.pack, d.n_pack);
  }
  void band_unpack(int xid) {
    const BandExchange& x = bplan.xs[xid];
    const BandXDev& d = bx_dev[xid];
    const BRow dv = band_row(x.dst_buf, x);
    if (dv.width * dv.hpr != x.row_bytes) throw StateError("band: row size mismatch in " + x.name);
    // the rows of a long-attention redistribution arrive with their LayerNorm partials: every row of the new layout passes through one of
    // the two copies below (wx_band.h: to_long / to_short gather whole layouts, no zero fill), so the sub-block behind the exchange
    // starts from statpart instead of an ln_stats launch
    int slots = 0, row_off = 0, rows = 0;
    if (opt.band_stats_ship && opt.fuse_ln && (x.name.compare(0, 8, "to_long.") == 0 || x.name.compare(0, 9, "to_short.") == 0) && d.n_zero == 0) {
      const int64_t w16 = dv.width / 16;
      const bool to_long = x.dst_buf == BB_STREAM_L;
      rows = to_long ? bplan.g.rows_long(x.stage, b_rank) : bplan.g.rows_short(x.stage, b_rank);
      row_off = (!to_long && x.stage < 3) ? -1 : 0;   // the short layout sits behind one halo row of the concat buffer
      if (w16 >= 1 && (w16 & (w16 - 1)) == 0 && w16 <= 512 && d.n_unpack + d.n_self == rows) slots = (int)std::max<int64_t>(1, w16 / 64);
    }
    b_unpack_slots = slots;
    if (d.n_merged <= 0) return;
    // one launch for the received rows, the rows that stay on this rank and the zero rows beyond the pole (band_unpack_kernel)
    const BRow g = band_staging(b_recv, dv);
    const BRow o = d.n_self > 0 ? band_row(x.src_buf, x) : g;
    if (o.width != dv.width || o.hpr != dv.hpr || (dv.width & 15)) throw StateError("band: row shape mismatch");
    const int64_t per_row = (int64_t)dv.hpr * (dv.width / 16);
    const dim3 grid((unsigned)std::min<int64_t>(64, cdiv(per_row, 256)), (unsigned)std::min(d.n_merged, 16384));
    hipLaunchKernelGGL(band_unpack_kernel<T>, grid, dim3(256), 0, cur_stream, dv.base, dv.row_stride, dv.pitch, g.base, g.row_stride, g.pitch, o.base,
                       o.row_stride, o.pitch, (int)(dv.width / 16), dv.hpr, d.n_merged, d.merged,
                       slots > 0 ? stat_dst((int64_t)rows * dv.hpr, slots) : nullptr, slots, row_off, rows);
    WX_HIP(hipGetLastError());
  }

  // ---- the program
  int b_next_x = 0;
  void band_op(std::function<void()> f, const char* exchange = nullptr, const std::string& suffix = "") {
    int xid = -1;
    if (exchange) {
      const std::string name = exchange + suffix;
      if (b_next_x >= (int)bplan.xs.size() || bplan.xs[b_next_x].name != name)
        throw StateError("band: program / plan out of step at " + name);
      xid = b_next_x++;
    }
    b_ops.push_back(std::move(f));
    b_xid.push_back(xid);
    b_pre.emplace_back();
  }
  void band_pre(std::function<void()> f) { b_pre.back() = std::move(f); }   // the exchange-independent part of the op pushed last
  void band_attach(const std::string& name) {   // the exchange follows the op pushed last
    if (b_xid.empty() || b_xid.back() >= 0) throw StateError("band: two exchanges after one op at " + name);
    b_xid.back() = band_take(name);
  }
  // the stream's rows were just replaced by an exchange: the LayerNorm partials belonged to the rows that left -- unless the unpack of the
  // redistribution that brought the new rows took them along
  void band_adopt_unpacked_stats() {
    stat_tiles_ready = b_unpack_slots;
    b_unpack_slots = 0;
  }
  // GroupNorm: local (sum, sum sq) -> gn_acc
  void band_gn_local(const T* x, int c, int64_t m, int tiles) {
    if (m <= 0) { WX_HIP(hipMemsetAsync(gn_acc, 0, 2 * c * sizeof(double), cur_stream)); return; }
    gn_local_stats(x, c, m, tiles);
  }
  void band_gn_finish(const T* x, int c, int64_t m_local, int64_t m_global, int64_t g_off, int64_t b_off, const T* res, int64_t res_ld,
                      T* out, int64_t out_ld) {
    hipLaunchKernelGGL(band_gn_sum_kernel, dim3(cdiv(2 * c, 128)), dim3(128), 0, cur_stream, gn_all, b_n, 2 * c, gn_acc);
    WX_HIP(hipGetLastError());
    if (m_local <= 0) return;
    gn_finalize_apply(x, c, m_local, m_global, g_off, b_off, res, res_ld, out, out_ld);
  }
  // A 3x3 conv (+ GroupNorm partials) over a band whose input buffer carries one halo row above and below (rows + 2 buffer rows).
  // Output rows 1 .. rows - 2 need no halo: they are launched as the op's `pre` part, right after the halo exchange was packed
  // (boundary = false); the two outer rows follow once the halo rows have arrived (boundary = true).  The GroupNorm tile
  // partials of the three launches are appended to one list and folded together.  Returns the boundary call's tile count for
  // band_gn_local (0: no partials -- it falls back to the two-pass statistics kernel).
  int b_gn_tiles = 0;   // tiles the interior launch of the current conv wrote (boundary = false)
  int band_conv3_rows(const ConvW& w, const T* in, T* out, int rows, int wd, int c, bool boundary) {
    const int64_t row = (int64_t)wd * c;
    const bool split = b_split && rows >= 4;
    auto conv = [&](const T* src, int out_rows, T* dst, bool gn, int gn_off) {   // output rows of dst from rows out_rows + 2 of src
      return gemm("gemm_conv3", w, {.in = src, .in_h = out_rows + 2, .in_w = wd, .in_ld = c, .out = dst, .out_ld = c, .pad_y = 0, .out_h = out_rows,
                                    .want_gn = gn, .gn_off = gn_off}).gn_tiles;
    };
    if (!boundary) {
      b_gn_tiles = rows > 0 && split ? conv(in + row, rows - 2, out + row, true, 0) : 0;
      return b_gn_tiles;
    }
    if (rows <= 0) return 0;
    if (!split) return conv(in, rows, out, true, 0);
    const int pre = b_gn_tiles;
    const int top = conv(in, 1, out, pre > 0, pre);
    const int bottom = conv(in + (rows - 1) * row, 1, out + (rows - 1) * row, pre > 0, pre + top);
    return pre > 0 && top > 0 && bottom > 0 ? pre + top + bottom : 0;
  }
  void band_build_program() {
    const BandGeom& g = bplan.g;
    const int r = b_rank;
    b_ops.clear(); b_xid.clear(); b_pre.clear(); b_next_x = 0;
    band_op([] {}, "x_rows");
    // stage 0: pack the band's padded patch, CrossEmbed
    band_op([this, r] {
      const BandGeom& g = bplan.g;
      const int st0 = cfg.embed_strides[0], a0 = g.ps[0][r], rows0 = g.rows_short(0, r);
      cur_stage = 0;
      stat_tiles_ready = 0;
      const int Hb = st0 * rows0 + 2 * halo;
      pack_input(bxneed, bxin, bxin_planar, Hb, bplan.pad_lo[r], bplan.pad_hi[r] - bplan.pad_lo[r], bplan.pad_lo[r] - (st0 * a0 - halo),
                 bplan.x_need_lo[r], bplan.x_need_hi[r] - bplan.x_need_lo[r]);
      cross_embed(band_view(0, false), bxin, bxin_planar, Hb, 0, 0);
    });
    for (int s = 0; s < 4; ++s) {
      if (s > 0) {
        band_attach("embed_in.s" + std::to_string(s));
        band_op([this, s, r] {
          const BandGeom& g = bplan.g;
          cur_stage = s;
          band_adopt_unpacked_stats();
          const int rows = g.rows_short(s, r);
          cross_embed(band_view(s, false), bemb_in, nullptr, cfg.embed_strides[s] * rows + bplan.m.emb_lo[s] + bplan.m.emb_hi[s], -bplan.m.emb_lo[s], cfg.dim[s - 1]);
        });
      }
      const bool a2a = cfg.global_window_size[s] > 1;
      for (int d = 0; d < cfg.depth[s]; ++d) {
        const std::string tag = ".s" + std::to_string(s) + "." + std::to_string(d);
        if (a2a) {
          band_op([this, s, d] { cur_stage = s; block_half(band_view(s, false), d, false); }, "to_long", tag);
          band_op([this, s, d] { band_adopt_unpacked_stats(); block_half(band_view(s, true), d, true); }, "to_short", tag);
          band_op([this] { band_adopt_unpacked_stats(); });
        } else {
          band_op([this, s, d] { cur_stage = s; block_half(band_view(s, false), d, false); block_half(band_view(s, false), d, true); });
        }
      }
    }
    // decoder
    for (int i = 0; i < 3; ++i) {
      const int si = 3 - i, so = 2 - i;
      const std::string lv = ".l" + std::to_string(i);
      band_attach("dec_in" + lv);
      band_op([this, i, si, so, r] {
        const BandGeom& g = bplan.g;
        cur_stage = 4 + i;
        stat_tiles_ready = 0;
        const UpL& u = ups[i];
        const int a = g.ps[so][r], b = g.ps[so][r + 1];
        const int64_t in_ld = i == 0 ? cfg.dim[3] : 2 * cfg.dim[si];
        if (b > a && cfg.arch == WX_ARCH_WXFORMER) {
          // x = PixelShuffle(conv3x3(x)); x = x + sharp(x)  (wxformer/crossformer.py:157-158) on rows a-1 .. b of the
          // shuffled map, recomputed here instead of exchanged; bdec_in holds input rows j0-1 .. j1 (zero beyond the map)
          int j0, j1;
          bplan.dec_ps_rows(so, a, b, &j0, &j1);
          const int64_t row = (int64_t)sw[so] * u.cout;
          T* ps = bps[i];                                    // buffer row 0 = map row a - 2
          gemm("gemm_convPS", u.convps, {.in = bdec_in, .in_h = j1 - j0 + 2, .in_w = sw[si], .in_ld = in_ld, .out = ps + (2 * j0 - (a - 2)) * row,
                                         .out_ld = u.cout, .pad_y = 0, .out_h = j1 - j0, .out_mode = 1, .cout = u.cout});
          gemm("gemm_conv3", u.sharp, {.in = ps + row, .in_h = b - a + 2, .in_w = sw[so], .in_ld = u.cout, .out = bscut + row, .out_ld = u.cout, .pad_y = 0,
                                       .out_h = b - a, .res = ps + 2 * row, .res_ld = u.cout});
        } else if (b > a) {
          const int j0 = a / 2, j1 = (b + 1) / 2;
          T* out = bscut + (int64_t)(2 * j0 - (a - 1)) * sw[so] * u.cout;   // output rows 2 j0 .. 2 j1 - 1; owned row `a` is buffer row 1
          gemm("gemm_convT2", u.convt, {.in = bdec_in, .in_h = j1 - j0, .in_w = sw[si], .in_ld = in_ld, .out = out, .out_ld = u.cout, .out_mode = 1,
                                        .cout = u.cout});
        }
      }, "halo_scut", lv);
      band_op([this, i, so, r] {
        const UpL& u = ups[i];
        const int rows = bplan.g.rows_short(so, r);
        band_gn_local(bta, u.cout, (int64_t)rows * sw[so], band_conv3_rows(u.c1, bscut, bta, rows, sw[so], u.cout, /*boundary=*/true));
      }, "gn", lv + ".0");
      band_pre([this, i, so, r] { band_conv3_rows(ups[i].c1, bscut, bta, bplan.g.rows_short(so, r), sw[so], ups[i].cout, /*boundary=*/false); });
      band_op([this, i, so, r] {
        const BandGeom& g = bplan.g;
        const UpL& u = ups[i];
        const int rows = g.rows_short(so, r);
        band_gn_finish(bta, u.cout, (int64_t)rows * sw[so], (int64_t)sh[so] * sw[so], u.g1, u.b1, nullptr, 0,
                       btb + (int64_t)sw[so] * u.cout, u.cout);
      }, "halo_tb", lv);
      band_op([this, i, so, r] {
        const UpL& u = ups[i];
        const int rows = bplan.g.rows_short(so, r);
        band_gn_local(bta, u.cout, (int64_t)rows * sw[so], band_conv3_rows(u.c2, btb, bta, rows, sw[so], u.cout, /*boundary=*/true));
      }, "gn", lv + ".1");
      band_pre([this, i, so, r] { band_conv3_rows(ups[i].c2, btb, bta, bplan.g.rows_short(so, r), sw[so], ups[i].cout, /*boundary=*/false); });
      band_op([this, i, so, r] {
        const BandGeom& g = bplan.g;
        const UpL& u = ups[i];
        const int rows = g.rows_short(so, r);
        const int64_t row_el = (int64_t)sw[so] * 2 * cfg.dim[so];
        band_gn_finish(bta, u.cout, (int64_t)rows * sw[so], (int64_t)sh[so] * sw[so], u.g2, u.b2, bscut + (int64_t)sw[so] * u.cout, u.cout,
                       bcat[so] + row_el, 2 * cfg.dim[so]);
      });
    }
    band_attach("halo_cat0");
    if (cfg.arch == WX_ARCH_WXFORMER) {
      band_op([this, r] {
        cur_stage = 7;
        const int rows = bplan.g.rows_short(0, r);
        gemm("gemm_convPS", ps4, {.in = bcat[0], .in_h = rows + 2, .in_w = sw[0], .in_ld = 2 * cfg.dim[0], .out = bps4 + (int64_t)Wd * cpad4,
                                  .out_ld = cpad4, .pad_y = 0, .out_h = rows, .out_mode = 1, .cout = cpad4});
      }, "halo_ps4");
    }
    band_op([this, r] {
      const BandGeom& g = bplan.g;
      cur_stage = 7;
      const int rows = g.rows_short(0, r);
      if (cfg.arch == WX_ARCH_WXFORMER) {
        gemm("gemm_conv3", fin4, {.in = bps4, .in_h = 2 * rows + 2, .in_w = Wd, .in_ld = cpad4, .out = bdec + (int64_t)Wd * ld_dec, .out_ld = ld_dec,
                                  .pad_y = 0, .out_h = 2 * rows});
        return;
      }
      gemm("gemm_convT4", up4[0], {.in = bcat[0], .in_h = rows + 2, .in_w = sw[0], .in_ld = 2 * cfg.dim[0], .out = bdec + (int64_t)Wd * ld_dec,
                                   .out_ld = ld_dec, .pad_y = 0, .pad_x = 1, .out_h = rows, .out_mode = 2, .par = up4});
    }, "halo_dec");
    band_op([this, r] { band_tail(2 * bplan.g.ps[0][r] - 1, post != nullptr); });
    if (post) {   // a12 under sharding: local integrals, every rank's sums to everyone, added in rank order, local correction
      int k = 0;
      for (size_t o = 0; o < post->ops.size(); ++o) {
        if (post->ops[o].kind == 0) {
          band_op([this, o] { post->tracer_op(post->ops[o], by ? by : by_internal, cur_stream); });
          continue;
        }
        band_op([this, o] { post->reduce_op(post->ops[o], bx_own, by ? by : by_internal, cur_stream); }, "fix", "." + std::to_string(k++));
        band_op([this, o] {
          hipLaunchKernelGGL(band_gn_sum_kernel, dim3(1), dim3(64), 0, cur_stream, fix_all, b_n, 4, post->sums);
          WX_HIP(hipGetLastError());
          post->finish_op(post->ops[o], bx_own, by ? by : by_internal, cur_stream);
        });
      }
      band_op([this] { band_finish_post(); });
    }
    if (b_next_x != (int)bplan.xs.size()) throw StateError("band: program does not consume every exchange of the plan");
    (void)g;
  }
  int band_take(const std::string& name) {
    if (b_next_x >= (int)bplan.xs.size() || bplan.xs[b_next_x].name != name) throw StateError("band: program / plan out of step at " + name);
    return b_next_x++;
  }
  void band_x_next_copies() {
    const int own = b_own_rows();
    if (!bx_next || own <= 0) return;
    const int64_t plane_b = (int64_t)own * cfg.image_width;
    copy_layout_groups(bx_own, bfrc_own, bx_next, plane_b, cur_stream);
  }
  void band_finish_post() {
    const int own = b_own_rows();
    if (own > 0 && (by_phys || bx_next)) launch_finish(by ? by : by_internal, (int64_t)own * Wo, by_phys, bx_next);
    band_x_next_copies();
  }
  void band_tail(int dec_row0, bool post_mode) {
    const int own = b_own_rows();
    if (own <= 0) return;
    float* y = post_mode ? (by ? by : by_internal) : by;
    launch_tail(bdec, dec_row0, bplan.g.po[b_rank], own, y, post_mode ? nullptr : by_phys, post_mode ? nullptr : bx_next);
    if (!post_mode) band_x_next_copies();
  }
  int band_run() {
    while (b_pc < b_ops.size()) {
      b_ops[b_pc]();
      const int xid = b_xid[b_pc];
      ++b_pc;
      if (xid >= 0) {
        timed("band_pack", 0.0, (double)band_send_bytes(bplan.xs[xid], b_rank) * 2.0, [&] { band_pack(xid); });
        if (b_async) {   // the transport (second stream) may start now ...
          WX_HIP(hipEventRecord(b_ev_pack, cur_stream));
          WX_HIP(hipStreamWaitEvent(b_cstream, b_ev_pack, 0));
        }
        if (b_pc < b_ops.size() && b_pre[b_pc]) b_pre[b_pc]();   // ... while the next op's interior rows are computed
        b_pending = xid;
        return xid;
      }
    }
    b_pending = -1;
    if (prof_on) drain();
    return -1;
  }
  int band_begin(const float* x_own, const float* frc_own, float* y, float* y_phys, float* x_next, hipStream_t s) override {
    band_need();
    check_ready();
    if (b_pending >= 0) throw StateError("wx_band_begin: the previous step is still waiting for an exchange");
    if ((b_send_need && !b_send) || (b_recv_need && !b_recv)) throw StateError("wx_band_begin: no staging buffers (wx_band_set_staging)");
    if (!x_own && b_own_rows() > 0) throw ConfigError("wx_band_begin: null input band");   // a polar rank may own pad rows only
    if (x_next) {
      if (n_prog < 0) throw StateError("wx_band_begin with x_next needs wx_set_layout first");
      if (x_next == x_own) throw ConfigError("x_next may not alias x");
      if (n_dyn > 0 && !frc_own) throw ConfigError("forcing pointer is NULL but the layout has dynamic forcing channels");
    }
    if (y_phys && !have_denorm) throw StateError("wx_band_begin with y_phys needs wx_set_denorm first");
    cur_stream = s;
    bx_own = x_own; bfrc_own = frc_own; by = y; by_phys = y_phys; bx_next = x_next;
    b_pc = 0;
    return band_run();
  }
  // ---- RCCL transport inside the engine: no host code between the segments of a step besides the launches themselves
  ncclComm_t b_comm = nullptr;
  std::vector<std::pair<std::vector<BandMsg>, std::vector<BandMsg>>> b_msgs;
  void band_rccl_init(const ncclUniqueId& id) override {
    band_need();
    if (b_comm) throw StateError("wx_band_rccl_init: communicator already created");
    WX_HIP(hipSetDevice(device));
    RcclApi& api = RcclApi::get();
    api.check(api.CommInitRank(&b_comm, b_n, id, b_rank), "ncclCommInitRank");
    if (!b_send && b_send_need) b_send = (char*)mem.alloc((size_t)b_send_need);
    if (!b_recv && b_recv_need) b_recv = (char*)mem.alloc((size_t)b_recv_need);
    b_msgs.resize(bplan.xs.size());
    for (size_t x = 0; x < bplan.xs.size(); ++x) band_messages(bplan.xs[x], b_rank, &b_msgs[x].first, &b_msgs[x].second);
    if (opt.band_overlap) band_comm_stream(nullptr);
  }
  void band_step_rccl(const float* x_own, const float* frc_own, float* y, float* y_phys, float* x_next, hipStream_t s) override {
    if (!b_comm) throw StateError("wx_band_step_rccl: no communicator (wx_band_rccl_init)");
    RcclApi& api = RcclApi::get();
    int xid = band_begin(x_own, frc_own, y, y_phys, x_next, s);
    while (xid >= 0) {
      const auto& m = b_msgs[xid];
      if (!m.first.empty() || !m.second.empty()) {   // every pair at once: the grouped send/recv idiom (all-to-all safe)
        api.check(api.GroupStart(), "ncclGroupStart");
        hipStream_t ts = b_async ? b_cstream : cur_stream;   // second stream: the exchange overlaps the next op's interior rows
        for (const BandMsg& q : m.first) api.check(api.Send(b_send + q.offset, (size_t)q.bytes, ncclInt8, q.peer, b_comm, ts), "ncclSend");
        for (const BandMsg& q : m.second) api.check(api.Recv(b_recv + q.offset, (size_t)q.bytes, ncclInt8, q.peer, b_comm, ts), "ncclRecv");
        api.check(api.GroupEnd(), "ncclGroupEnd");
      }
      xid = band_resume();
    }
  }
  int band_resume() override {
    band_need();
    if (b_pending < 0) throw StateError("wx_band_resume: no exchange is pending");
    WX_HIP(hipSetDevice(device));
    {
      const int xid = b_pending;
      if (b_async) {   // everything the transport put on the second stream has to land before the unpack
        WX_HIP(hipEventRecord(b_ev_done, b_cstream));
        WX_HIP(hipStreamWaitEvent(cur_stream, b_ev_done, 0));
      }
      timed("band_unpack", 0.0, (double)band_recv_bytes(bplan.xs[xid], b_rank) * 2.0, [&] { band_unpack(xid); });
    }
    return band_run();
  }
  void check_ready() {
    if (!finalized) throw StateError("weights not finalized (call wx_finalize_weights after loading every tensor)");
    WX_HIP(hipSetDevice(device));
  }
  void forward(const float* x, float* y, int batch, hipStream_t s) override {
    check_ready();
    if (band_on) throw StateError("this engine is in lat-band mode: drive it with wx_band_begin / wx_band_resume");
    if (batch < 1) throw ConfigError("batch must be >= 1");
    cur_stream = s;
    const int64_t in_item = (int64_t)C_in * cfg.image_height * cfg.image_width;
    const int64_t out_item = (int64_t)C_out * Ho * Wo;
    for (int b = 0; b < batch; ++b) {
      cur_row = b;
      core(x + b * in_item);
      finish_item(x + b * in_item, y + b * out_item, nullptr, nullptr);
    }
    cur_row = 0;
    noise_next_step();
    if (prof_on) drain();
  }
  void step(const float* x, const float* frc, float* y, float* y_phys, float* x_next, hipStream_t s) override {
    check_ready();
    if (band_on) throw StateError("this engine is in lat-band mode: drive it with wx_band_begin / wx_band_resume");
    if (cfg.frames != 1 || cfg.output_frames != 1) throw ConfigError("wx_step needs frames == output_frames == 1");
    if (x_next) {
      if (n_prog < 0) throw StateError("wx_step with x_next needs wx_set_layout first");
      if (x_next == x) throw ConfigError("x_next may not alias x");
      if (n_dyn > 0 && !frc) throw ConfigError("forcing pointer is NULL but the layout has dynamic forcing channels");
      if (Ho != cfg.image_height || Wo != cfg.image_width) throw ConfigError("wx_step needs output size == input size");
    }
    if (y_phys && !have_denorm) throw StateError("wx_step with y_phys needs wx_set_denorm first");
    cur_stream = s;
    core(x);
    finish_item(x, y, y_phys, x_next);
    noise_next_step();
    if (x_next) {
      const int64_t plane = (int64_t)cfg.image_height * cfg.image_width;
      copy_layout_groups(x, frc, x_next, plane, s);
    }
    if (prof_on) drain();
  }

  // ------------------------------------------------------------------ wx_rollout
  // The predict() loop of credit/applications/rollout_to_netcdf.py:262-316 inside the library: n steps of
  // (forward, fixers, de-normalise, update_x) with the state ping-ponging between two engine-owned buffers -- no host code
  // between steps.  Optionally (WX_GRAPH=1) every step is captured once as a hipGraph per (ping-pong parity, y_phys destination,
  // need-next) and replayed; both ways issue exactly the launches of wx_step.
  float* roll_x[2] = {nullptr, nullptr};
  float* roll_frc = nullptr;
  hipStream_t roll_stream = nullptr;
  hipEvent_t roll_ev_in = nullptr, roll_ev_out = nullptr;
  std::map<std::tuple<int, const void*, int>, hipGraphExec_t> roll_graphs;
  bool roll_warm = false;
  int roll_frc_ndyn = 0;   // forcing planes roll_frc was sized for
  // captured step graphs bake in the de-normalisation / tracer arguments, the layout-group copies and the post-block decision:
  // every setter that changes one of them drops the graphs (after the replays in flight on roll_stream have finished)
  void roll_invalidate() {
    if (roll_graphs.empty()) return;
    if (roll_stream) (void)hipStreamSynchronize(roll_stream);
    for (auto& kv : roll_graphs) (void)hipGraphExecDestroy(kv.second);
    roll_graphs.clear();
  }
  // WX_GRAPH=1 (Options::graph_mode) replays each step from a captured hipGraph; off by default, measured slower (wx_options.h)
  bool want_graph() const { return opt.graph_mode == 1 && !prof_on && !dbg_on && !band_on && !post; }
  void step_body(const float* x, const float* frc, float* y_phys, float* x_next, hipStream_t s, bool with_static = true) {
    cur_stream = s;
    core(x);
    finish_item(x, nullptr, y_phys, x_next);
    noise_next_step();
    if (x_next) copy_layout_groups(x, frc, x_next, (int64_t)cfg.image_height * cfg.image_width, s, with_static);
  }
  void rollout(const float* x0, const float* const* frc, int n, float* const* y_phys, float* x_final, hipStream_t s) override {
    check_ready();
    if (band_on) throw StateError("this engine is in lat-band mode: drive it with wx_band_begin / wx_band_resume");
    if (cfg.frames != 1 || cfg.output_frames != 1) throw ConfigError("wx_rollout needs frames == output_frames == 1");
    if (n < 1) throw ConfigError("wx_rollout: n_steps must be >= 1");
    if (!x0) throw ConfigError("wx_rollout: x0 is NULL");
    if (n_prog < 0) throw StateError("wx_rollout needs wx_set_layout first");
    if (Ho != cfg.image_height || Wo != cfg.image_width) throw ConfigError("wx_rollout needs output size == input size");
    if (!have_denorm && y_phys) {
      for (int t = 0; t < n; ++t) if (y_phys[t]) throw StateError("wx_rollout with y_phys needs wx_set_denorm first");
    }
    const int64_t plane = (int64_t)cfg.image_height * cfg.image_width;
    const size_t x_bytes = (size_t)C_in * plane * sizeof(float);
    if (n_dyn > 0)
      for (int t = 0; t < n; ++t)
        if ((t < n - 1 || x_final) && (!frc || !frc[t])) throw ConfigError("wx_rollout: forcing pointer is NULL but the layout has dynamic forcing channels");
    if (!roll_x[0]) {
      roll_x[0] = (float*)mem.alloc(x_bytes);
      roll_x[1] = (float*)mem.alloc(x_bytes);
    }
    if (n_dyn > roll_frc_ndyn) {   // a later layout may carry more forcing planes than the first call's
      roll_invalidate();           // (the captured copies point at the old buffer)
      roll_frc = (float*)mem.alloc((size_t)n_dyn * plane * sizeof(float));
      roll_frc_ndyn = n_dyn;
    }
    const bool graph = want_graph() && roll_warm;
    if (!graph) {
      const float* x = x0;
      for (int t = 0; t < n; ++t) {
        const bool next = t < n - 1 || x_final;
        float* xn = next ? roll_x[t & 1] : nullptr;
        if (xn == x) throw ConfigError("wx_rollout: x0 aliases an internal state buffer");
        // the fixed (static) planes never change during a rollout: each ping-pong buffer receives them once per call
        step_body(x, frc ? frc[t] : nullptr, y_phys ? y_phys[t] : nullptr, xn, s, /*with_static=*/t < 2);
        if (xn) x = xn;
      }
      if (x_final) WX_HIP(hipMemcpyAsync(x_final, roll_x[(n - 1) & 1], x_bytes, hipMemcpyDeviceToDevice, s));
      roll_warm = true;   // every kernel's launch attributes are set now: later calls may capture
      if (prof_on) drain();
      return;
    }
    // graph path: the caller's stream may be the legacy default stream (not capturable) -> own stream, fenced by events
    if (!roll_stream) {
      WX_HIP(hipStreamCreateWithFlags(&roll_stream, hipStreamNonBlocking));
      WX_HIP(hipEventCreateWithFlags(&roll_ev_in, hipEventDisableTiming));
      WX_HIP(hipEventCreateWithFlags(&roll_ev_out, hipEventDisableTiming));
    }
    WX_HIP(hipEventRecord(roll_ev_in, s));
    WX_HIP(hipStreamWaitEvent(roll_stream, roll_ev_in, 0));
    WX_HIP(hipMemcpyAsync(roll_x[1], x0, x_bytes, hipMemcpyDeviceToDevice, roll_stream));   // step t reads roll_x[(t + 1) & 1]
    for (int t = 0; t < n; ++t) {
      const bool next = t < n - 1 || x_final;
      float* yp = y_phys ? y_phys[t] : nullptr;
      if (next && n_dyn > 0)
        WX_HIP(hipMemcpyAsync(roll_frc, frc[t], (size_t)n_dyn * plane * sizeof(float), hipMemcpyDeviceToDevice, roll_stream));
      const auto key = std::make_tuple(t & 1, (const void*)yp, next ? 1 : 0);
      auto it = roll_graphs.find(key);
      if (it == roll_graphs.end()) {
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        WX_HIP(hipStreamBeginCapture(roll_stream, hipStreamCaptureModeRelaxed));
        try {
          step_body(roll_x[(t + 1) & 1], roll_frc, yp, next ? roll_x[t & 1] : nullptr, roll_stream);
        } catch (...) {
          (void)hipStreamEndCapture(roll_stream, &g);
          if (g) (void)hipGraphDestroy(g);
          throw;
        }
        WX_HIP(hipStreamEndCapture(roll_stream, &g));
        WX_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        WX_HIP(hipGraphDestroy(g));
        if (roll_graphs.size() >= 64) roll_invalidate();   // callers that hand out a fresh y_phys pointer every step: bounded; waits for replays in flight
        it = roll_graphs.emplace(key, ge).first;
      }
      WX_HIP(hipGraphLaunch(it->second, roll_stream));
    }
    if (x_final) WX_HIP(hipMemcpyAsync(x_final, roll_x[(n - 1) & 1], x_bytes, hipMemcpyDeviceToDevice, roll_stream));
    WX_HIP(hipEventRecord(roll_ev_out, roll_stream));
    WX_HIP(hipStreamWaitEvent(s, roll_ev_out, 0));
    cur_stream = s;
  }
};

}  // namespace wx

#include "wx_abi.h"

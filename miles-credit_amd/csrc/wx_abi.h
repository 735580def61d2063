// wxengine: the C ABI of include/wxengine.h -- exception-to-status mapping and the extern "C" wrappers of every handle type
// (engine, lat-band plan, pre block, post block, window attention, Swin stage, FuXi model).  Included last by wx_engine.hip: it
// needs every class defined there and in the headers before it.
#pragma once

namespace wx {
static thread_local std::string g_last_error;
}  // namespace wx

// every opaque handle of the header: the tag keeps its name, the body is the wrapped object
template <class Impl>
struct Handle {
  std::unique_ptr<Impl> impl;
};
struct wx_engine : Handle<wx::EngineBase> {};

template <typename F>
static int guarded(F&& fn) {
  try {
    fn();
    return WX_OK;
  } catch (const wx::ConfigError& e) { wx::g_last_error = e.what(); return WX_ERR_INVALID;
  } catch (const wx::StateError& e) { wx::g_last_error = e.what(); return WX_ERR_STATE;
  } catch (const wx::MissingError& e) { wx::g_last_error = e.what(); return WX_ERR_MISSING;
  } catch (const wx::ShapeError& e) { wx::g_last_error = e.what(); return WX_ERR_SHAPE;
  } catch (const wx::HipError& e) { wx::g_last_error = e.what(); return WX_ERR_HIP;
  } catch (const std::exception& e) { wx::g_last_error = e.what(); return WX_ERR_INVALID; }
}
// the first test of a wrapper that takes a handle: a live one, or `what` as WX_ERR_INVALID
template <typename H>
static void need(const H* h, const char* what) {
  if (!h || !h->impl) throw wx::ConfigError(what);
}
static void need_device(int device, const char* fn) {
  int ndev = 0;
  WX_HIP(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) throw wx::ConfigError(std::string(fn) + ": no such GPU device");
}
// a wrapped object's std::runtime_error becomes the ABI error class `Err`; a HIP failure keeps its own
template <typename Err, typename F>
static void remap(F&& fn) {
  try {
    fn();
  } catch (const wx::HipError&) {
    throw;
  } catch (const std::runtime_error& e) {
    throw Err(e.what());
  }
}

// wx_X_create of a device product: a null argument, then `check()`'s reason (it needs no device to be told), then the device,
// then the object `make()` news
template <typename H, typename Check, typename Make>
static int create(const char* fn, H** out, bool args_ok, int device, Check&& check, Make&& make) {
  return guarded([&] {
    if (!out || !args_ok) throw wx::ConfigError(std::string(fn) + ": null argument");
    const std::string why = check();
    if (!why.empty()) throw wx::ConfigError(std::string(fn) + ": " + why);
    need_device(device, fn);
    std::unique_ptr<H> h(new H);
    h->impl.reset(make());
    *out = h.release();
  });
}
static std::string no_check() { return {}; }
// every other wrapper of a device product: a live handle (or `what`), then `fn`; use_remapped also turns the object's
// std::runtime_error into WX_ERR_INVALID
template <typename H, typename F>
static int use(const H* h, const char* what, F&& fn) {
  return guarded([&] { need(h, what); fn(); });
}
template <typename H, typename F>
static int use_remapped(const H* h, const char* what, F&& fn) {
  return use(h, what, [&] { remap<wx::ConfigError>(fn); });
}

extern "C" {

int wx_create(const wx_config* cfg, int device, wx_handle* out) {
  return guarded([&] {
    if (!cfg || !out) throw wx::ConfigError("wx_create: null argument");
    if (cfg->precision != WX_PREC_FP32 && cfg->precision != WX_PREC_FP32_SPLIT && cfg->precision != WX_PREC_BF16)
      throw wx::ConfigError("wx_create: unknown precision");
    { const wx::ModelSpec check(*cfg); }   // the config's own faults first: they need no device to be told
    need_device(device, "wx_create");
    WX_HIP(hipSetDevice(device));
    std::unique_ptr<wx_engine> h(new wx_engine);
    const wx::Options opt = wx::Options::from_env();
    if (cfg->precision == WX_PREC_FP32) h->impl.reset(new wx::Engine<float>(*cfg, device, opt));
    else if (cfg->precision == WX_PREC_FP32_SPLIT) h->impl.reset(new wx::Engine<float>(*cfg, device, opt, /*split=*/true));
    else if (cfg->precision == WX_PREC_BF16) h->impl.reset(new wx::Engine<wx::bf16_t>(*cfg, device, opt));
    else throw wx::ConfigError("wx_create: unknown precision");
    *out = h.release();
  });
}
int wx_destroy(wx_handle h) {
  return guarded([&] { delete h; });
}
int wx_load_tensor(wx_handle h, const char* key, const float* data, int ndim, const int64_t* shape) {
  return guarded([&] { need(h, "null engine handle"); if (!key || !data || !shape) throw wx::ConfigError("wx_load_tensor: null argument"); h->impl->load_tensor(key, data, ndim, shape); });
}
int wx_finalize_weights(wx_handle h) { return guarded([&] { need(h, "null engine handle"); h->impl->finalize(); }); }
int wx_num_tensors(wx_handle h) { return (h && h->impl) ? h->impl->num_tensors() : WX_ERR_INVALID; }
int wx_tensor_info(wx_handle h, int index, const char** key, int* ndim, int64_t shape[8]) {
  return guarded([&] { need(h, "null engine handle"); h->impl->tensor_info(index, key, ndim, shape); });
}
int wx_set_denorm(wx_handle h, const float* mean, const float* stdv, int n) {
  return guarded([&] { need(h, "null engine handle"); if (!mean || !stdv) throw wx::ConfigError("wx_set_denorm: null argument"); h->impl->set_denorm(mean, stdv, n); });
}
int wx_set_tracer_fixer(wx_handle h, const int32_t* inds, const float* thres, const float* thres_max, int n, int denorm) {
  return guarded([&] { need(h, "null engine handle"); if (n > 0 && (!inds || !thres)) throw wx::ConfigError("wx_set_tracer_fixer: null argument"); h->impl->set_tracer(inds, thres, thres_max, n, denorm); });
}
int wx_set_layout(wx_handle h, int n_prog, int n_static, int n_dyn) {
  return guarded([&] { need(h, "null engine handle"); h->impl->set_layout(n_prog, n_static, n_dyn); });
}
int wx_set_layout_groups(wx_handle h, int n_groups, const int32_t* kind, const int32_t* x_start, const int32_t* src_start, const int32_t* count) {
  return guarded([&] { need(h, "null engine handle"); h->impl->set_layout_groups(n_groups, kind, x_start, src_start, count); });
}
int wx_forward(wx_handle h, const float* x_dev, float* y_dev, int batch, void* stream) {
  return guarded([&] { need(h, "null engine handle"); if (!x_dev || !y_dev) throw wx::ConfigError("wx_forward: null pointer"); h->impl->forward(x_dev, y_dev, batch, (hipStream_t)stream); });
}
int wx_step(wx_handle h, const float* x_dev, const float* frc_dev, float* y_dev, float* y_phys_dev, float* x_next_dev, void* stream) {
  return guarded([&] { need(h, "null engine handle"); if (!x_dev) throw wx::ConfigError("wx_step: null input"); h->impl->step(x_dev, frc_dev, y_dev, y_phys_dev, x_next_dev, (hipStream_t)stream); });
}
int wx_rollout(wx_handle h, const float* x0_dev, const float* const* frc_dev, int n_steps, float* const* y_phys_dev, float* x_final_dev,
               void* stream) {
  return guarded([&] { need(h, "null engine handle"); h->impl->rollout(x0_dev, frc_dev, n_steps, y_phys_dev, x_final_dev, (hipStream_t)stream); });
}
int wx_band_enable(wx_handle h, int rank, int nranks) { return guarded([&] { need(h, "null engine handle"); h->impl->band_enable(rank, nranks); }); }
int wx_band_info(wx_handle h, int* own_row0, int* own_rows, int64_t* send_bytes, int64_t* recv_bytes, int* n_exchanges) {
  return guarded([&] {
    need(h, "null engine handle");
    if (!own_row0 || !own_rows || !send_bytes || !recv_bytes || !n_exchanges) throw wx::ConfigError("wx_band_info: null argument");
    h->impl->band_info(own_row0, own_rows, send_bytes, recv_bytes, n_exchanges);
  });
}
int wx_band_set_staging(wx_handle h, void* send_dev, int64_t send_bytes, void* recv_dev, int64_t recv_bytes) {
  return guarded([&] { need(h, "null engine handle"); h->impl->band_set_staging(send_dev, send_bytes, recv_dev, recv_bytes); });
}
int wx_band_exchange(wx_handle h, int xid, wx_band_msg* sends, int cap_sends, int* n_sends, wx_band_msg* recvs, int cap_recvs, int* n_recvs) {
  return guarded([&] {
    need(h, "null engine handle");
    if (!sends || !recvs || !n_sends || !n_recvs) throw wx::ConfigError("wx_band_exchange: null argument");
    h->impl->band_messages_of(xid, sends, cap_sends, n_sends, recvs, cap_recvs, n_recvs);
  });
}
int wx_band_begin(wx_handle h, const float* x_band, const float* frc_band, float* y_band, float* y_phys_band, float* x_next_band, void* stream,
                  int* next_xid) {
  return guarded([&] {
    need(h, "null engine handle");
    if (!next_xid) throw wx::ConfigError("wx_band_begin: null next_xid");
    *next_xid = h->impl->band_begin(x_band, frc_band, y_band, y_phys_band, x_next_band, (hipStream_t)stream);
  });
}
int wx_band_resume(wx_handle h, int* next_xid) {
  return guarded([&] {
    need(h, "null engine handle");
    if (!next_xid) throw wx::ConfigError("wx_band_resume: null next_xid");
    *next_xid = h->impl->band_resume();
  });
}
int wx_band_comm_stream(wx_handle h, void* adopt_stream, void** stream_out) {
  return guarded([&] {
    need(h, "null engine handle");
    void* st = h->impl->band_comm_stream(adopt_stream);
    if (stream_out) *stream_out = st;
  });
}
int wx_band_rccl_unique_id(uint8_t id[128]) {
  return guarded([&] {
    if (!id) throw wx::ConfigError("wx_band_rccl_unique_id: null argument");
    wx::RcclApi& api = wx::RcclApi::get();
    ncclUniqueId u;
    api.check(api.GetUniqueId(&u), "ncclGetUniqueId");
    static_assert(sizeof(u) == 128, "ncclUniqueId size");
    std::memcpy(id, &u, 128);
  });
}
int wx_band_rccl_init(wx_handle h, const uint8_t id[128]) {
  return guarded([&] {
    need(h, "null engine handle");
    if (!id) throw wx::ConfigError("wx_band_rccl_init: null argument");
    ncclUniqueId u;
    std::memcpy(&u, id, 128);
    h->impl->band_rccl_init(u);
  });
}
int wx_band_step_rccl(wx_handle h, const float* x_band, const float* frc_band, float* y_band, float* y_phys_band, float* x_next_band,
                      void* stream) {
  return guarded([&] { need(h, "null engine handle"); h->impl->band_step_rccl(x_band, frc_band, y_band, y_phys_band, x_next_band, (hipStream_t)stream); });
}
// host-only plan: the model spec supplies the derived geometry (no HIP call is made)
struct wx_band_plan_s { wx::BandPlan plan; };
int wx_band_plan_create(const wx_config* cfg, int nranks, wx_band_plan* out) {
  return guarded([&] {
    if (!cfg || !out) throw wx::ConfigError("wx_band_plan_create: null argument");
    if (nranks < 1) throw wx::ConfigError("wx_band_plan_create: nranks must be >= 1");
    std::unique_ptr<wx_band_plan_s> p(new wx_band_plan_s);
    const wx::ModelSpec spec(*cfg);
    wx::band_check_supported(spec);
    // the plan depends on geometry and the element size, not on arithmetic
    const bool f32 = cfg->precision == WX_PREC_FP32 || cfg->precision == WX_PREC_FP32_SPLIT;
    p->plan.build(wx::band_model(spec, nranks, f32 ? 4 : 2, 0));
    *out = p.release();
  });
}
int wx_band_plan_destroy(wx_band_plan p) { return guarded([&] { delete p; }); }
int wx_band_plan_num_exchanges(wx_band_plan p, int* n) {
  return guarded([&] { if (!p || !n) throw wx::ConfigError("null argument"); *n = (int)p->plan.xs.size(); });
}
int wx_band_plan_exchange_name(wx_band_plan p, int xid, const char** name) {
  return guarded([&] {
    if (!p || !name || xid < 0 || xid >= (int)p->plan.xs.size()) throw wx::ConfigError("wx_band_plan_exchange_name: bad argument");
    *name = p->plan.xs[xid].name.c_str();
  });
}
int wx_band_plan_messages(wx_band_plan p, int xid, int rank, wx_band_msg* sends, int cap_sends, int* n_sends, wx_band_msg* recvs,
                          int cap_recvs, int* n_recvs) {
  return guarded([&] {
    if (!p || !sends || !recvs || !n_sends || !n_recvs || xid < 0 || xid >= (int)p->plan.xs.size() || rank < 0 || rank >= p->plan.m.n)
      throw wx::ConfigError("wx_band_plan_messages: bad argument");
    std::vector<wx::BandMsg> s, r;
    wx::band_messages(p->plan.xs[xid], rank, &s, &r);
    if ((int)s.size() > cap_sends || (int)r.size() > cap_recvs) throw wx::ConfigError("wx_band_plan_messages: arrays too small");
    for (size_t i = 0; i < s.size(); ++i) sends[i] = wx_band_msg{s[i].peer, s[i].offset, s[i].bytes};
    for (size_t i = 0; i < r.size(); ++i) recvs[i] = wx_band_msg{r[i].peer, r[i].offset, r[i].bytes};
    *n_sends = (int)s.size(); *n_recvs = (int)r.size();
  });
}
int wx_band_plan_partition(wx_band_plan p, int which, int32_t* starts) {
  return guarded([&] {
    if (!p || !starts || which < 0 || which > 8) throw wx::ConfigError("wx_band_plan_partition: bad argument");
    const std::vector<int>& v = which < 4 ? p->plan.g.ps[which] : which < 8 ? p->plan.g.pl[which - 4] : p->plan.g.po;
    for (size_t i = 0; i < v.size(); ++i) starts[i] = v[i];
  });
}
int wx_set_noise(wx_handle h, uint64_t seed, int member0, int step) {
  return guarded([&] { need(h, "null engine handle"); h->impl->set_noise(seed, member0, step); });
}
int wx_set_noise_tape(wx_handle h, const float* const* draws, int n) {
  return guarded([&] { need(h, "null engine handle"); h->impl->set_noise_tape(draws, n); });
}
int wx_set_debug(wx_handle h, int level) { return guarded([&] { need(h, "null engine handle"); h->impl->set_debug(level); }); }
int wx_debug_read(wx_handle h, const char* name, float* host_out, int64_t capacity, int64_t shape[3]) {
  return guarded([&] { need(h, "null engine handle"); if (!name || !shape) throw wx::ConfigError("wx_debug_read: null argument"); h->impl->debug_read(name, host_out, capacity, shape); });
}
int wx_query(wx_handle h, const char* key, int64_t* value) {
  return guarded([&] {
    need(h, "null engine handle");
    if (!key || !value) throw wx::ConfigError("wx_query: null argument");
    if (!h->impl->query(key, value)) throw wx::ConfigError(std::string("wx_query: unknown key '") + key + "'");
  });
}
int wx_profile(wx_handle h, int enable) { return guarded([&] { need(h, "null engine handle"); h->impl->profile(enable); }); }
int wx_profile_reset(wx_handle h) { return guarded([&] { need(h, "null engine handle"); h->impl->profile_reset(); }); }
int wx_profile_read(wx_handle h, wx_kernel_stat* out, int capacity, int* count) {
  return guarded([&] { need(h, "null engine handle"); if (!out || !count) throw wx::ConfigError("wx_profile_read: null argument"); *count = h->impl->profile_read(out, capacity); });
}
// ---- pre block (input normalisation + channel concatenation) ---------------------------------------------------------
struct wx_pre : Handle<wx::PreBlock> {};
int wx_pre_create(int n_fields, const int32_t* n_levels, int frames, int H, int W, const float* mean, const float* stdv, int device,
                  wx_pre_handle* out) {
  return create("wx_pre_create", out, n_levels != nullptr, device, no_check,
                [&] { return new wx::PreBlock(n_fields, n_levels, frames, H, W, mean, stdv, device); });
}
int wx_pre_destroy(wx_pre_handle p) { return guarded([&] { delete p; }); }
int wx_pre_channels(wx_pre_handle p, int* channels) {
  return use(p, "wx_pre_channels: null argument", [&] {
    if (!channels) throw wx::ConfigError("wx_pre_channels: null argument");
    *channels = p->impl->channels();
  });
}
int wx_pre_apply(wx_pre_handle p, const float* const* fields_dev, float* x_dev, int batch, void* stream) {
  return use(p, "wx_pre_apply: null argument", [&] {
    if (!fields_dev || !x_dev) throw wx::ConfigError("wx_pre_apply: null argument");
    p->impl->apply(fields_dev, x_dev, batch, (hipStream_t)stream);
  });
}
int wx_pre_set_transforms(wx_pre_handle p, const int32_t* kind, const float* eps, const float* log_eps, const int32_t* n_rules,
                          const int32_t* rule_op, const float* rule_search, const float* rule_fill) {
  return use_remapped(p, "wx_pre_set_transforms: null pre-block handle", [&] {
    if (!kind || !eps || !log_eps || !n_rules || !rule_op || !rule_search || !rule_fill) throw wx::ConfigError("wx_pre_set_transforms: null argument");
    p->impl->set_transforms(kind, eps, log_eps, n_rules, rule_op, rule_search, rule_fill);
  });
}
// ---- inverse scale + inverse transforms of named tensors (csrc/wx_unxform.h) ----------------------------------------------------
struct wx_unxform : Handle<wx::Unxform> {};
int wx_unxform_create(int n_vars, const int32_t* n_levels, int H, int W, const int32_t* kind, const float* eps, const float* log_eps,
                      const int32_t* has_stats, const float* mean, const float* stdv, int device, wx_unxform_handle* out) {
  bool any_stats = false;
  const auto check = [&]() -> std::string {
    if (n_vars < 1 || n_vars > wx::kMaxFields) return "1..64 variables";
    if (H < 1 || W < 1) return "bad geometry";
    for (int v = 0; v < n_vars; ++v) {
      if (n_levels[v] < 1) return "a variable needs at least one level";
      if (kind[v] < wx::kUnxNone || kind[v] > wx::kUnxSquare) return "unknown transform kind " + std::to_string(kind[v]);
      if (kind[v] >= wx::kUnxExpE && kind[v] <= wx::kUnxExp10 && !(eps[v] > 0.f && std::isfinite(eps[v]) && std::isfinite(log_eps[v])))
        return "an exp transform needs a finite eps > 0 and its finite log";
      any_stats = any_stats || has_stats[v] != 0;
    }
    return any_stats && (!mean || !stdv) ? "statistics flagged but mean / std are null" : "";
  };
  return create("wx_unxform_create", out, n_levels && kind && eps && log_eps && has_stats, device, check, [&] {
    return new wx::Unxform(n_vars, n_levels, H, W, kind, eps, log_eps, has_stats, any_stats ? mean : nullptr, any_stats ? stdv : nullptr, device);
  });
}
int wx_unxform_destroy(wx_unxform_handle u) { return guarded([&] { delete u; }); }
int wx_unxform_apply(wx_unxform_handle u, const float* const* src_dev, const int64_t* batch_stride, float* const* dst_dev, int batch,
                     int n_time, void* stream) {
  return use_remapped(u, "wx_unxform_apply: null argument", [&] {
    if (!src_dev || !batch_stride || !dst_dev) throw wx::ConfigError("wx_unxform_apply: null argument");
    u->impl->apply(src_dev, batch_stride, dst_dev, batch, n_time, (hipStream_t)stream);
  });
}
// ---- wind artifact filter (jet mask, masked Gaussian blend; csrc/wx_wind.h) -----------------------------------------------------
struct wx_wind : Handle<wx::Wind> {};
int wx_wind_create(int H, int W, const float* smooth_lat, int n_smooth_lat, const float* smooth_lon, int n_smooth_lon,
                   const float* falloff_lat, int n_falloff_lat, const float* falloff_lon, int n_falloff_lon, int dilation_lat,
                   int dilation_lon, float speed_threshold, int preserve_amplitude, int device, wx_wind_handle* out) {
  const float* const w[4] = {smooth_lat, smooth_lon, falloff_lat, falloff_lon};
  const int n[4] = {n_smooth_lat, n_smooth_lon, n_falloff_lat, n_falloff_lon};
  return create("wx_wind_create", out, true, device,
                [&] { return wx::wind_check_create(H, W, w, n, dilation_lat, dilation_lon, speed_threshold); },
                [&] { return new wx::Wind(H, W, w, n, dilation_lat, dilation_lon, speed_threshold, preserve_amplitude != 0, device); });
}
int wx_wind_destroy(wx_wind_handle f) { return guarded([&] { delete f; }); }
int wx_wind_apply(wx_wind_handle f, const float* u_dev, int64_t u_batch_stride, const float* v_dev, int64_t v_batch_stride, int n_vars,
                  const float* const* src_dev, const int64_t* batch_stride, const int32_t* n_levels, float* const* dst_dev,
                  const int32_t* target_levels, int n_target_levels, int batch, float* mask_out_dev, void* stream) {
  return use_remapped(f, "wx_wind_apply: null wind-filter handle", [&] {
    if (!u_dev || !v_dev || !src_dev || !batch_stride || !n_levels || !dst_dev) throw wx::ConfigError("wx_wind_apply: null argument");
    f->impl->apply(u_dev, u_batch_stride, v_dev, v_batch_stride, n_vars, src_dev, batch_stride, n_levels, dst_dev, target_levels,
                   n_target_levels, batch, mask_out_dev, (hipStream_t)stream);
  });
}
// ---- semi-Lagrangian tracer advection (omega, back-trajectory, trilinear gather; csrc/wx_advect.h) -----------------------------
struct wx_advect : Handle<wx::Advect> {};
int wx_advect_create(int H, int W, int n_levels, const float* a_half, const float* b_half, const float* row_tables, float dlon_rad,
                     float timestep_seconds, int n_iterations, float dp_dlevel_floor, int surface_to_top, int device,
                     wx_advect_handle* out) {
  const float* rows[6];   // the six [H] tables of row_tables, sliced once a non-null row_tables is known
  const auto check = [&] {
    for (int i = 0; i < 6; ++i) rows[i] = row_tables + (size_t)i * (H > 0 ? H : 0);
    return wx::advect_check_create(H, W, n_levels, a_half, b_half, rows, dlon_rad, timestep_seconds, n_iterations, dp_dlevel_floor);
  };
  return create("wx_advect_create", out, row_tables != nullptr, device, check, [&] {
    return new wx::Advect(H, W, n_levels, a_half, b_half, rows, dlon_rad, timestep_seconds, n_iterations, dp_dlevel_floor,
                          surface_to_top != 0, device);
  });
}
int wx_advect_destroy(wx_advect_handle a) { return guarded([&] { delete a; }); }
int wx_advect_apply(wx_advect_handle a, const float* u_dev, int64_t u_batch_stride, const float* v_dev, int64_t v_batch_stride,
                    const float* sp_dev, int64_t sp_batch_stride, const float* omega_dev, int64_t omega_batch_stride, int n_tracers,
                    const float* const* src_dev, const int64_t* batch_stride, float* const* dst_dev, int batch, void* stream) {
  return use_remapped(a, "wx_advect_apply: null advection handle", [&] {
    if (!u_dev || !v_dev || !sp_dev || !src_dev || !batch_stride || !dst_dev) throw wx::ConfigError("wx_advect_apply: null argument");
    a->impl->apply(u_dev, u_batch_stride, v_dev, v_batch_stride, sp_dev, sp_batch_stride, omega_dev, omega_batch_stride, n_tracers,
                   src_dev, batch_stride, dst_dev, batch, (hipStream_t)stream);
  });
}
// ---- hybrid-level interpolation (one set of hybrid levels onto another, linear in log p; csrc/wx_hybrid.h) ----------------------
struct wx_hybrid : Handle<wx::Hybrid> {};
int wx_hybrid_create(int H, int W, int n_src, const float* a_src, const float* b_src, int n_dst, const float* a_dst, const float* b_dst,
                     int device, wx_hybrid_handle* out) {
  return create("wx_hybrid_create", out, true, device,
                [&] { return wx::hybrid_check_create(H, W, n_src, a_src, b_src, n_dst, a_dst, b_dst); },
                [&] { return new wx::Hybrid(H, W, n_src, a_src, b_src, n_dst, a_dst, b_dst, device); });
}
int wx_hybrid_destroy(wx_hybrid_handle h) { return guarded([&] { delete h; }); }
int wx_hybrid_apply(wx_hybrid_handle h, int n_vars, const float* const* src_dev, const int64_t* batch_stride, float* const* dst_dev,
                    int batch, int n_time, const float* sp_dev, int64_t sp_batch_stride, void* stream) {
  return use_remapped(h, "wx_hybrid_apply: null hybrid-interpolation handle", [&] {
    if (!src_dev || !batch_stride || !dst_dev || !sp_dev) throw wx::ConfigError("wx_hybrid_apply: null argument");
    h->impl->apply(n_vars, src_dev, batch_stride, dst_dev, batch, n_time, sp_dev, sp_batch_stride, (hipStream_t)stream);
  });
}
// ---- horizontal regridding (an ESMF sparse weight matrix on every plane, sliced-ELL SpMM; csrc/wx_regrid.h) -------------------------
struct wx_regrid : Handle<wx::Regrid> {};
int wx_regrid_create(int64_t n_a, int64_t n_b, const int64_t* row_ptr, const int32_t* col, const float* val, int device,
                     wx_regrid_handle* out) {
  return create("wx_regrid_create", out, true, device, [&] { return wx::regrid_check_create(n_a, n_b, row_ptr, col, val); },
                [&] { return new wx::Regrid(n_a, n_b, row_ptr, col, val, device); });
}
int wx_regrid_destroy(wx_regrid_handle h) { return guarded([&] { delete h; }); }
int wx_regrid_apply(wx_regrid_handle h, int n_vars, const float* const* src_dev, const int64_t* batch_stride, const int32_t* planes_per_item,
                    int batch, float* const* dst_dev, void* stream) {
  return use_remapped(h, "wx_regrid_apply: null regridding handle", [&] {
    if (!src_dev || !batch_stride || !planes_per_item || !dst_dev) throw wx::ConfigError("wx_regrid_apply: null argument");
    h->impl->apply(n_vars, src_dev, batch_stride, planes_per_item, batch, dst_dev, (hipStream_t)stream);
  });
}
// ---- TISR forcing (top-of-atmosphere incident solar radiation per step, a coefficient table and one sum per point; csrc/wx_tisr.h) ----
struct wx_tisr : Handle<wx::Tisr> {};
int wx_tisr_create(int ny, int nx, const float* lat_host, const float* lon_host, int n_tsi, const float* tsi_times_host,
                   const float* tsi_values_host, int device, wx_tisr_handle* out) {
  return create("wx_tisr_create", out, true, device,
                [&] { return wx::tisr_check_create(ny, nx, lat_host, lon_host, n_tsi, tsi_times_host, tsi_values_host); },
                [&] { return new wx::Tisr(ny, nx, lat_host, lon_host, n_tsi, tsi_times_host, tsi_values_host, device); });
}
int wx_tisr_destroy(wx_tisr_handle h) { return guarded([&] { delete h; }); }
int wx_tisr_compute(wx_tisr_handle h, int n_times, const int64_t* t_end_ns_host, int64_t period_ns, int n_steps, float* dst_dev,
                    int64_t plane_stride, void* stream) {
  return use_remapped(h, "wx_tisr_compute: null TISR handle", [&] {
    h->impl->compute(n_times, t_end_ns_host, period_ns, n_steps, dst_dev, plane_stride, (hipStream_t)stream);
  });
}
// ---- perturbed initial conditions (white, colour-filtered and AR(1) noise on the planes of one member; csrc/wx_perturb.h) ----------
struct wx_perturb : Handle<wx::Perturb> {};
int wx_perturb_create(int H, int W, int kind, const float* S_host, int device, wx_perturb_handle* out) {
  return create("wx_perturb_create", out, true, device, [&] { return wx::perturb_check_create(H, W, kind, S_host); },
                [&] { return new wx::Perturb(H, W, kind, S_host, device); });
}
int wx_perturb_destroy(wx_perturb_handle h) { return guarded([&] { delete h; }); }
int wx_perturb_batch(wx_perturb_handle h, int* planes_out) {
  return use(h, "wx_perturb_batch: null perturbation handle", [&] {
    if (!planes_out) throw wx::ConfigError("wx_perturb_batch: null argument");
    *planes_out = h->impl->batch_planes();
  });
}
int wx_perturb_apply(wx_perturb_handle h, int n_planes, const float* tape_dev, uint64_t seed, int member, int step, float amplitude,
                     const float* chan_scale_host, float rho, const float* prev_dev, int64_t prev_stride, const float* lat_weight_host,
                     const float* x_dev, int64_t x_stride, float* delta_out_dev, int64_t delta_stride, float* x_out_dev, int64_t x_out_stride,
                     void* stream) {
  return use_remapped(h, "wx_perturb_apply: null perturbation handle", [&] {
    h->impl->apply(n_planes, tape_dev, seed, member, step, amplitude, chan_scale_host, rho, prev_dev, prev_stride, lat_weight_host, x_dev, x_stride,
                   delta_out_dev, delta_stride, x_out_dev, x_out_stride, (hipStream_t)stream);
  });
}
// ---- zonal power spectra (PSD, latitude-mean spectra and the two spectral scores from a folded fp64 DFT; csrc/wx_spectrum.h) -------
struct wx_spectrum : Handle<wx::Spectrum> {};
int wx_spectrum_create(int H, int W, const float* lat_w_host, int device, wx_spectrum_handle* out) {
  return create("wx_spectrum_create", out, true, device, [&] { return wx::spectrum_check_create(H, W, lat_w_host); },
                [&] { return new wx::Spectrum(H, W, lat_w_host, device); });
}
int wx_spectrum_destroy(wx_spectrum_handle h) { return guarded([&] { delete h; }); }
int wx_spectrum_apply(wx_spectrum_handle h, int n_planes, const float* a_dev, int64_t a_stride, const float* b_dev, int64_t b_stride, int k_init,
                      float* psd_a_dev, float* psd_b_dev, double* mean_psd_a_dev, double* mean_psd_b_dev, double* mean_amp_a_dev,
                      double* mean_amp_b_dev, double* scores_dev, void* stream) {
  return use_remapped(h, "wx_spectrum_apply: null spectrum handle", [&] {
    h->impl->apply(n_planes, a_dev, a_stride, b_dev, b_stride, k_init, psd_a_dev, psd_b_dev, mean_psd_a_dev, mean_psd_b_dev, mean_amp_a_dev,
                   mean_amp_b_dev, scores_dev, (hipStream_t)stream);
  });
}
// ---- verification metrics (the eight per-variable scores from one two-pass fp64 reduction; csrc/wx_metrics.h) --------------------
struct wx_metrics : Handle<wx::Metrics> {};
int wx_metrics_create(int H, int W, const float* lat_w, int device, wx_metrics_handle* out) {
  return create("wx_metrics_create", out, true, device, [&] { return wx::grid_check(H, W, lat_w); },
                [&] { return new wx::Metrics(H, W, lat_w, device); });
}
int wx_metrics_destroy(wx_metrics_handle h) { return guarded([&] { delete h; }); }
int wx_metrics_apply(wx_metrics_handle h, int n_vars, const float* const* pred_dev, const int64_t* pred_batch_stride,
                     const float* const* target_dev, const int64_t* target_batch_stride, const float* const* clim_dev,
                     const int64_t* clim_level_stride, const int64_t* clim_time_stride, const int32_t* n_levels, const int32_t* n_time,
                     int batch, double eps, float* scores_dev, void* stream) {
  return use_remapped(h, "wx_metrics_apply: null metrics handle", [&] {
    if (!pred_dev || !pred_batch_stride || !target_dev || !target_batch_stride || !n_levels || !n_time || !scores_dev)
      throw wx::ConfigError("wx_metrics_apply: null argument");
    h->impl->apply(n_vars, pred_dev, pred_batch_stride, target_dev, target_batch_stride, clim_dev, clim_level_stride, clim_time_stride,
                   n_levels, n_time, batch, eps, scores_dev, (hipStream_t)stream);
  });
}
// ---- ensemble verification (CRPS, spread, ensemble-mean error from one reading pass; csrc/wx_ensemble.h) ---------------------------
struct wx_ensemble : Handle<wx::Ensemble> {};
int wx_ensemble_create(int H, int W, const float* lat_w, int n_members, int device, wx_ensemble_handle* out) {
  return create("wx_ensemble_create", out, true, device, [&] { return wx::ensemble_check_create(H, W, lat_w, n_members); },
                [&] { return new wx::Ensemble(H, W, lat_w, n_members, device); });
}
int wx_ensemble_destroy(wx_ensemble_handle h) { return guarded([&] { delete h; }); }
int wx_ensemble_apply(wx_ensemble_handle h, int n_vars, const float* const* member_dev, const int64_t* member_batch_stride,
                      const float* const* target_dev, const int64_t* target_batch_stride, const int32_t* n_levels, const int32_t* n_time,
                      int batch, double alpha, float* const* maps_dev, double* planes_dev, void* stream) {
  return use_remapped(h, "wx_ensemble_apply: null ensemble handle", [&] {
    if (!member_dev || !member_batch_stride || !target_dev || !target_batch_stride || !n_levels || !n_time || !planes_dev)
      throw wx::ConfigError("wx_ensemble_apply: null argument");
    h->impl->apply(n_vars, member_dev, member_batch_stride, target_dev, target_batch_stride, n_levels, n_time, batch, alpha, maps_dev,
                   planes_dev, (hipStream_t)stream);
  });
}
// ---- post block ------------------------------------------------------------------------------------------------
struct wx_post : Handle<wx::PostBlock> {};
int wx_post_create(int H, int W, int c_in, int frames, int c_out, int device, wx_post_handle* out) {
  return create("wx_post_create", out, true, device, no_check, [&] { return new wx::PostBlock(H, W, c_in, frames, c_out, device); });
}
int wx_post_destroy(wx_post_handle p) { return guarded([&] { delete p; }); }
int wx_post_set_band(wx_post_handle p, int row0, int rows) {
  return use(p, "null post handle", [&] { p->impl->set_band(row0, rows); });
}
int wx_post_set_grid_sigma(wx_post_handle p, const float* lat2d, const float* lon2d, const float* coef_a, const float* coef_b,
                           int n_levels, int midpoint, int sp_ind) {
  return use(p, "null post-block handle", [&] {
    if (!lat2d || !lon2d || !coef_a || !coef_b) throw wx::ConfigError("wx_post_set_grid_sigma: null argument");
    p->impl->set_grid_sigma(lat2d, lon2d, coef_a, coef_b, n_levels, midpoint, sp_ind);
  });
}
int wx_post_set_grid(wx_post_handle p, const float* lat2d, const float* lon2d, const float* p_levels, int n_levels, int midpoint) {
  return use(p, "null post-block handle", [&] {
    if (!lat2d || !lon2d || !p_levels) throw wx::ConfigError("wx_post_set_grid: null argument");
    p->impl->set_grid(lat2d, lon2d, p_levels, n_levels, midpoint);
  });
}
int wx_post_set_stats(wx_post_handle p, const float* mi, const float* si, const float* mo, const float* so) {
  return use(p, "null post-block handle", [&] {
    if (!mi || !si || !mo || !so) throw wx::ConfigError("wx_post_set_stats: null argument");
    p->impl->set_stats(mi, si, mo, so);
  });
}
int wx_post_add_tracer_fixer(wx_post_handle p, const int32_t* inds, const float* thres, const float* thres_max, int n, int denorm) {
  return use(p, "null post-block handle", [&] {
    if (n < 1 || !inds || !thres) throw wx::ConfigError("wx_post_add_tracer_fixer: bad argument");
    p->impl->add_tracer(inds, thres, thres_max, n, denorm);
  });
}
int wx_post_add_mass_fixer(wx_post_handle p, int q_start, int fix_level_num, int denorm) {
  return use(p, "null post-block handle", [&] { p->impl->add_mass(q_start, fix_level_num, denorm); });
}
int wx_post_add_water_fixer(wx_post_handle p, int q_start, int precip_ind, int evapor_ind, float n_seconds, int denorm) {
  return use(p, "null post-block handle", [&] { p->impl->add_water(q_start, precip_ind, evapor_ind, n_seconds, denorm); });
}
int wx_post_add_energy_fixer_signed(wx_post_handle p, int T_start, int q_start, int U_start, int V_start, int n_toa,
                                    const int32_t* toa_inds, const float* toa_signs, int n_srf, const int32_t* srf_inds,
                                    const float* srf_signs, const float* gph_surf, float n_seconds, int denorm) {
  return use(p, "null post-block handle", [&] {
    if (!toa_inds || !toa_signs || !srf_inds || !srf_signs || !gph_surf) throw wx::ConfigError("wx_post_add_energy_fixer_signed: null argument");
    p->impl->add_energy_signed(T_start, q_start, U_start, V_start, n_toa, toa_inds, toa_signs, n_srf, srf_inds, srf_signs, gph_surf,
                               n_seconds, denorm);
  });
}
int wx_post_add_energy_fixer_updown(wx_post_handle p, int T_start, int q_start, int U_start, int V_start, const int32_t flux_inds[9],
                                    const float* gph_surf, float n_seconds, int denorm) {
  return use(p, "null post-block handle", [&] {
    if (!flux_inds || !gph_surf) throw wx::ConfigError("wx_post_add_energy_fixer_updown: null argument");
    p->impl->add_energy_updown(T_start, q_start, U_start, V_start, flux_inds, gph_surf, n_seconds, denorm);
  });
}
int wx_post_add_energy_fixer(wx_post_handle p, int T_start, int q_start, int U_start, int V_start, const int32_t rad_inds[6],
                             const float* gph_surf, float n_seconds, int denorm) {
  return use(p, "null post-block handle", [&] {
    if (!rad_inds || !gph_surf) throw wx::ConfigError("wx_post_add_energy_fixer: null argument");
    p->impl->add_energy(T_start, q_start, U_start, V_start, rad_inds, gph_surf, n_seconds, denorm);
  });
}
int wx_post_apply(wx_post_handle p, const float* x_dev, float* y_dev, void* stream) {
  return use(p, "null post-block handle", [&] {
    if (!x_dev || !y_dev) throw wx::ConfigError("wx_post_apply: null pointer");
    p->impl->apply(x_dev, y_dev, (hipStream_t)stream);
  });
}
int wx_attach_postblock(wx_handle h, wx_post_handle p) {
  return guarded([&] { need(h, "null engine handle"); h->impl->attach_post(p ? p->impl.get() : nullptr); });
}

// ---- pressure-level products (geopotential, model -> pressure levels, MSLP; csrc/wx_diag.h) ------------------------------------
struct wx_diag : Handle<wx::Diag> {};
int wx_diag_create(int H, int W, int n_levels, int device, wx_diag_handle* out) {
  return create("wx_diag_create", out, true, device,
                [&] { return n_levels < 2 || n_levels > wx::kDiagMaxLevels ? "n_levels must be 2 .. 137" : ""; }, [&] {
                  wx::Diag* d = nullptr;
                  remap<wx::ConfigError>([&] { d = new wx::Diag(H, W, n_levels, device); });
                  return d;
                });
}
int wx_diag_destroy(wx_diag_handle d) { return guarded([&] { delete d; }); }
int wx_diag_set_levels(wx_diag_handle d, const float* a_half, const float* b_half, const float* a_mid, const float* b_mid, int flip_vertical) {
  return use_remapped(d, "null diagnostics handle", [&] { d->impl->set_levels(a_half, b_half, a_mid, b_mid, flip_vertical); });
}
int wx_diag_set_pressure_levels(wx_diag_handle d, const float* p_pa, int n_plev, float temp_height) {
  return use_remapped(d, "null diagnostics handle", [&] { d->impl->set_pressure_levels(p_pa, n_plev, temp_height); });
}
int wx_diag_apply(wx_diag_handle d, int batch, int n_time, const float* T, const float* q, const float* sp, const float* phis,
                  int phis_n_time, const float* t_near_surface, const float* const* fields, int n_fields, float* z_model_out,
                  float* const* plev_out, float* mslp_out, void* stream) {
  return use_remapped(d, "null diagnostics handle", [&] {
    d->impl->apply(batch, n_time, T, q, sp, phis, phis_n_time, t_near_surface, fields, n_fields, z_model_out, plev_out, mslp_out,
                   (hipStream_t)stream);
  });
}

// ---- standalone window attention (the Swin / FuXi mode of the attention kernel) -----------------------
struct wx_winattn {
  wx_winattn_desc d;
  int device;
  wx::DeviceArena mem;
  int NP = 0;
  float* bias_dev = nullptr;     // [n_bias_heads][NP][NP], padded keys -1e30, x log2(e) for bf16
  float* logit_dev = nullptr;    // [heads] or nullptr
  int64_t n_bias_stride = 0;     // floats between two heads' tables (0: one table shared by every head)
  wx_winattn(const wx_winattn_desc& desc, int dev) : d(desc), device(dev), mem(dev) {}
};
int wx_winattn_create(const wx_winattn_desc* d, const float* bias_host, int n_bias_heads, const float* logit_scale_host, int device,
                      wx_winattn_handle* out) {
  return guarded([&] {
    if (!d || !out) throw wx::ConfigError("null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw wx::HipError("no HIP device visible: wxengine has no CPU fallback");
    const int wsx = d->wsz_x > 0 ? d->wsz_x : d->wsz_y;
    if (d->precision != WX_PREC_FP32 && d->precision != WX_PREC_BF16) throw wx::ConfigError("winattn: unknown precision");
    if (d->head_dim != 32 && d->head_dim != 64 && d->head_dim != 96 && d->head_dim != 128) throw wx::ConfigError("winattn: head_dim must be 32, 64, 96 or 128");
    if (d->heads < 1 || d->C != d->heads * d->head_dim) throw wx::ConfigError("winattn: C must equal heads * head_dim");
    if (d->wsz_y < 1 || wsx < 1 || d->H % d->wsz_y || d->W % wsx) throw wx::ConfigError("winattn: the window must divide the token map");
    if (d->kind != 0 && d->kind != 1 && d->kind != 3) throw wx::ConfigError("winattn: kind must be 0 (block), 1 (dilated) or 3 (shifted block)");
    if (d->kind == 1 && wsx != d->wsz_y) throw wx::ConfigError("winattn: dilated windows must be square");
    if (d->kind == 3 && (d->shift_y < 0 || d->shift_y >= d->wsz_y || d->shift_x < 0 || d->shift_x >= wsx)) throw wx::ConfigError("winattn: shift must lie inside the window");
    const int N = d->wsz_y * wsx;
    if (wx::attn_nkf_tokens(N) > 0 && !wx::window_attn_lds_ok(d->precision == WX_PREC_BF16 ? 2 : 4, wx::attn_nkf_tokens(N), d->head_dim))
      throw wx::ConfigError("winattn: head_dim x window size exceeds the kernel's 160 KB of LDS (fp32: head_dim 96 / 128 take windows of at most 64 tokens)");
    const int nkf = wx::attn_nkf_tokens(N);
    if (nkf < 0 || nkf > 8) throw wx::ConfigError("winattn: at most 128 tokens per window");
    if (n_bias_heads != 0 && n_bias_heads != 1 && n_bias_heads != d->heads) throw wx::ConfigError("winattn: bias for 0, 1 or `heads` heads");
    WX_HIP(hipSetDevice(device));
    auto w = std::make_unique<wx_winattn>(*d, device);
    w->NP = nkf * 16;
    const int NP = w->NP, nb = n_bias_heads > 0 ? n_bias_heads : 1;
    const float l2e = d->precision == WX_PREC_BF16 ? 1.4426950408889634f : 1.0f;   // bf16 softmax runs on exp2
    std::vector<float> tab((size_t)nb * NP * NP, -1.0e30f);
    for (int h = 0; h < nb; ++h)
      for (int q = 0; q < NP; ++q)
        for (int k = 0; k < N; ++k)
          tab[((size_t)h * NP + q) * NP + k] = (q < N && bias_host && n_bias_heads > 0) ? bias_host[((size_t)h * N + q) * N + k] * l2e : 0.f;
    w->bias_dev = w->mem.upload(tab.data(), tab.size());
    w->n_bias_stride = nb > 1 ? (int64_t)NP * NP : 0;
    if (logit_scale_host) {
      std::vector<float> ls(d->heads);
      for (int h = 0; h < d->heads; ++h) ls[h] = logit_scale_host[h] * l2e;
      w->logit_dev = w->mem.upload(ls.data(), ls.size());
    }
    *out = w.release();
  });
}
int wx_winattn_destroy(wx_winattn_handle w) { return guarded([&] { delete w; }); }
int wx_winattn_apply(wx_winattn_handle w, const void* qkv_dev, void* out_dev, void* stream) {
  return guarded([&] {
    if (!w) throw wx::StateError("null winattn handle");
    if (!qkv_dev || !out_dev) throw wx::ConfigError("winattn: null tensor pointer");
    WX_HIP(hipSetDevice(w->device));
    const wx_winattn_desc& d = w->d;
    wx::AttnParams p;
    p.trace = nullptr; p.tb = nullptr; p.pack = 1;
    p.qkv = qkv_dev; p.ld_qkv = 3 * (int64_t)d.C; p.out = out_dev; p.ld_out = d.C;
    p.bias = w->bias_dev;
    p.H = d.H; p.W = d.W; p.C = d.C; p.heads = d.heads; p.wsz = d.wsz_y; p.wsz_x = d.wsz_x > 0 ? d.wsz_x : d.wsz_y; p.kind = d.kind;
    p.shift_y = d.kind == 3 ? d.shift_y : 0; p.shift_x = d.kind == 3 ? d.shift_x : 0;
    const float l2e = d.precision == WX_PREC_BF16 ? 1.4426950408889634f : 1.0f;
    p.mask_val = d.mask_value * l2e;
    p.mask_x = (d.kind == 3 && (d.mask_axes & 2)) ? 1 : 0;
    p.logit_scale = w->logit_dev;
    // scores: cosine mode has its scale in q (logit_scale); otherwise softmax_scale (x log2 e on the exp2 path)
    p.scale = w->logit_dev ? 1.0f : d.softmax_scale;                                             // fp32 path: scores * scale
    p.q_scale = (!w->logit_dev && d.precision == WX_PREC_BF16) ? d.softmax_scale * l2e : 0.f;   // bf16 path: scale rides on q
    p.bias_head_stride = w->n_bias_stride;
    if (d.precision == WX_PREC_BF16) wx::launch_window_attn_any<wx::bf16_t>(p, d.head_dim, (hipStream_t)stream);
    else wx::launch_window_attn_any<float>(p, d.head_dim, (hipStream_t)stream);
  });
}

// ---- a stage of Swin V2 (Cr) blocks (BASELINE config 5: the FuXi U-Transformer's stage) -----------------
struct wx_swin : Handle<wx::SwinStageBase> {};
int wx_swin_create(const wx_swin_desc* d, int device, wx_swin_handle* out) {
  return guarded([&] {
    if (!d || !out) throw wx::ConfigError("null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw wx::HipError("no HIP device visible: wxengine has no CPU fallback");
    if (d->precision != WX_PREC_FP32 && d->precision != WX_PREC_BF16 && d->precision != WX_PREC_FP32_SPLIT) throw wx::ConfigError("swin: unknown precision");
    if (d->depth < 1 || d->H < 1 || d->W < 1 || d->heads < 1 || d->wsz_y < 1 || d->wsz_x < 1) throw wx::ConfigError("swin: bad geometry");
    wx::SwinDesc sd{d->H, d->W, d->C, d->heads, d->wsz_y, d->wsz_x, d->depth, d->hidden, d->shift_y, d->shift_x, d->mask_value, d->ln_eps};
    if (d->mask_axes != 0 && d->mask_axes != 1 && d->mask_axes != 3) throw wx::ConfigError("swin: mask_axes must be 1 (latitude) or 3 (both axes)");
    sd.mask_axes = d->mask_axes == 3 ? 3 : 1;
    const wx::Options opt = wx::Options::from_env();
    auto w = std::make_unique<wx_swin>();
    remap<wx::ConfigError>([&] {
      if (d->precision == WX_PREC_BF16) w->impl = std::make_unique<wx::SwinStage<wx::bf16_t>>(sd, device, opt);
      else w->impl = std::make_unique<wx::SwinStage<float>>(sd, device, opt, d->precision == WX_PREC_FP32_SPLIT);
    });
    *out = w.release();
  });
}
int wx_swin_load(wx_swin_handle w, int block, const char* name, const float* host, int64_t count) {
  return guarded([&] {
    if (!w || !name || !host) throw wx::ConfigError("swin: null argument");
    remap<wx::ShapeError>([&] { w->impl->load(block, name, host, count); });
  });
}
int wx_swin_finalize(wx_swin_handle w) {
  return guarded([&] {
    if (!w) throw wx::StateError("null swin handle");
    remap<wx::StateError>([&] { w->impl->finalize(); });
  });
}
int wx_swin_apply(wx_swin_handle w, const void* x_in_dev, void* x_out_dev, void* stream) {
  return guarded([&] {
    if (!w) throw wx::StateError("null swin handle");
    if (!x_in_dev || !x_out_dev) throw wx::ConfigError("swin: null tensor pointer");
    remap<wx::StateError>([&] { w->impl->apply(x_in_dev, x_out_dev, (hipStream_t)stream); });
  });
}
int wx_swin_flops(wx_swin_handle w, double* flops) {
  return guarded([&] { if (!w || !flops) throw wx::ConfigError("swin: null argument"); *flops = w->impl->flops(); });
}
int wx_swin_destroy(wx_swin_handle w) { return guarded([&] { delete w; }); }

// ---- the FuXi forward (BASELINE config 5; credit/models/fuxi.py:454-500) -----------------------------------------------------------
struct wx_fuxi : Handle<wx::FuxiBase> {};
int wx_fuxi_create(const wx_fuxi_desc* d, int device, wx_fuxi_handle* out) {
  return guarded([&] {
    if (!d || !out) throw wx::ConfigError("null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw wx::HipError("no HIP device visible: wxengine has no CPU fallback");
    if (d->precision != WX_PREC_FP32 && d->precision != WX_PREC_BF16 && d->precision != WX_PREC_FP32_SPLIT) throw wx::ConfigError("fuxi: unknown precision");
    if (d->H < 1 || d->W < 1 || d->C_in < 1 || d->C_out < 1 || d->frames < 1 || d->patch_h < 1 || d->patch_w < 1 || d->dim < 1 || d->heads < 1 ||
        d->window < 1 || d->depth < 1 || d->groups_down < 1 || d->groups_up < 1)
      throw wx::ConfigError("fuxi: bad geometry");
    if (d->stage_variant != WX_STAGE_V2_CR && d->stage_variant != WX_STAGE_TIMM_V2) throw wx::ConfigError("fuxi: unknown stage_variant");
    wx::FuxiDesc fd{d->H, d->W, d->C_in, d->C_out, d->frames, d->patch_h, d->patch_w, d->dim, d->heads, d->window, d->depth, d->groups_down, d->groups_up};
    fd.stage_variant = d->stage_variant;
    const wx::Options opt = wx::Options::from_env();
    auto w = std::make_unique<wx_fuxi>();
    remap<wx::ConfigError>([&] {
      if (d->precision == WX_PREC_BF16) w->impl = std::make_unique<wx::FuxiModel<wx::bf16_t>>(fd, device, opt);
      else w->impl = std::make_unique<wx::FuxiModel<float>>(fd, device, opt, d->precision == WX_PREC_FP32_SPLIT);
    });
    *out = w.release();
  });
}
int wx_fuxi_load(wx_fuxi_handle w, const char* name, const float* host, int64_t count) {
  return guarded([&] {
    if (!w || !name || !host) throw wx::ConfigError("fuxi: null argument");
    remap<wx::ShapeError>([&] { w->impl->load(name, host, count); });
  });
}
int wx_fuxi_finalize(wx_fuxi_handle w) {
  return guarded([&] {
    if (!w) throw wx::StateError("null fuxi handle");
    remap<wx::StateError>([&] { w->impl->finalize(); });
  });
}
int wx_fuxi_forward(wx_fuxi_handle w, const float* x_dev, float* y_dev, void* stream) {
  return guarded([&] {
    if (!w) throw wx::StateError("null fuxi handle");
    if (!x_dev || !y_dev) throw wx::ConfigError("fuxi: null tensor pointer");
    remap<wx::StateError>([&] { w->impl->forward(x_dev, y_dev, (hipStream_t)stream); });
  });
}
int wx_fuxi_debug_map(wx_fuxi_handle w, const char* name, float* host, int64_t capacity, int64_t shape[3]) {
  return guarded([&] {
    if (!w || !name || !shape) throw wx::ConfigError("fuxi: null argument");
    remap<wx::ShapeError>([&] { w->impl->debug_copy(name, host, capacity, shape); });
  });
}
int wx_fuxi_query(wx_fuxi_handle w, const char* key, int64_t* value) {
  return guarded([&] {
    if (!w) throw wx::StateError("null fuxi handle");
    if (!key || !value) throw wx::ConfigError("wx_fuxi_query: null argument");
    if (!w->impl->query(key, value)) throw wx::ConfigError(std::string("wx_fuxi_query: unknown key '") + key + "'");
  });
}
int wx_fuxi_flops(wx_fuxi_handle w, double* flops) {
  return guarded([&] { if (!w || !flops) throw wx::ConfigError("fuxi: null argument"); *flops = w->impl->flops(); });
}
int wx_fuxi_destroy(wx_fuxi_handle w) { return guarded([&] { delete w; }); }

// ---- spherical harmonic transforms (scalar pair, vector analysis, spectra; csrc/wx_sht.h, declared in include/wxengine_sht.h) --------
struct wx_sht : Handle<wx::Sht> {};
int wx_sht_create(int nlat, int nlon, int lmax, int mmax, const double* theta_host, const double* w_host, int csphase, const char* norm,
                  int device, wx_sht_handle* out) {
  return create("wx_sht_create", out, theta_host && w_host, device, [&] { return wx::sht_check_create(nlat, nlon, lmax, mmax, theta_host, w_host, norm); },
                [&] { return new wx::Sht(nlat, nlon, lmax, mmax, theta_host, w_host, csphase, device); });
}
int wx_sht_destroy(wx_sht_handle h) { return guarded([&] { delete h; }); }
int wx_sht_analysis(wx_sht_handle h, int n_planes, const void* x_dev, int64_t x_stride, int dtype, double* c_dev, void* stream) {
  return use_remapped(h, "wx_sht_analysis: null sht handle", [&] { h->impl->analysis(n_planes, x_dev, x_stride, dtype, c_dev, (hipStream_t)stream); });
}
int wx_sht_synthesis(wx_sht_handle h, int n_planes, const double* c_dev, void* x_dev, int dtype, void* stream) {
  return use_remapped(h, "wx_sht_synthesis: null sht handle", [&] { h->impl->synthesis(n_planes, c_dev, x_dev, dtype, (hipStream_t)stream); });
}
int wx_sht_vector_analysis(wx_sht_handle h, int n_planes, const void* u_dev, int64_t u_stride, const void* v_dev, int64_t v_stride, int dtype,
                           double* s_dev, double* t_dev, void* stream) {
  return use_remapped(h, "wx_sht_vector_analysis: null sht handle", [&] {
    h->impl->vector_analysis(n_planes, u_dev, u_stride, v_dev, v_stride, dtype, s_dev, t_dev, (hipStream_t)stream);
  });
}
int wx_sht_spectra(wx_sht_handle h, int n_planes, const double* c_dev, double* zonal_dev, double* total_dev, void* stream) {
  return use_remapped(h, "wx_sht_spectra: null sht handle", [&] { h->impl->spectra(n_planes, c_dev, zonal_dev, total_dev, (hipStream_t)stream); });
}
int wx_sht_table(int nlat, int lmax, int mmax, const double* theta_host, const double* w_host, int csphase, int table, int m,
                 double* out_host, int* folds_out) {
  return guarded([&] {
    if (!theta_host || !out_host || (folds_out && !w_host)) throw wx::ConfigError("wx_sht_table: null argument");
    const std::string why = wx::sht_check_table(nlat, lmax, mmax, theta_host, table, m);
    if (!why.empty()) throw wx::ConfigError("wx_sht_table: " + why);
    std::vector<double> col;
    wx::sht_table_column(table, m, lmax, theta_host, nlat, csphase, col);
    std::memcpy(out_host, col.data(), col.size() * sizeof(double));
    if (folds_out) *folds_out = wx::sht_folds(nlat, theta_host, w_host) ? 1 : 0;
  });
}

// ---- inverse vector transform, diffusion and pole filter (csrc/wx_polefilter.h, declared in include/wxengine_polefilter.h) ----------
int wx_sht_vector_synthesis(wx_sht_handle h, int n_planes, const double* s_dev, const double* t_dev, void* u_dev, void* v_dev, int dtype,
                            void* stream) {
  return use_remapped(h, "wx_sht_vector_synthesis: null sht handle", [&] {
    h->impl->vector_synthesis(n_planes, s_dev, t_dev, nullptr, u_dev, v_dev, dtype, (hipStream_t)stream);
  });
}
// the transform first: the filter, which refers to it, is destroyed before it
struct wx_polefilter {
  wx_sht sht;
  std::unique_ptr<wx::PoleFilter> impl;
};
int wx_polefilter_create(int nlat, int nlon, int lmax, int mmax, const double* theta_host, const double* w_host, double radius, int indpol,
                         int cutoff_index, const float* sig_host, int device, wx_polefilter_handle* out) {
  return guarded([&] {
    if (!out || !theta_host || !w_host || !sig_host) throw wx::ConfigError("wx_polefilter_create: null argument");
    std::string why = wx::sht_check_create(nlat, nlon, lmax, mmax, theta_host, w_host, "ortho");
    if (why.empty()) why = wx::polefilter_check_create(nlat, nlon, radius, indpol, cutoff_index, sig_host);
    if (!why.empty()) throw wx::ConfigError("wx_polefilter_create: " + why);
    need_device(device, "wx_polefilter_create");
    std::unique_ptr<wx_polefilter> h(new wx_polefilter);
    h->sht.impl.reset(new wx::Sht(nlat, nlon, lmax, mmax, theta_host, w_host, 0, device));
    h->impl.reset(new wx::PoleFilter(*h->sht.impl, radius, indpol, cutoff_index, sig_host, device));
    *out = h.release();
  });
}
int wx_polefilter_destroy(wx_polefilter_handle h) { return guarded([&] { delete h; }); }
int wx_polefilter_sht(wx_polefilter_handle h, wx_sht_handle* out) {
  return use(h, "wx_polefilter_sht: null polefilter handle", [&] {
    if (!out) throw wx::ConfigError("wx_polefilter_sht: null argument");
    *out = &h->sht;
  });
}
int wx_polefilter_lowpass(wx_polefilter_handle h, int n_planes, const void* x_dev, int64_t x_stride, int dtype, void* out_dev, int64_t out_stride,
                          void* stream) {
  return use_remapped(h, "wx_polefilter_lowpass: null polefilter handle",
                      [&] { h->impl->lowpass(n_planes, x_dev, x_stride, dtype, out_dev, out_stride, (hipStream_t)stream); });
}
int wx_polefilter_scalar(wx_polefilter_handle h, int n_planes, const void* x_dev, int64_t x_stride, int dtype, int substeps, double coef,
                         void* out_dev, int64_t out_stride, void* stream) {
  return use_remapped(h, "wx_polefilter_scalar: null polefilter handle",
                      [&] { h->impl->scalar(n_planes, x_dev, x_stride, dtype, substeps, coef, out_dev, out_stride, (hipStream_t)stream); });
}
int wx_polefilter_vector(wx_polefilter_handle h, int n_planes, const void* u_dev, int64_t u_stride, const void* v_dev, int64_t v_stride, int dtype,
                         int substeps, double coef, void* u_out_dev, int64_t u_out_stride, void* v_out_dev, int64_t v_out_stride, void* stream) {
  return use_remapped(h, "wx_polefilter_vector: null polefilter handle", [&] {
    h->impl->vector(n_planes, u_dev, u_stride, v_dev, v_stride, dtype, substeps, coef, u_out_dev, u_out_stride, v_out_dev, v_out_stride,
                    (hipStream_t)stream);
  });
}
int wx_polefilter_gradient(wx_polefilter_handle h, int n_planes, const double* c_dev, void* gx_dev, void* gy_dev, int dtype, void* stream) {
  return use_remapped(h, "wx_polefilter_gradient: null polefilter handle",
                      [&] { h->impl->gradient(n_planes, c_dev, gx_dev, gy_dev, dtype, (hipStream_t)stream); });
}
int wx_polefilter_workspace(int nlat, int nlon, int lmax, int mmax, int n_planes, int64_t* bytes_out) {
  return guarded([&] {
    if (!bytes_out) throw wx::ConfigError("wx_polefilter_workspace: null argument");
    if (nlat < 1 || nlon < 1 || lmax < 1 || mmax < 1 || nlat > 32768 || nlon > wx::kDftMaxN || lmax > 32768 || mmax > lmax)
      throw wx::ConfigError("wx_polefilter_workspace: nlat, lmax in 1 .. 32768, nlon in 1 .. 4096 and mmax in 1 .. lmax are needed");
    if (n_planes < 1) throw wx::ConfigError("wx_polefilter_workspace: n_planes must be >= 1, got " + std::to_string(n_planes));
    *bytes_out = wx::polefilter_workspace(nlat, nlon, lmax, mmax, n_planes);
  });
}

const char* wx_last_error(void) { return wx::g_last_error.c_str(); }
#ifndef WX_SOURCE_HASH
#define WX_SOURCE_HASH "unhashed"
#endif
// "wxsrc:<hash of csrc/*.h, wx_engine.hip, include/wxengine.h>" is set by miles-credit_amd/build.py; the Python loader compares
// it with the sources next to the library and refuses a stale build
const char* wx_version(void) { return "wxengine 0.2 (gfx950) wxsrc:" WX_SOURCE_HASH; }

}  // extern "C"

// The engine's run-time switches: one field per WX_* environment variable, read once by Options::from_env() when an engine, a Swin
// stage or a FuXi model is created (wx_create, wx_band_plan_create, wx_swin_create, wx_fuxi_create) and kept by it for its lifetime.
// This is the only place in csrc/ that reads the environment; INTEGRATION.md section 4 lists the same variables.
//
// Two kinds.  A flag left unset keeps its default; a flag that is set is true exactly when its value begins with '1'.  A WX_NO_* flag
// names the negation of its field (`NO` below): WX_NO_SPLIT_K=1 turns split_k off.  An integer left unset keeps its default; a set
// one is read with atoll, then clamped where a lower bound is given.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <limits>

namespace wx {

struct Options {
  // ---- GEMM routes (Engine::gemm_route)
  bool use_dma = true;               // LDS-DMA implicit GEMM (the fast path; the only one that emits LayerNorm / GroupNorm partials)
  bool split_k = true;               // split-K plain / skinny forms of the deep-K launches
  bool merge_parity = true;          // the four parity convs of a ConvTranspose k4 s2 p1 as one launch
  int skinny_max = 8;                // skinny split-K: K ranges per tile (0 / 1: off)
  int skinny_steps = 2;              // ... 128-byte K steps per range, at least (>= 1)
  int skinny_min_nk = 16;
  int skinny_tiles = 32;
  int skinny_tiles_band = 128;       // lat-band ranks: the wider tile bound ...
  int skinny_max_band = 4;           // ... whose extra tiles take at most this many K ranges
  int split_bn64 = 1;                // 0: never the 64-column tiles of the badly quantised residual layers
  bool use_stream = true;            // persistent large-tile GEMM (wx_gemm_stream.h) for the LN-folded 1x1 layers of the deep stages
  int stream_min_rows = 4096;        // ... from this many map rows
  bool use_stream_lc = true;         // loader / consumer form of the persistent GEMM (one-tile-per-CU residual layers)
  bool use_gemm8p = true;            // eight-phase 160 x 256 kernel (wx_gemm8p.h) for the deep-K stride-1 k x k convs of the decoder
  int64_t gemm8p_min_rows = 16384;
  bool use_wreg = true;              // weight-stationary GEMM (wx_gemm_wreg.h) for K = 512 layers on mid-sized maps
  int wreg_min_rows = 1024;
  int wreg_max_rows = 4096;
  int gemm_cfg = 0;                  // launch_conv_gemm: 0 automatic, 1 force KB 128 (2 workgroups/CU), 2 force KB 64 (4 workgroups/CU), 3 64-column tiles
  bool fuse_ln = true;               // LayerNorm / GroupNorm statistics from the producing GEMM's epilogue
  int dbg_flags = 0;                 // experiment bits handed to the kernels' `dbg` fields; any bit set also turns the fused forms off

  // ---- CrossEmbed and input packing
  bool use_patch = true;             // stage 0: the LDS-patch CrossEmbed kernel (wx_embed.h)
  bool planar_xin = true;            // ... reading the chunk-planar copy of the packed input (else the pixel-major input)
  bool pack_align = true;            // pack_input: block origin shifted onto the source's 256-byte boundaries
  bool embed_merge = true;           // stages 1-3: the CrossEmbed branches of the same parity as one merged GEMM (launch-bound maps)
  bool embed_ride4 = true;           // stage 0: the k = 4 branch in the patch kernel's spare accumulator rows
  bool embed_split = true;           // small maps: the patch launch split over the channel chunks ...
  int embed_split_ways = 4;          // ... this many ways (>= 2)
  bool embed_tail_split = true;      // big maps: the partly filled last round of tiles as half-chunk workgroups
  bool stat_share = true;            // stages 1-3: every CrossEmbed branch leaves the LayerNorm partials of its channel range

  // ---- attention
  // LN + to_qkv + window attention + to_out + residual as ONE launch (wx_attn_block.h), bf16 engine.  0 never; 1 wherever the kernel
  // exists (C in {128, 256}); 2 (default) only where it measured faster than the fused feed-forward chain on MI355X: C = 128 with
  // 100-token windows on >= 2048 windows (C3 stage 0: 165 + 136 us against 91 + 218 us per sub-block, and 0.5 GB less HBM traffic each)
  // and on maps of <= 32768 tokens, where three launch-bound kernels become one (1-degree model +5 %); slower in between
  int attn_block = 2;
  bool attn_pack2 = true;            // the attention block kernel on 2 x 2 windows, four per fragment (launch-bound maps)
  bool attn_blk_on = true;           // attention sub-blocks on the k-blocked layouts (KBlk::attn)
  int attn_split = 0;                // launch_window_attn split_mode: 0 automatic, 1 never, 2 always (>= 4 key fragments), 3 the [NP][NP] bias table
  bool attn_no_b2 = false;           // launch_window_attn, A/B switch: 100-token bf16 windows without the 2 x 2-block bias order

  // ---- FeedForward (Engine::ff_form)
  bool fuse_ff = true;               // stages with C in {128, 256}: FeedForward as one kernel (wx_ff.h), bf16 engine
  bool fuse_out = true;              // ... with the attention's out-projection in front
  bool fuse_qkv = true;              // ... and the next attention's LayerNorm + to_qkv behind
  int ff_min_wgs = 256;              // fused feed-forward only when it yields at least this many workgroups
  bool ff_small_px64 = true;         // C = 128 plain block on 64-pixel tiles when the map yields < 128 tiles of 128 (1-degree stage 1: 21.5 -> 15.5 us)
  int ff_split_max = 8;              // hidden ranges of the split fused FeedForward (0 / 1: off)
  int ff_split_tiles = 32;           // ... pixel tiles, at most
  bool ff_split_fused = true;        // split-bf16 precision: the C = 128 / 256 FeedForward as one launch (wx_ff_split.h)
  bool ff_split_256 = true;          // ... at C = 256 too
  bool ff_split_pre = true;          // ... with the attention's out-projection in front (its PRE form)
  bool ff_split_post = true;         // ... and the next attention's LayerNorm + to_qkv behind (its POST form)
  int ff_split_tw = 0;               // ... token fragments per wave (1 or 2); 0: by map size

  // ---- GroupNorm, schedule, graphs
  int gn_fold_max_tiles = 16;        // 12 tiles: 13 -> 9 us; 45 tiles: 13 -> 17 us (the serial fold in every workgroup)
  // WX_GRAPH=1 replays each step from a captured hipGraph.  OFF by default, on measurement (MI355X, 1-degree model, 48 steps): eager
  // 557.7 steps/s (1.79 ms/step, ~170 launches), graph replay 484.8 (2.06 ms): on this stack the cost between two dependent kernels is
  // the device-side dispatch boundary (~1.5 us, MI355X_MICROARCH.md "boundary": eager == hipGraph), not host launch time, so a graph
  // removes nothing and adds its replay overhead plus the forcing staging copy.
  int graph_mode = 0;

  // ---- lat-band mode
  // interior / boundary split of the convolutions behind a halo exchange: OFF unless an overlapped transport asks for it (measured on
  // MI355X, profiles/r03_latband_overlap_virtual_ranks_C3_bf16.txt: the two one-row launches cost each rank more than the ~20 us exchange they would hide)
  bool band_split = false;
  bool band_overlap = false;         // wx_band_rccl_init: the exchanges on an engine-owned communication stream (wx_band_comm_stream)
  bool band_stats_ship = true;       // the rows of a long-attention redistribution arrive with their LayerNorm partials

  // ---- Swin stage (wx_swin.h)
  int64_t swin_stream_min_rows = 4096;   // the four Linear layers on the persistent GEMM from this many tokens (bf16, C >= 512) ...
  bool swin_stream = true;               // ... or never

  static constexpr bool NO = true;   // flag(): the variable is the negation of the field
  static void flag(bool& field, const char* name, bool negated = false) {
    if (const char* e = getenv(name)) field = (e[0] == '1') != negated;
  }
  template <typename I>
  static void num(I& field, const char* name, I lo = std::numeric_limits<I>::min()) {
    if (const char* e = getenv(name)) field = std::max(lo, (I)atoll(e));
  }

  static Options from_env() {
    Options o;
    flag(o.use_dma, "WX_NO_DMA", NO);
    flag(o.split_k, "WX_NO_SPLIT_K", NO);
    flag(o.merge_parity, "WX_NO_MERGE_PARITY", NO);
    num(o.skinny_max, "WX_SKINNY_MAX");
    num(o.skinny_steps, "WX_SKINNY_STEPS", 1);
    num(o.skinny_min_nk, "WX_SKINNY_MIN_NK");
    num(o.skinny_tiles, "WX_SKINNY_TILES");
    num(o.skinny_tiles_band, "WX_SKINNY_TILES_BAND");
    num(o.skinny_max_band, "WX_SKINNY_MAX_BAND");
    num(o.split_bn64, "WX_SPLIT_BN64");
    flag(o.use_stream, "WX_NO_STREAM", NO);
    num(o.stream_min_rows, "WX_STREAM_MIN_ROWS");
    flag(o.use_stream_lc, "WX_NO_STREAM_LC", NO);
    flag(o.use_gemm8p, "WX_NO_GEMM8P", NO);
    num(o.gemm8p_min_rows, "WX_GEMM8P_MIN_ROWS");
    flag(o.use_wreg, "WX_NO_WREG", NO);
    num(o.wreg_min_rows, "WX_WREG_MIN_ROWS");
    num(o.wreg_max_rows, "WX_WREG_MAX_ROWS");
    num(o.gemm_cfg, "WX_GEMM_CFG");
    flag(o.fuse_ln, "WX_NO_LNFUSE", NO);
    num(o.dbg_flags, "WX_DBG");
    flag(o.use_patch, "WX_NO_PATCH", NO);
    flag(o.planar_xin, "WX_NO_PLANAR", NO);
    flag(o.pack_align, "WX_NO_PACK_ALIGN", NO);
    flag(o.embed_merge, "WX_NO_EMBED_MERGE", NO);
    flag(o.embed_ride4, "WX_NO_EMBED_RIDE4", NO);
    flag(o.embed_split, "WX_NO_EMBED_SPLIT", NO);
    num(o.embed_split_ways, "WX_EMBED_SPLIT", 2);
    flag(o.embed_tail_split, "WX_NO_EMBED_TAIL_SPLIT", NO);
    flag(o.stat_share, "WX_NO_EMBED_STATS", NO);
    num(o.attn_block, "WX_ATTN_BLOCK");
    flag(o.attn_pack2, "WX_NO_ATTN_PACK2", NO);
    flag(o.attn_blk_on, "WX_NO_ATTN_BLK", NO);
    num(o.attn_split, "WX_ATTN_SPLIT");
    flag(o.attn_no_b2, "WX_ATTN_NO_B2");
    flag(o.fuse_ff, "WX_NO_FFFUSE", NO);
    flag(o.fuse_out, "WX_NO_OUTFUSE", NO);
    flag(o.fuse_qkv, "WX_NO_QKVFUSE", NO);
    num(o.ff_min_wgs, "WX_FF_MIN_WGS");
    flag(o.ff_small_px64, "WX_FF_PX64");
    num(o.ff_split_max, "WX_FF_SPLIT");
    num(o.ff_split_tiles, "WX_FF_SPLIT_TILES");
    flag(o.ff_split_fused, "WX_NO_FF_SPLIT_FUSED", NO);
    flag(o.ff_split_256, "WX_NO_FF_SPLIT_256", NO);
    flag(o.ff_split_pre, "WX_NO_FF_SPLIT_PRE", NO);
    flag(o.ff_split_post, "WX_NO_FF_SPLIT_POST", NO);
    num(o.ff_split_tw, "WX_FF_SPLIT_TW");
    num(o.gn_fold_max_tiles, "WX_GN_FOLD_TILES");
    num(o.graph_mode, "WX_GRAPH");
    flag(o.band_split, "WX_BAND_SPLIT");
    flag(o.band_overlap, "WX_BAND_OVERLAP");
    flag(o.band_stats_ship, "WX_NO_BAND_STATS", NO);
    num(o.swin_stream_min_rows, "WX_SWIN_STREAM_MIN_ROWS");
    flag(o.swin_stream, "WX_SWIN_NO_STREAM", NO);
    return o;
  }
};

}  // namespace wx

// The GEMM / implicit-GEMM conv tile menu: one row per live tile config (GemmArgs::cfg), read by the
// planner (gemm.hip), the launch dispatch (gemm_impl.h, gemm_pp.h) and the gemm_tile_menu() binding.
// Adding or retiring a tile is one row here, plus tests/golden/ and, to be picked, ops/gemm_tuning.json.
// The ids are an external interface (tuning table, gemm_set_override, CASSMANTLE_GEMM_CFG, tools) and
// keep their meaning: a retired index simply has no row.  Retired in round 4 (measured, picked by no
// shape of the SD-1.5 / SDXL census; results in profiles/ and git history): 11, 17-19, 23-25, 28-30.
//
// Families:
//   kTileStatic    gemm_impl.h, 4 waves at 2 blocks per CU by LDS (2 stages) or 8 waves at 1 block per
//                  CU (3-stage ring); every A-operand mode, bf16 or fp32 out
//   kTilePingPong  gemm_pp.h, 8 waves, 1 block per CU, 2 LDS buffers, counted vmcnt; buffer-resource
//                  modes, bf16 out
//   kTileDeep      gemm_impl.h with a 3-5 stage LDS ring, one block per CU, optionally with DMA-only
//                  producer waves beside the MFMA waves; buffer-resource modes, bf16 out
//   kTileAreg      gemm_areg.hip, A-in-registers short-K kernel (K = 320 / 640, W streamed in chunks);
//                  picks its own tiles, so the row carries no geometry
#pragma once
#include <utility>

enum GemmTileFamily { kTileStatic, kTilePingPong, kTileDeep, kTileAreg };

struct GemmTile {
  int id;
  GemmTileFamily family;
  int BM, BN, WM, WN;      // block tile, WM x WN MFMA waves
  int stages, producers;   // LDS ring depth, DMA-only producer waves
  int GWM, GWN;            // wave layout of the gated (GEGLU / SwiGLU) instantiation; 0 x 0: there is none
  bool model;              // the cost model may pick it; false: only from the tuning table or when forced
  float eff;               // cost model: relative per-k-tile efficiency
  int slots;               // cost model: resident blocks on the chip
  constexpr bool gated() const { return GWM != 0; }
};

// slots: 128x64 needs 48 KiB of LDS per block, so 3 blocks fit a CU (768 slots); with 512 the model
// undercounted it and missed the measured best on the level-2..4 plain GEMMs
// (profiles/r1_gemm_plan_sweep.jsonl: 14.5 vs 17.8 us at 8192x640x640)
// clang-format off
constexpr GemmTile kGemmTiles[] = {
    // id family         BM   BN  WMxWN st np  gated  model eff   slots
    {  0, kTileStatic,   128, 128, 2, 2, 2, 0, 2, 2, true,  1.00f, 512},  // the default tile
    {  1, kTileStatic,   128, 160, 2, 2, 2, 0, 0, 0, true,  1.02f, 512},  // wave 80x64
    {  2, kTileStatic,   256,  64, 4, 1, 2, 0, 0, 0, true,  0.95f, 512},  // N = 64 (mod 128)
    {  3, kTileStatic,   128,  64, 2, 2, 2, 0, 0, 0, true,  0.80f, 768},
    {  4, kTileStatic,   256,  16, 4, 1, 2, 0, 0, 0, true,  0.25f, 512},  // N <= 16 (3/4-channel conv_out), and only those
    {  5, kTileStatic,   256, 160, 4, 2, 3, 0, 0, 0, true,  1.02f, 256},  // wave 64x80; 8-wave: CASSMANTLE_GEMM_8WAVE
    {  6, kTileStatic,   256, 128, 4, 2, 3, 0, 4, 2, true,  1.00f, 256},  // 8-wave
    {  7, kTilePingPong, 256, 256, 4, 2, 2, 0, 0, 0, true,  1.60f, 256},  // the ping-pong default (gated would spill: 256 VGPRs)
    {  8, kTilePingPong, 256, 160, 4, 2, 2, 0, 8, 1, true,  1.55f, 256},  // gated: waves stacked along M, 80 outputs per block
    {  9, kTilePingPong, 256, 128, 4, 2, 2, 0, 4, 2, true,  1.45f, 256},  // the ping-pong gated default
    { 10, kTilePingPong, 128, 256, 2, 4, 2, 0, 0, 0, true,  1.45f, 256},
    { 12, kTileDeep,     128, 128, 2, 2, 4, 0, 2, 2, false, 1.00f, 256},  // the deep-ring gated tile
    { 13, kTileDeep,     128,  64, 2, 2, 5, 0, 0, 0, false, 1.00f, 256},
    { 14, kTileDeep,     128, 160, 4, 2, 4, 0, 0, 0, false, 1.00f, 256},
    { 15, kTileAreg,       0,   0, 0, 0, 0, 0, 0, 0, false, 1.00f, 256},  // also gated, in its own kernel
    { 16, kTileDeep,     128,  80, 4, 1, 4, 0, 0, 0, false, 1.00f, 256},  // wave 32x80: M 2048 x N 1280 is 256 tiles, one per CU
    { 20, kTilePingPong, 128, 160, 4, 2, 2, 0, 0, 0, false, 1.00f, 256},  // wave 32x80: twice the blocks of 256x160 without split-K
    { 21, kTilePingPong, 128, 128, 4, 2, 2, 0, 0, 0, false, 1.00f, 512},  // wave 32x64, 64 KiB LDS: 2 blocks per CU
    { 22, kTilePingPong, 128,  64, 4, 2, 2, 0, 0, 0, false, 1.00f, 768},  // 48 KiB LDS
    // 26 / 27: the small-grid tiles with twice the waves issuing LDS-DMA.  A CU's LDS-DMA fill rate
    // is set by the number of waves issuing it, not by the bytes in flight (4 waves: 22 B/cycle on
    // the GEMM row pattern at any ring depth, 8 waves: 37; profiles/r3_lds_fill_probe.jsonl)
    { 26, kTileDeep,     128,  80, 8, 1, 4, 0, 0, 0, false, 1.00f, 256},  // wave 16x80
    { 27, kTileDeep,     128,  64, 4, 2, 3, 0, 0, 0, false, 1.00f, 256},
    // 31-33: warp-specialised, 8 MFMA waves + 8 DMA-only producer waves (1024 threads).  (Removed in
    // round 4, bench-neutral: 256x128 / 128x256 / 128x128 / 128x160 8x1 producer tiles and 31-33 with
    // the MFMA waves staging too, profiles/r4_producer_waves_ab.txt; 6-stage rings of 31 / 32: no
    // faster with weights from HBM on every call, profiles/r4_cold_weight_probe.jsonl)
    { 31, kTileDeep,     128,  80, 8, 1, 4, 8, 0, 0, false, 1.00f, 256},
    { 32, kTileDeep,     128,  64, 4, 2, 4, 8, 0, 0, false, 1.00f, 256},
    { 33, kTileDeep,     128, 160, 4, 2, 4, 8, 0, 0, false, 1.00f, 256},
};
// clang-format on
constexpr int kNumGemmTiles = sizeof(kGemmTiles) / sizeof(kGemmTiles[0]);
using GemmTileRows = std::make_integer_sequence<int, kNumGemmTiles>;   // for the launchers' fold over the rows

// row of a config; null: not live (retired or unknown index)
constexpr const GemmTile* gemm_tile(int cfg) {
  for (const GemmTile& t : kGemmTiles)
    if (t.id == cfg) return &t;
  return nullptr;
}

// where a call lands that names a config its family has no instantiation for: an unknown cfg at
// launch (static tiles: also a deep-ring cfg in a mode without deep rings), a forced gated call
constexpr int gemm_default_tile(GemmTileFamily f, bool gated) {
  return f == kTilePingPong ? (gated ? 9 : 7) : (f == kTileDeep && gated) ? 12 : 0;
}
constexpr int kGemmAregTile = 15;

// has row t an instantiation?  In the gemm_pp.h units (pingpong): the ping-pong rows; in the
// gemm_impl.h units: the static rows in every A-operand mode, the deep rings in the buffer-resource
// modes (buf) with bf16 out; a gated call takes the rows with a gated wave layout.  The launchers
// instantiate by this predicate and the route (gemm.hip) names the tile that runs by it
constexpr bool gemm_tile_built(const GemmTile& t, bool pingpong, bool gated, bool out_f32, bool buf) {
  const bool here = pingpong ? t.family == kTilePingPong
                             : t.family == kTileStatic || (t.family == kTileDeep && buf && !out_f32);
  return here && (!gated || t.gated());
}
// the tile that runs when a call names cfg: cfg itself, or its units' default when they hold no such instantiation
constexpr int gemm_tile_that_runs(int cfg, bool pingpong, bool gated, bool out_f32, bool buf) {
  const GemmTile* t = gemm_tile(cfg);
  return t != nullptr && gemm_tile_built(*t, pingpong, gated, out_f32, buf)
             ? cfg : gemm_default_tile(pingpong ? kTilePingPong : kTileStatic, gated);
}

static_assert(gemm_tile(gemm_default_tile(kTileStatic, true))->gated() && gemm_tile(gemm_default_tile(kTilePingPong, true))->gated() &&
                  gemm_tile(gemm_default_tile(kTileDeep, true))->gated() && gemm_tile(gemm_default_tile(kTilePingPong, false)) != nullptr &&
                  gemm_tile(kGemmAregTile)->family == kTileAreg,
              "gemm_tiles.h: the family defaults are live rows");

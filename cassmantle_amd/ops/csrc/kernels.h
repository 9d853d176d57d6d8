// Host-visible launcher declarations of the gfx950 kernel library.  Kernel translation units
// (*.hip) are compiled without torch headers; bindings.cpp converts tensors to these structs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct GemmArgs {
  const uint16_t* A = nullptr;          // activations [batch][M][lda] or NHWC conv input
  const uint16_t* W = nullptr;          // weights [batch][Nw][K], K contiguous
  const uint16_t* bias = nullptr;       // [Nw] (geglu: [2N])
  const uint16_t* residual = nullptr;   // [M][ldc]
  const uint16_t* chan_bias = nullptr;  // [B][N] per-image bias (ResNet time embedding)
  int ldcb = 0;                         // chan_bias row stride (0 -> N): slices of one batched GEMM
  void* C = nullptr;                    // [batch][M][ldc] bf16 or f32
  int M = 0, N = 0, K = 0, Nw = 0;
  int lda = 0, ldc = 0, ldw = 0;      // ldw = W row stride (0 -> K)
  long long sA = 0, sW = 0, sC = 0;
  int batch = 1;
  float alpha = 1.f;
  int act = 0;
  int out_f32 = 0;
  int split = 1;                       // split-K slices (gemm_plan)
  int cfg = 0;                         // tile config index (gemm_plan)
  int raster = 0;                      // tile raster group (gemm_impl.h tile_of; 0 = compiled default)
  // implicit-GEMM convolution (conv != 0)
  int conv = 0, IH = 0, IW = 0, Cin = 0, Ho = 0, Wo = 0, stride = 1, pad = 0, ksize = 1, upsample = 0;
  // parity-upsample conv (nearest-2x upsample + 3x3 conv as four 2x2 convs on the low-res input,
  // 4/9 of the MACs): grid z = parity class 2a+b, W = [4][Cout][2][2][Cin] folded weights
  // (sW = one class), Ho/Wo = low-res size, output written at pixel (2i+a, 2j+b)
  int parity = 0;
  // fused RMSNorm of A's rows (GEMV path only): A <- A * gamma / rms(A)
  const uint16_t* rms_gamma = nullptr;
  float rms_eps = 0.f;
  // second A source (1x1 conv / linear over a channel concatenation [A | A2]): k < ka reads A
  // (row stride lda), k >= ka reads A2 (row stride lda2); ka % 64 == 0 (whole k-tiles)
  const uint16_t* A2 = nullptr;
  int lda2 = 0, ka = 0;
  // LayerNorm folded into this GEMM (A = raw rows x, W = W * gamma, bias = bias + W . beta):
  // out[m][n] = rstd[m] * (acc - mean[m] * wsum[n]) + bias[n] ...; ln_rows [M] (mean, rstd)
  // float2, ln_wsum [Nw] fp32 column sums of the folded W
  const float* ln_rows = nullptr;
  const float* ln_wsum = nullptr;
  // ln_wsum set, ln_rows null, ln_eps > 0: the row statistics are computed INSIDE the kernel from
  // the register-resident A rows (A-in-registers short-K GEMM, gemm_areg.hip, only)
  float ln_eps = 0.f;
  // folded LayerNorm whose row statistics a PRODUCER epilogue accumulated (row_stats below):
  // [M][2] int64 fixed-point (sum, sum of squares) over the K columns; mean / rstd (with ln_eps)
  // are derived in this GEMM's epilogue -- no row-statistics pass
  const long long* ln_rows_fx = nullptr;
  // row statistics of THIS GEMM's stored output (after bias / residual), for a LayerNorm-folded
  // consumer: atomically accumulated [M][2] int64 fixed-point (sum, sum of squares) over the N
  // columns (zeroed by the caller); LDS-staged bf16 epilogue only (no split-K, no GroupNorm stats)
  long long* row_stats = nullptr;
  // GroupNorm (no SiLU) of the A rows folded into the A-in-registers kernel (gemm_areg.hip only):
  // A = the raw input x, gn_stats = its producer-accumulated per-(image, channel) int64 (sum,
  // sum of squares) [M / gn_hw][K][2]; the kernel folds them to per-group mean / rstd and applies
  // x * gamma * rstd + (beta - mean * gamma * rstd) to the register-resident fragments
  const long long* gn_stats = nullptr;
  const uint16_t* gn_gamma = nullptr;
  const uint16_t* gn_beta = nullptr;
  int gn_groups = 0, gn_hw = 0;
  float gn_eps = 0.f;
  // GroupNorm statistics of the output: atomically accumulated per-(image, column) sum and
  // sum-of-squares [M / stats_hw][N][2] int64 fixed point (common.h; zeroed by the caller);
  // stats_hw = rows per image
  long long* stats = nullptr;
  int stats_hw = 0;
  // e4m3 K/V emission for the fp8 attention kernel (SDXL self-attention): output columns
  // [kv8_col0, kv8_col0 + 128 kv8_hk) are the K then V heads (64 wide) of images of kv8_ntok
  // tokens (kv8_ntok % 64 == 0); they are stored as K8 [B][Hk][ntok][64] and V8t [B][Hk][64][ntok]
  // (slot-permuted key blocks) in kv8 instead of bf16 in C (attention.hip's packed image)
  uint8_t* kv8 = nullptr;
  int kv8_col0 = 0, kv8_ntok = 0, kv8_hk = 0;
};
#define GEMM_MAX_SPLIT 16
struct GemmPlan { int cfg; int split; };
GemmPlan gemm_plan(const GemmArgs& p);
// force a tile config (-1: cost model) and split-K factor (0: cost model) for every later plan
void gemm_set_override(int cfg, int split);
// measured tuning table: shape key (gemm_key) -> plan; key recording for the autotuner
#include <string>
std::string gemm_key(const GemmArgs& p);
void gemm_tune_set(const std::string& key, int cfg, int split);
void gemm_tune_clear();
int gemm_tune_size();
void gemm_record_keys(bool on);
std::string gemm_last_key();
void gemm_last_plan(int* cfg, int* split);
// Which kernel a call ends up in, and the passes around it: decided in one place, gemm_route (pure
// host code: no launch, no allocation; tests/golden/gemm_routes.txt).  The caller (bindings.cpp
// run_gemm) refuses, runs the pre-pass, allocates ws_floats, launches, runs the post-pass.
enum GemmKernel { kGemmGemv, kGemmSimt, kGemmAreg, kGemmPingPong, kGemmTiled };   // lm.hip, gemm.hip, gemm_areg.hip, gemm_pp.h, gemm_impl.h
// the A-operand mode = the gemm_c*.hip unit (ping-pong: gemm_pp_c0 / _c2 as c0_buf / c2_buf; the
// kernels without units: c1 for a SIMT conv, else c0)
enum GemmAMode { kA_c0, kA_c0_buf, kA_c1, kA_c2, kA_c2_buf, kA_c3 };
// kPreRowStats: launch_row_stats(A) -> rows fp32 [M][2] (the folded LayerNorm's statistics where the
// kernel cannot compute them); kPreGnApply: launch_group_norm_cs(A) -> xn bf16 [M][K] (the GroupNorm
// fold where the A-in-registers kernel does not take the call).  gemm_apply_pre rewrites the arguments
enum GemmPre { kPreNone, kPreRowStats, kPreGnApply };
struct GemmRoute {
  GemmKernel kernel; GemmAMode mode;
  int cfg, split;          // cfg: the tile that RUNS (the planner's, unless its units hold no such instantiation; -1: no tile)
  GemmPre pre;
  bool post_stats;         // the kernel does not fuse p.stats: launch_channel_stats over C afterwards, p.stats cleared
  long long ws_floats;     // split-K slabs, 0 if none
  const char* refuse;      // non-null: no kernel computes this call; the text of the error
};
GemmRoute gemm_route(const GemmArgs& p);
void gemm_apply_pre(GemmArgs& p, GemmPre pre, const void* tmp);   // tmp: the pre-pass's output
GemmRoute gemm_last_route();                                      // of the calling thread, as gemm_last_plan
inline const char* gemm_kernel_name(GemmKernel k) { static const char* const n[] = {"gemv", "simt", "areg", "pingpong", "tiles"}; return n[k]; }
inline const char* gemm_amode_name(GemmAMode m) { static const char* const n[] = {"c0", "c0_buf", "c1", "c2", "c2_buf", "c3"}; return n[m]; }
inline const char* gemm_pre_name(GemmPre p) { static const char* const n[] = {"none", "row_stats", "gn_apply"}; return n[p]; }
// launches route.kernel in route.mode with route.cfg / route.split; ws: route.ws_floats floats (else may be null)
void launch_gemm(const GemmArgs& p, const GemmRoute& route, float* ws, hipStream_t s);

struct AttnArgs {
  const uint16_t* q; const uint16_t* k; const uint16_t* v; uint16_t* o;
  long long q_sb, q_sn, q_sh;     // element strides: batch, token, head
  long long k_sb, k_sn, k_sh;
  long long v_sb, v_sn, v_sh;
  long long o_sb, o_sn, o_sh;
  int B, H, Nq, Nk, d;
  float scale;
  int causal;
  const int* kv_lens;             // [B] or null
  int group = 1;                  // query heads per K/V head (GQA)
};
void launch_attention(const AttnArgs& a, hipStream_t s);
// the attention kernel the calling thread launched last (as gemm_last_plan): the family, the
// template widths of QK^T and P.V (fp8 / d512: the head dim) and the waves per block.  Written by
// every attention launcher, so it is never stale
enum AttnFamily { kAttnFwd, kAttnA16, kAttnFp8, kAttnD512 };
void attention_note_kernel(AttnFamily family, int dqk, int dout, int nw);
void attention_last_kernel(int* family, int* dqk, int* dout, int* nw);
// head dim 512 (VAE mid-block): flash kernel; ws = attention_d512_workspace bytes (key-split
// partials for short grids, 0 otherwise)
long long attention_d512_workspace(const AttnArgs& a);
void launch_attention_d512(const AttnArgs& a, float* ws, hipStream_t s);
// fp8 (OCP e4m3) attention for head dim 64: ws = attention_fp8_workspace bytes (K8 + V8t)
long long attention_fp8_workspace(const AttnArgs& a, int Hk);
// packed = true: ws already holds K8/V8t of these K/V (attention_fp8_pack once per text
// context for cross-attention), only the attention kernel runs
void set_fp8_attn_variant(int v);
void set_attn_d40_variant(int v);
void launch_attention_fp8(const AttnArgs& a, int Hk, uint8_t* ws, hipStream_t s, bool packed = false);
void launch_attention_fp8_pack(const AttnArgs& a, int Hk, uint8_t* ws, hipStream_t s);

// norms
void launch_group_norm(const uint16_t* x, const uint16_t* gamma, const uint16_t* beta, uint16_t* y,
                       float* ws, int B, long long S, int C, int G, float eps, int silu, hipStream_t s);
// GroupNorm from producer-accumulated per-channel stats ([B][Ca][2] for channels < Ca, then
// [B][C-Ca][2] from stats_b when the input is a channel concatenation); no statistics pass.
// x2 != null: the input is the concatenation [x (Ca channels) | x2 (C - Ca channels)] read from
// the two tensors (the concatenated tensor is never materialised)
void launch_group_norm_cs(const uint16_t* x, const uint16_t* x2, const long long* stats_a, int Ca, const long long* stats_b,
                          const uint16_t* gamma, const uint16_t* beta, uint16_t* y, int B, long long S, int C,
                          int G, float eps, int silu, hipStream_t s);
// per-channel stats of an NHWC tensor into zeroed int64 fixed-point [B][C][2] (for producers
// without a fused path)
void launch_channel_stats(const uint16_t* x, long long* stats, int B, long long S, int C, hipStream_t s);
long long group_norm_workspace(int B, long long S, int C);
// The launch geometry of the three launchers above for x [B][S][C], computed in one place (as
// gemm_plan for the GEMMs) so tests can assert which branches of the kernels a shape reaches.
// Two-pass path (launch_group_norm, launch_channel_stats): VPT 8-channel vectors per thread,
// T vector lanes x R row lanes, statistics chunks of rpc rows, apply blocks of apply_rpb rows.
// Statistics-fed path (launch_group_norm_cs): its own VPT / T / R, U rows per thread in flight,
// blocks of cs_rpb rows.  launch_group_norm and launch_channel_stats instantiate VPT 1 and 2
// only (C <= GN_MAX_C); launch_group_norm_cs also VPT 4.
constexpr int GN_MAX_C = 4096;
struct GnLaunchGeom {
  int vpt, T, R, chunks;
  long long rpc, apply_rpb, apply_nb;
  int cs_vpt, cs_T, cs_R, cs_U;
  long long cs_rpb, cs_nb;
};
GnLaunchGeom group_norm_geometry(int B, long long S, int C);
void launch_layer_norm(const uint16_t* x, const uint16_t* gamma, const uint16_t* beta, uint16_t* y,
                       long long rows, int D, float eps, hipStream_t s);
// per-row (mean, rstd) float2 of [rows][D] (LayerNorm statistics for a folded-LN GEMM)
// A-in-registers short-K GEMM (gemm_areg.hip): shapes it takes, and the launch
bool gemm_areg_ok(const GemmArgs& p);
void launch_gemm_areg(const GemmArgs& p, hipStream_t s);
void launch_row_stats(const uint16_t* x, float* stats, long long rows, int D, float eps, hipStream_t s);
// fused encoder input layer: y[r] = LN(word[ids[r]] + pos[r % seq] + add) (bf16, D % 8 == 0)
void launch_embed_layer_norm(const uint16_t* word, const long long* ids, const uint16_t* pos, int seq,
                             const uint16_t* add, const uint16_t* gamma, const uint16_t* beta, uint16_t* y,
                             long long rows, int D, float eps, hipStream_t s);
void launch_rms_norm(const uint16_t* x, const uint16_t* gamma, uint16_t* y, long long rows, int D, float eps,
                     hipStream_t s);

// decode path (lm.hip)
constexpr bool gemv_rows(int M) { return M <= 8; }    // skinny: the row counts the GEMV is instantiated for
bool gemv_ok(const GemmArgs& p);                      // the calls the GEMV takes (gemm.hip, with the other routes)
bool launch_gemv(const GemmArgs& p, hipStream_t s);   // false -> !gemv_ok(p)
struct RopeArgs {
  const uint16_t* qkv; long long ld;   // [B*T][ld], heads [q | k | v] x d
  const int* pos0;                     // [B] first position of this chunk (null -> 0)
  uint16_t* q_out;                     // [B][T][H][d]
  uint16_t* k_cache; uint16_t* v_cache;   // [B][L][Hk][d]
  int B, T, H, Hk, d, L;
  float log2_theta;
};
void launch_rope_kv(const RopeArgs& a, hipStream_t s);
struct DecodeArgs {
  const uint16_t* q; long long q_sb;   // [B][H][d] (batch stride q_sb)
  const uint16_t* k_cache; const uint16_t* v_cache;   // [B][L][Hk][d]
  const int* lens;                     // [B] valid keys (device)
  uint16_t* o; long long o_sb;         // [B][H][d]
  float* ws;                           // split partials [B*H][ns][d+2]
  int* tickets;                        // [B*Hk] zeroed arrival counters (re-armed by the kernel)
  int B, H, Hk, d, L;
  float scale;
};
int decode_splits(int B, int Hk, int L);
void launch_decode_attention(const DecodeArgs& a, int ns, hipStream_t s);
// weight-only fp8 decode path (lm_fp8.hip; weight contract in its header comment)
struct GemvFp8Args {
  const uint16_t* A = nullptr; int lda = 0;   // raw bf16 activations [M][lda], lda % 8 == 0
  const uint8_t* Q = nullptr;                 // e4m3 codes [Nw][K], K % 16 == 0, 16-byte aligned
  const float* scale = nullptr;               // [Nw]
  const uint16_t* bias = nullptr;             // [Nw] or null
  const uint16_t* residual = nullptr; int ldr = 0;   // [M][ldr] or null
  void* C = nullptr; int ldc = 0;             // [M][ldc] bf16 or fp32
  int M = 0, N = 0, K = 0;                    // N outputs (gated: Nw = 2N, value row n and gate row N + n)
  int act = 0, out_f32 = 0;
  int rms = 0; float rms_eps = 0.f;           // rms: rows scaled by rsqrt(mean x^2 + rms_eps)
};
bool launch_gemv_fp8(const GemvFp8Args& p, hipStream_t s);   // false -> shape not handled (M > 8, K % 16, lda % 8)
// q, scale of w [rows][K] bf16 times gamma [K] bf16 (null: no gain); K % 16 == 0
void launch_quant_rows_fp8(const uint16_t* w, const uint16_t* gamma, uint8_t* q, float* scale, long long rows, int K,
                           hipStream_t s);
// out [rows][K] bf16 = bf16(e4m3(q) * scale[row])
void launch_dequant_rows_fp8(const uint8_t* q, const float* scale, uint16_t* out, long long rows, int K,
                             hipStream_t s);
// decode-step sampler (lm_sample.hip): top-k of logits / T (+ EOS bias of the row's step) + Gumbel-max,
// then token / position / length / step counter updated on the device; one workgroup per row, every
// row with its own step counter.  The noise is either row `step` of a table (batch 1, seeds null) or
// drawn in the kernel from the row's seed (the GUMBEL CONTRACT of philox_gumbel.h, noise null)
struct LmSampleArgs {
  const void* logits; long long ld;    // [B][V] bf16 / fp32, row stride in elements
  const float* noise;                  // [steps][1][V] table, or null
  const long long* seeds;              // [B] 64-bit sequence seeds, or null
  const float* eos_bias;               // [steps]
  long long* step;                     // [B] per-row step counters
  long long* out;                      // [steps][B]
  long long* tok;                      // [B]
  int* pos; int* lens;                 // [B]
  int B, V, k, eos, steps;
  float temp;
};
void launch_lm_sample(const LmSampleArgs& a, int logits_f32, hipStream_t s);
// out[b][j] = g(seeds[b], step, ids[j]) fp32
void launch_lm_gumbel(const long long* seeds, unsigned step, const long long* ids, int n, int B, float* out,
                      hipStream_t s);

// scorer
void launch_gather_cosine(const void* table, int table_f32, int D, const int* ia, const int* ib,
                          float* out, int n, hipStream_t s);
void launch_pair_cosine(const float* a, const float* b, int D, float* out, int n, hipStream_t s);
void launch_cosine_gemv(const void* table, int table_f32, int V, int D, const void* vec, int vec_f32,
                        float* out, hipStream_t s);
int cosine_topk_workspace(int V, int k);
void launch_cosine_topk(const void* table, int table_f32, int V, int D, const void* vec, int vec_f32, int k,
                        unsigned long long* ws, float* vals, long long* idx, hipStream_t s);
void launch_mean_pool_l2(const uint16_t* h, const int* lens, float* out, int B, int T, int D, hipStream_t s);

// image / diffusion glue
void launch_gaussian_blur(const void* img, int u8, int H, int W, int C, const float* w, int R,
                          float* tmp, void* out, hipStream_t s);
void launch_to_uint8(const uint16_t* x, uint8_t* out, long long n, hipStream_t s);
void launch_timestep_embedding(const float* t, void* out, int B, int dim, int flip, float shift, int out_bf16,
                               hipStream_t s);
void launch_gather_add(const uint16_t* table, const int* ids, const uint16_t* pos, int seq, int D, long long rows,
                       uint16_t* out, hipStream_t s);
void launch_concat2(const uint16_t* a, int Da, const void* b, int Db, int b_f32, long long rows, uint16_t* out,
                    hipStream_t s);
void launch_silu_bf16(uint16_t* x, long long n, hipStream_t s);
void launch_latent_init(const float* x0, float c_in0, float* x, float* xs, float* hist, int nhist, uint16_t* unet_in,
                        long long n, int cfg, int cin, int cstride, hipStream_t s);
void launch_copy(const void* src, void* dst, long long bytes, hipStream_t s);
void launch_finalize_latents(const float* x, uint16_t* z, long long n, uint8_t* finite, hipStream_t s);
// CFG combine + scheduler update + next UNet input (channel-padded to cstride); the optional
// tables' rows for step+1 (time conditioning) are copied into buf0/buf1 by extra blocks.
// ``seeds`` (nullptr: a deterministic plan, row column 15 ignored): one 64-bit noise seed per
// image, ``images`` of them; then cin == 4 and 16-byte aligned latents (philox_normal.h)
void launch_latent_step(const uint16_t* eps, float* x, float* hist, float* xs, const float* coef, const int* step,
                        uint16_t* unet_in, long long n, int cfg, int cin, int cstride, const void* tab0, void* buf0,
                        long long row_bytes0, const void* tab1, void* buf1, long long row_bytes1, int rows,
                        const void* seeds, int images, hipStream_t s);
void launch_advance_step(int* step, hipStream_t s);
void launch_zero(void* p, long long bytes, hipStream_t s);
void launch_prefetch(const void* p, long long bytes, int blocks, void* sink, hipStream_t s);
void launch_softmax_rows(const float* S, uint16_t* P, int rows, int cols, int Nq, int causal,
                         const int* kv_lens, hipStream_t s);

// batched baseline JPEG encoder (jpeg.hip; byte contract in its header comment)
struct JpegArgs {
  const uint8_t* img = nullptr;      // [B][H][W][3]
  int B = 0, H = 0, W = 0;
  int nb = 0;                        // blocks per MCU: 6 (4:2:0, 16x16 MCU) or 3 (4:4:4, 8x8 MCU)
  int mx = 0, my = 0;                // MCUs per row / MCU rows
  int restart = 0, nint = 0;         // MCUs per restart interval, intervals per image
  const int* qtab = nullptr;         // [2][64] luma, chroma quantisation tables, natural order
  const int* huff = nullptr;         // [2*16 + 2*256] (length << 16) | code: DC luma, DC chroma, AC luma, AC chroma
  int16_t* coef = nullptr;           // [B][mx*my][nb][64] quantised zig-zag coefficients
  uint32_t* lens = nullptr;          // [B][nint] bytes per interval (stuffing, padding, RSTn / EOI included)
  uint32_t* offs = nullptr;          // [B][nint] exclusive scan of lens per image
  uint32_t* base = nullptr;          // [B + 1] byte offset of every image in the payload
  const uint8_t* header = nullptr;   // SOI .. SOS, the same for every image of the batch
  int hdr_len = 0;
  // 1: the libjpeg forward contract (jpeg_fdct_lj.h): its transform kernel, and with optimised
  // tables a DHT segment per table in every image's header
  int lj = 0;
  uint8_t* out = nullptr;            // payload (launch_jpeg_write)
  // launch_jpeg_reconstruct (decode contract in jpeg.hip's header comment)
  uint8_t* planes = nullptr;         // scratch: Y [B][yh][yw], Cb, Cr [B][8 my][8 mx]; yh x yw = 16 my x 16 mx (4:2:0) or 8 my x 8 mx
  uint8_t* dec = nullptr;            // [B][H][W][3] the pixels a libjpeg decoder gives for coef
  // optimised Huffman tables (section of that name in jpeg.hip's header comment; jpeg_huff_opt.h).
  // ihuff == nullptr: the standard tables, and none of these is read.  Otherwise header holds the
  // bytes before the DHT segment (hdr_split of them) followed by those behind it, B <= 65535.
  uint32_t* freq = nullptr;          // [B][2*16 + 2*256] symbol counts, the layout of huff
  uint32_t* ihuff = nullptr;         // [B][2*16 + 2*256] every image's own (length << 16) | code words
  uint8_t* hdrs = nullptr;           // [B][hdr_cap] every image's header
  uint32_t* hdr_lens = nullptr;      // [B] its length (0: a table was refused); in work, behind base
  int hdr_cap = 0, hdr_split = 0;
};
// transform + interval byte counts + scans: fills coef, lens, offs, base
void launch_jpeg_count(const JpegArgs& a, hipStream_t s);
// entropy-coded data at the final offsets + headers: fills out[0 .. base[B])
void launch_jpeg_write(const JpegArgs& a, hipStream_t s);
// block-parallel entropy coder (block-parallel entropy coder section of jpeg.hip's header comment;
// jpeg_entropy_blk.h).  With it a.restart = MCUs per interval (all of them without DRI), never 0.
struct JpegBlkArgs {
  uint32_t* bits = nullptr;          // [B][mx*my][nb] bit length of every block, then its bit offset in its interval
  uint32_t* ubits = nullptr;         // [B][nint] bits of every interval's unstuffed string
  uint32_t* scratch = nullptr;       // [B][nint][stride] the unstuffed strings, MSB first in 32-bit words
  uint32_t stride = 0;               // words per interval = ceil(min(restart, mcus) * nb * JPEG_BLK_MAX_BITS / 32)
  uint32_t* err = nullptr;           // one word, raised by a refused scratch index (behind base: read with it)
  uint32_t out_size = 0;             // launch_jpeg_write_blocks: payload bytes = base[B]; out[out_size] is raised
                                     // by a refused payload index
};
// transform + bits per block + scan per interval + pack + 0xFF count per piece + the scans of
// launch_jpeg_count: fills coef, bits, ubits, scratch, err, lens, offs, base
void launch_jpeg_count_blocks(const JpegArgs& a, const JpegBlkArgs& k, hipStream_t s);
// the stuffed bytes at the final offsets + markers + headers: fills out[0 .. out_size], out[out_size] = error byte
void launch_jpeg_write_blocks(const JpegArgs& a, const JpegBlkArgs& k, hipStream_t s);
// inverse DCT of coef into planes, then upsampling + colour into dec (reads B, H, W, nb, mx, my,
// qtab, coef only)
void launch_jpeg_reconstruct(const JpegArgs& a, hipStream_t s);
// entropy decode (entropy decode contract in jpeg.hip's header comment; jpeg_entropy_dec.h)
struct JpegDecodeIn {
  const uint8_t* bytes = nullptr;        // the entropy-coded data of the batch
  uint32_t nbytes = 0;                   // every interval is checked to lie in bytes[0 .. nbytes)
  const uint32_t* intervals = nullptr;   // [B][nint] (offset into bytes, length), markers excluded
  const uint32_t* tables = nullptr;      // [JPEG_DEC_WORDS] zig-zag quantisation tables | four decode tables
  unsigned long long* status = nullptr;  // 0: every interval OK, else (0xffffffff - gid) << 32 | status of the lowest gid
  long long zero_bytes = 0;              // from a.coef: the coefficients and the status word behind them
};
// zeroes coef and status, then one lane per interval: fills coef (reads B, nb, mx, my, restart,
// nint, coef of a; restart = MCUs per interval, all of them without DRI)
void launch_jpeg_entropy_decode(const JpegArgs& a, const JpegDecodeIn& d, hipStream_t s);
// chunked entropy decode (chunked entropy decode contract in jpeg.hip's header comment; jpeg_entropy_sync.h)
struct JpegSyncIn {
  const uint32_t* lane0 = nullptr;       // [B][nint] the interval's first lane within its group
  const uint32_t* groups = nullptr;      // [ngroups][2] (first interval gid, intervals): one image, at most 1024 chunks
  int ngroups = 0;
  uint32_t cb = 0;                       // chunk bytes, a multiple of 16
  uint32_t* words = nullptr;             // [4] flag, rounds, blocks completed, unused: behind the status word, zeroed with it
};
// zeroes coef, status and words, then sync (one lane per chunk, `threads` a multiple of 64 that
// covers the largest group), DC prefix and check: fills coef unless words[0] is raised or
// words[2] is below the block count
void launch_jpeg_entropy_decode_chunked(const JpegArgs& a, const JpegDecodeIn& d, const JpegSyncIn& y, int threads,
                                        hipStream_t s);

// PIL's GaussianBlur, bit for bit (blur_pil.hip; blur contract in its header comment)
int blur_pil_max_tiled_radius();
// table int32 [n][4] = (r, ww, fw, slot) on the device, every r <= rmax <= blur_pil_max_tiled_radius():
// row z blurs img [H][W][3] into out[slot] of out [nslots][H][W][3]
void launch_blur_pil_tiled(const uint8_t* img, int H, int W, const int* table, int n, int rmax, int nslots,
                           uint8_t* out, hipStream_t s);
// any box radius: six one-pass launches img -> s1 -> s2 -> ... -> out, all [H][W][3]
void launch_blur_pil_general(const uint8_t* img, int H, int W, int r, uint32_t ww, uint32_t fw, uint8_t* s1,
                             uint8_t* s2, uint8_t* out, hipStream_t s);

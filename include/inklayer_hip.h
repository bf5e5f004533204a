/*
 * inklayer_hip.h — C ABI of libinklayer_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the InkLayer detector→segmentor hot path.  The
 * reference (ooowedyn/InkLayer) is Python on torch.nn modules plus ONE native
 * extension (groundingdino._C: ms_deform_attn_forward / _backward).  Every entry point below
 * replaces one reference call site (cited as file:line under
 * /root/reference; GD/ = InkLayer/third_party/GroundingDINO/groundingdino/,
 * SA/ = InkLayer/third_party/segment-anything/segment_anything/).
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers
 *     unless a parameter says "host";
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work
 *     on it (no allocation, no synchronisation: safe under hipGraph capture);
 *   - return value: 0 = ok, 1 = bad argument (nothing was launched),
 *     2 = the HIP launch failed;
 *   - "f16" is IEEE binary16 (_Float16); accumulation is always f32;
 *   - inputs are borrowed, outputs are caller-allocated.
 */
#ifndef INKLAYER_HIP_H
#define INKLAYER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INK_ABI_VERSION 10
int ink_abi_version(void);

/* ------------------------------------------------------------------------
 * Dense projection:  C[row_map[m], n] = residual[row_map[m], n]
 *                       + col_scale[n] * act( sum_k A[m,k] * W[n,k] + bias[n] )
 * W is in nn.Linear layout [N,K] (K contiguous).  MFMA 16x16x32 f16, f32 acc.
 * Replaces every nn.Linear / 1x1-conv / im2col-conv on the path, e.g.
 *   SA/modeling/image_encoder.py:231 (qkv), :237 (proj), SA/modeling/common.py:25
 *   (MLPBlock lin1+GELU+lin2), GD/.../swin_transformer.py:140,170 (qkv/proj),
 *   GD/.../transformer.py:789-795 (encoder FFN), SA/modeling/mask_decoder.py:53-59
 *   (ConvTranspose2d k2s2 as a [256 -> 4*64] projection).
 * Constraints: K % 32 == 0, N % 4 == 0, lda/ldw % 8 == 0, ldc/ldr % 4 == 0,
 * A/W 16-byte aligned.
 * --------------------------------------------------------------------- */
typedef struct InkGemm {
  const void* A;            /* f16 [M, lda] */
  const void* W;            /* f16 [N, ldw] */
  const float* bias;        /* [N] or NULL */
  const float* col_scale;   /* [N] or NULL */
  const float* residual;    /* f32 [*, ldr] or NULL; indexed by OUTPUT row */
  const int32_t* row_map;   /* [M]: output row of input row m, <0 drops the row; NULL = identity */
  void* C;                  /* f32 or f16 [*, ldc] */
  int32_t M, N, K;
  int32_t lda, ldw, ldr, ldc;
  int32_t act;              /* 0 none, 1 GELU(erf), 2 ReLU */
  int32_t c_f16;            /* 0: C is f32, 1: C is f16 */
} InkGemm;
#define INK_ACT_NONE 0
#define INK_ACT_GELU 1
#define INK_ACT_RELU 2
int ink_gemm_f16(const InkGemm* p, void* stream);
/* Test hook: force one of the heuristic's tile families for every following ink_gemm_f16 call (0 = 128x128,
 * 10 = 16-wave 256x256, 45 = ping-pong 256x320, each with the tile order the heuristic gives it); -1 restores the
 * built-in shape heuristic.  Any other v returns INK_ERR_ARG.  Results are identical across families up to f32
 * summation order; K % 64 != 0 always takes the 128x128x32 tile, and a family that cannot take a call's form makes
 * ink_gemm_f16 return INK_ERR_ARG.  Process-wide, not thread-safe, never set by the product path. */
int ink_gemm_set_variant(int32_t v);
/* Which tile variant the built-in heuristic picks for (M,N,K): 45 = 256x320 ping-pong (the dominant kernel),
 * 10 = 256x256x64 / 16 waves, 0 = 128x128x64 / 4 waves, 32 = 128x128x32 (K % 64 != 0).  Pure host function, used by
 * bench.py's roofline. */
int ink_gemm_query_variant(int32_t M, int32_t N, int32_t K);

/* ------------------------------------------------------------------------
 * Row LayerNorm with optional row gather (fuses window-partition / pad /
 * cyclic shift into the normalisation pass).
 *   out[r, :] = LN(x[gather[r], :]) * gamma + beta      (gather[r] < 0 -> zeros)
 * Replaces nn.LayerNorm + window_partition (SA/modeling/image_encoder.py:168-172,
 * :243-264) and norm1 + pad + roll + window_partition
 * (GD/.../swin_transformer.py:246-265).  x is f32; out is f16 and/or f32.
 * C % 4 == 0, C <= 2048.  act: INK_ACT_NONE or INK_ACT_GELU applied after the affine
 * (LayerNorm2d + GELU of SA/modeling/mask_decoder.py:54-56).
 * split = 1: out_f16 rows are SPLIT-f16 operands [hi | lo*64 | hi/64] of 3*C columns (ldo >= 3*C), see
 * ink_add_split_f16; an f32 copy may be written in the same pass: out_f32 rows then have stride ldo / 3.
 * add (f32 or NULL, not together with gather): the row normalised is x[r] + add[add_batch_rows[r / rows_per_batch] +
 * r % rows_per_batch] (add_batch_rows NULL: add[r]) - the residual add of SA/modeling/transformer.py:180-181 when the
 * image keys are still shared by all boxes of an image (no per-box copy of them is ever made).
 * --------------------------------------------------------------------- */
int ink_layernorm_rows(const float* x, int64_t ldx, const float* gamma, const float* beta,
                       float eps, const int32_t* gather, int32_t rows_out, int32_t C,
                       void* out_f16, float* out_f32, int64_t ldo, int32_t act, int32_t split,
                       const float* add, int64_t ld_add, const int32_t* add_batch_rows, int32_t rows_per_batch,
                       void* stream);

/* f32 -> f16 conversion with optional broadcast addend:  out[i] = f16(a[i] + b[i % n_b])
 * (b may be NULL).  n % 4 == 0, n_b % 4 == 0, n % n_b == 0.  Used for the "x + pos" operands of
 * GD/.../transformer.py:783 and SA/modeling/transformer.py:164-165,178-179 (keys + key_pe). */
int ink_add_cvt_f16(const float* a, const float* b, int64_t n_b, void* out_f16, int64_t n,
                    void* stream);
/* Split-f16 GEMM operand: v = a[i] + b[i % n_b] (f32, rows of C columns, contiguous) is written as three
 * f16 K-segments  out[r, 0:C] = hi = f16(v),  out[r, C:2C] = f16((v - hi) * 64),  out[r, 2C:3C] = f16(hi / 64)
 * (out is [n / C, 3*C]).  Multiplied by ink_gemm_f16 against weights laid out [W_hi | W_hi/64 | (W - W_hi)*64]
 * the f32 accumulator receives hi*W_hi + lo*W_hi + hi*W_lo, i.e. an fp32-grade product (~2^-21 relative) on the
 * f16 MFMA pipe.  Used for the layers whose f16 rounding dominates the mask error (SAM neck, prompt/mask decoder,
 * upscaler, hyper-network: SA/modeling/image_encoder.py:88-104, mask_decoder.py:112-149, transformer.py:62-240);
 * the reference computes these in fp32. */
int ink_add_split_f16(const float* a, const float* b, int64_t n_b, void* out_f16, int64_t n, int32_t C,
                      void* stream);
/* Same with an f32 result (src = image_embeddings + dense_prompt, SA/modeling/mask_decoder.py:124-125). */
int ink_add_f32(const float* a, const float* b, int64_t n_b, float* out, int64_t n, void* stream);

/* ------------------------------------------------------------------------
 * Fused softmax attention  O = softmax(scale * Q K^T + bias) V   (f16 in/out, f32 math),
 * never materialising the score matrix.  Rows of batch b start at b*n_q (Q, O) and
 * b*n_k (K, V); head h occupies columns [h*head_dim, (h+1)*head_dim) of each row, so the
 * packed qkv projection output is consumed in place (ldq = ldk = ldv = 3*dim).
 * bias_mode 0: none.
 * bias_mode 1: SAM global blocks (SA/modeling/image_encoder.py:231-237,325-361) on a 64x64
 *              token grid: bias[q,k] = scale*(rel_h[q, k/64] + rel_w[q, k%64]); rel_h/rel_w are
 *              f32 [n_batch*n_heads, n_q, 64] as produced by ink_relpos_bias.
 * bias_mode 2: SAM 14x14 windows: rel_aug f16 [n_batch*n_heads, n_q, 32] from ink_relpos_bias
 *              (cols 0..S-1 = rel_h, S..2S-1 = rel_w); grid_w = S <= 16.  At SAM's own size
 *              (193 <= n_k <= 208, i.e. S = 14) a dedicated kernel runs (csrc/attention_win.hip); it addresses
 *              rows through 32-bit byte offsets: the O rows it writes must lie within 2 GiB of O, the
 *              q / k / v rows it gathers within 4 GiB of Q / K / V.
 * bias_mode 3: Swin windows (GD/.../swin_transformer.py:148-167), n_q, n_k <= 64: dense_bias f32
 *              [n_heads, n_q, 64] (relative_position_bias_table gathered by relative_position_index)
 *              + optional dense_mask f32 [n_mask, n_q, 64] (the 0/-100 SW-MSA mask; batch entry b
 *              uses mask b % n_mask).  Both are PRE-DIVIDED by `scale` and row-padded to 64.
 * Supported (head_dim, bias_mode) pairs: (80, 0), (80, 1), (80, 2), (64, 0), (64, 1), (64, 2), (32, 0), (32, 3),
 * (16, 0); anything else returns INK_ERR_ARG.  head_dim 64 with modes 1 and 2 (SAM ViT-B / ViT-L) runs the generic
 * templated kernel of csrc/attention.hip with the argument rules of head_dim 80 (mode 1: grid_w == 64,
 * n_k % 64 == 0, n_k <= 4096; mode 2: grid_w <= 16, n_k <= grid_w^2) and f32 rel_h / rel_w only: rel_f16 != 0 is a
 * head_dim-80 feature (csrc/attention_glob.hip) and returns INK_ERR_ARG at head_dim 64.
 * q_batch_rows / kv_batch_rows (int32 [n_batch], optional): first row of batch entry b in Q and in K/V;
 * NULL means b*n_q and b*n_k.  Lets many batch entries share one K/V (or Q) block, e.g.
 * SAM decoder layer 0 where the image keys are identical for all boxes of an image.  The tables redirect reads
 * only.  O is always dense: row b*n_q + i holds query i of entry b (entries that share Q rows still get their
 * own output rows), unless tok_rows scatters it.
 * tok_rows (int32 [n_batch, n_q], optional, bias_mode 2 only, n_q == n_k): token i of batch entry
 *   (window) b lives in row tok_rows[b*n_q + i] of Q, K, V AND O, or is window padding (-1).  This
 *   is window_partition / window_unpartition (SA/modeling/image_encoder.py:243-289) folded into
 *   the attention: a padding token is skipped as a query and contributes the rows pad_k / pad_v
 *   (f16 [n_heads*head_dim]: the k and v slices of the qkv bias, i.e. qkv(0)) as a key, exactly
 *   what the reference computes for its zero-padded rows - without ever projecting them.
 * --------------------------------------------------------------------- */
typedef struct InkAttn {
  const void* Q; const void* K; const void* V;   /* f16 */
  void* O;                                        /* f16 */
  int64_t ldq, ldk, ldv, ldo;                     /* row strides in elements */
  int32_t n_batch, n_heads, n_q, n_k, head_dim;
  float scale;
  int32_t bias_mode;
  int32_t grid_w;
  const int32_t* q_batch_rows;
  const int32_t* kv_batch_rows;
  const float* rel_h; const float* rel_w;         /* mode 1 (f16 tables when rel_f16 != 0: ink_relpos_bias64_f16) */
  const void* rel_aug;                            /* mode 2 */
  const float* dense_bias; const float* dense_mask; /* mode 3 */
  int32_t n_mask; int32_t rel_f16;                /* rel_f16: 0 / 1, SAM's own shape only (was padding: 0 in older callers) */
  const int32_t* tok_rows;                        /* mode 2, optional */
  const void* pad_k; const void* pad_v;           /* f16 rows used for tok_rows == -1 keys */
} InkAttn;
int ink_flash_attn(const InkAttn* p, void* stream);

/* ------------------------------------------------------------------------
 * Swin window attention with the relative-position bias and the SW-MSA mask computed in the kernel (ABI 9 gained
 * this one entry point; nothing else changed, so the version stays 9).  Per window w and head h
 *   O = softmax(scale q k^T + bias_table[h][rel(q, k)] + (region[w % nW][q] != region[w % nW][k] ? -100 : 0)) v
 * with rel(q, k) = (qy - ky + ws - 1) * (2 ws - 1) + (qx - kx + ws - 1), token i of a window at (i / ws, i % ws):
 * WindowAttention.forward (GD/.../swin_transformer.py:134-174) with relative_position_index (:111-121) and the
 * attn_mask of BasicLayer.forward (:417-441).  It serves the windows bias_mode 3 of ink_flash_attn cannot (ws = 12:
 * 144 tokens, Swin-B/384) without dense per-window tables; ws = 7 is served too, so the two can be compared.
 * Token i of window w is row w * ws^2 + i of Q, K, V (f16; head h in columns [32 h, 32 h + 32); column slices of the
 * packed qkv buffer: only the row strides matter) and of the dense output O f16 [n_windows * ws^2, >= n_heads * 32].
 * bias_table: f32 [n_heads, (2 ws - 1)^2], LOGIT units (relative_position_bias_table transposed; not divided by scale).
 * region: uint8 [nW, ws^2] ids (the nine-slice labelling of the shifted image), or NULL for an unshifted block.
 * head_dim is 32.  Refused with INK_ERR_ARG before any launch: ws other than 7 or 12; a null Q / K / V / O /
 * bias_table; a row stride that is not a multiple of 8 or is below n_heads * 32; Q / K / V not 16-byte or O not 8-byte
 * aligned; region with nW <= 0; nW > 0 with n_windows % nW != 0; n_windows, n_heads or scale <= 0.
 * --------------------------------------------------------------------- */
int ink_swin_attn(const void* Q, const void* K, const void* V, int64_t ldq, int64_t ldk, int64_t ldv,
                  void* O, int64_t ldo, int32_t n_windows, int32_t n_heads, int32_t ws, float scale,
                  const float* bias_table, const uint8_t* region, int32_t nW, void* stream);

/* ink_relpos_bias for the 64 x 64 grid with f16 output tables [n_batch*n_heads*4096, 64] (InkAttn.rel_f16 = 1). */
int ink_relpos_bias64_f16(const void* Q, int64_t ldq, const float* rel_pos_h, const float* rel_pos_w, int32_t n_batch,
                          int32_t n_heads, int32_t head_dim, float scale, void* out_h_f16, void* out_w_f16, void* stream);

/* Decomposed relative-position terms of SA/modeling/image_encoder.py:292-361
 * (get_rel_pos + the two einsums of add_decomposed_rel_pos), divided by `scale`:
 *   rel_h[bh, q, j] = (Q[b, q, h, :] . rel_pos_h[q_h - j + S - 1, :]) / scale   (same for w).
 * rel_pos_h / rel_pos_w: f32 [2S-1, head_dim], head_dim 80 (SAM ViT-H) or 64 (ViT-B / ViT-L) in both forms:
 * S == 64 writes out_h/out_w (f32 [.., 64]); S == 14 writes out_aug_f16 ([.., 32], rel_h then rel_w then zeros).
 * Any other head_dim returns INK_ERR_ARG (ink_relpos_bias64_f16 above stays head_dim 80 only).
 * tok_rows (optional, S <= 16 only): as in InkAttn - query i of window b is row tok_rows[b*S*S+i]
 * of Q (-1: padding, its output row is left untouched). */
int ink_relpos_bias(const void* Q, int64_t ldq, const float* rel_pos_h, const float* rel_pos_w,
                    int32_t S, int32_t n_batch, int32_t n_heads, int32_t head_dim, float scale,
                    const int32_t* tok_rows, float* out_h, float* out_w, void* out_aug_f16,
                    void* stream);

/* Sam.preprocess + PatchEmbed gather (SA/modeling/sam.py:164-174, image_encoder.py:364-395):
 * image_u8 is the ResizeLongestSide output, HWC uint8 [h, w, 3] (h, w <= L); writes the f16
 * im2col matrix [ (L/P)^2, 3*P*P ] (column = c*P*P + ky*P + kx, matching proj.weight.view(D,-1)),
 * with (x - mean[c]) / std[c] applied and the bottom/right padding left at 0.
 * mean3 / std3 are HOST pointers.  chan_reverse != 0 reads channel 2-c (the BGR/RGB quirk of
 * InkLayer/segmentor/sam.py:24-26 without an extra host copy).  split = 1: rows are split-f16 operands
 * [hi | lo*64 | hi/64] of 3*(3*P*P) columns (see ink_add_split_f16): the patch embedding is the one ViT-H
 * projection whose rounding error stays in the residual stream of all 32 blocks. */
int ink_sam_patchify(const void* image_u8, int32_t h, int32_t w, int32_t L, int32_t P,
                     const float* mean3, const float* std3, int32_t chan_reverse, int32_t split,
                     void* out_f16, void* stream);

/* Pillow's 8-bit two-pass resampler (PIL Image.resize with an antialiasing filter) on an HWC uint8 image of 1 or 3
 * interleaved channels, bit for bit: the bilinear `F.resize` of load_image (GD/util/inference.py:39-50,
 * GD/datasets/transforms.py:87-117: shorter side 800, max 1333) and of ResizeLongestSide.apply_image
 * (SA/utils/transforms.py:26-31, 93-102); the inpainting stage's Image.resize(LANCZOS) of images and masks
 * (inpaint_ControlNet.py:150-151, 161, 176, inpaint_single_layer.py:43-44, 63) and the default bicubic resize of
 * inpaint_SDXL.py:23-24.  src [h, w, channels] -> dst [oh, ow, channels], not in place, every side <= 16384.
 * xbounds/ybounds: int32 [ow|oh, 2] = (first input sample, number of samples); xcoef/ycoef: int32 [ow|oh, kx|ky]
 * 22-bit fixed-point weights, both exactly as Pillow's precompute_coeffs + normalize_coeffs_8bpc produce them for the
 * filter (inklayer_amd/resize.py::pil_resize_coeffs); the tables of an axis that keeps its size may be NULL.
 * Horizontal pass first, rounded to u8 into tmp_u8 [h, ow, channels] (needed only when both sizes change), then the
 * vertical pass.  The same size on both axes is a copy, as Image.resize makes one. */
int ink_resize_u8(const void* src_u8, int32_t h, int32_t w, int32_t channels, void* dst_u8, int32_t oh, int32_t ow,
                  const int32_t* xbounds, const int32_t* xcoef, int32_t kx, const int32_t* ybounds,
                  const int32_t* ycoef, int32_t ky, void* tmp_u8, void* stream);

/* 3x3 / pad 1 im2col of an NHWC f16 map with stride 1 or 2 and an optional ReLU applied to the gathered values:
 * [B*H*W, C] -> [B*OH*OW, 9*C] with column (ky*3+kx)*C + c, OH = (H - 1) / stride + 1, OW likewise; C % 8 == 0.
 * The neck conv of SA/modeling/image_encoder.py:96-103; ResidualConvUnit's activation(x) before conv1
 * (DA/util/blocks.py:69-70) and the stride-2 resize conv of DA/dpt.py:72-77. */
int ink_im2col3x3_f16(const void* in_f16, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride, int32_t relu,
                      void* out_f16, void* stream);

/* PositionEmbeddingRandom._pe_encoding (SA/modeling/prompt_encoder.py:186-193):
 * out[n] = [sin(2*pi*((2c-1) @ G)), cos(2*pi*((2c-1) @ G))], coords01 f32 [N,2] in [0,1]^2,
 * G f32 [2,F], out f32 [N,2F]; if `add` (f32 [n_add, 2F]) is given, out[n] += add[n % n_add]
 * (the learned corner embeddings).  Serves _embed_boxes (:93-100) and get_dense_pe (:62-71). */
int ink_sam_pe_encode(const float* coords01, const float* gauss, int32_t N, int32_t F,
                      const float* add, int32_t n_add, float* out, void* stream);

/* The whole token block of the SAM mask decoder for P prompts (SA/modeling/prompt_encoder.py:73-100, 128-166;
 * mask_decoder.py:113-116): out f32 [P, NT, 2F], NT = 5 + n_pts + pad + 2 * (boxes != NULL) <= 16, holds the 5 output
 * tokens (out_tok f32 [5, 2F]: iou token + 4 mask tokens), then the point tokens, then the two box corners.  points f32
 * [P, n_pts, 2] (x, y) and boxes f32 [P, 4] (xyxy) are in the resized-input frame: they are shifted by +0.5 and divided
 * by input_size here.  labels int32 [P, n_pts]; pad = 1 appends the point (0, 0) with label -1 (the reference pads when
 * there is no box).  Label -1: not_a_point (f32 [2F]) in place of the positional encoding; 0 / 1: the encoding +
 * point_emb[label]; any other label: the encoding alone.  point_emb f32 [4, 2F] = point_embeddings 0..3 (negative,
 * positive, box corner 0, box corner 1).  A box-only block equals ink_sam_pe_encode(.., add = point_emb + 2F, n_add 2)
 * behind the 5 output tokens, bit for bit. */
int ink_sam_prompt_tokens(const float* points, const int32_t* labels, int32_t n_pts, int32_t pad, const float* boxes,
                          const float* gauss, int32_t F, const float* point_emb, const float* not_a_point,
                          const float* out_tok, float input_size, int32_t P, float* out, void* stream);

/* Mask prompt (PromptEncoder.mask_downscaling, prompt_encoder.py:50-59) added to the image embedding
 * (mask_decoder.py:123-126), fused: keys f32 [P*g*g, 256], keys[p*g*g + t] = emb[emb_rows[p] + t] + dense(mask[p])[t]
 * with dense = Conv1x1(16 -> 256)(GELU(LN2d(Conv2x2s2(4 -> 16)(GELU(LN2d(Conv2x2s2(1 -> 4)(mask))))))).  mask f32
 * [P, 1, 4g, 4g] logits (g <= 64), emb f32 [*, 256] token rows, emb_rows int32 [P].  params f32 [4684] = the layers'
 * tensors flattened in order: conv1 w [4,1,2,2], b [4], LN w [4], b [4], conv2 w [16,4,2,2], b [16], LN w [16], b [16],
 * conv3 w [256,16,1,1], b [256]; n_params must be 4684.  eps: the LayerNorm2d epsilon (1e-6).  split_f16 (f16 [P*g*g, 768]
 * or NULL) receives the split-f16 GEMM operand of keys (see ink_add_split_f16) in the same pass.  16-byte aligned
 * mask / emb / keys. */
int ink_sam_mask_embed(const float* mask, const float* emb, const int32_t* emb_rows, const float* params,
                       int32_t n_params, float eps, int32_t P, int32_t g, float* keys, void* split_f16, void* stream);

/* masks = hyper_in @ upscaled_embedding for ONE mask token (SA/modeling/mask_decoder.py:139-144),
 * reading the ConvTranspose output in its un-shuffled GEMM layout
 * up[((b*g*g + y*g + x)*4 + (dy1*2+dx1))*4 + (dy2*2+dx2), C] and writing the pixel-shuffled
 * low-res logits out[b, 4y+2dy1+dy2, 4x+2dx1+dx2] (f32 [n, 4g, 4g]).  C in {32, 8}. */
int ink_sam_mask_logits(const float* up, const float* hyper, int32_t n, int32_t g, int32_t C,
                        float* out, void* stream);

/* Sam.postprocess_masks + `> mask_threshold` (SA/modeling/sam.py:133-162, SA/predictor.py:238-241)
 * fused: bilinear S->L (align_corners=False), crop to [in_h,in_w], bilinear to [out_h,out_w],
 * compare.  out_u8 [n,out_h,out_w] gets 0/1; out_logits (optional, f32) the un-thresholded value. */
int ink_sam_postprocess(const float* low, int32_t n, int32_t S, int32_t L, int32_t in_h,
                        int32_t in_w, int32_t out_h, int32_t out_w, float thr, void* out_u8,
                        float* out_logits, void* stream);

/* ------------------------------------------------------------------------
 * Multi-scale deformable attention forward — the reference's ONLY native op.
 * ink_ms_deform_attn_forward mirrors groundingdino._C.ms_deform_attn_forward
 * (GD/models/GroundingDINO/csrc/vision.cpp:53-56, MsDeformAttn/ms_deform_attn.h:21-40,
 * ms_deform_attn_cuda.cu:21-81): value f32 [B,S,M,C], spatial_shapes int64 [L,2] (h,w),
 * level_start_index int64 [L], sampling_loc f32 [B,Q,M,L,P,2] (x,y in [0,1]), attn_weight f32
 * [B,Q,M,L,P], im2col_step (only validated: B % min(B, step) == 0) -> out f32 [B,Q,M*C].
 * The two int64 arrays are HOST pointers here (the reference reads them on the device; they are
 * 8 numbers known to the caller).  C must be 32.
 * --------------------------------------------------------------------- */
int ink_ms_deform_attn_forward(const float* value, const int64_t* spatial_shapes_host,
                               const int64_t* level_start_index_host, const float* sampling_loc,
                               const float* attn_weight, int32_t B, int32_t S, int32_t M, int32_t C,
                               int32_t Q, int32_t L, int32_t P, int32_t im2col_step, float* out,
                               void* stream);

/* ABI 5: the whole of groundingdino._C (vision.cpp:54-55) with the reference's DEVICE tables.
 * spatial_shapes int64 [L,2] (h,w) and level_start_index int64 [L] are device pointers, read by the
 * kernels (no host synchronisation); dtype selects the element type of every float buffer: 0 = f32,
 * 1 = f64 (anything else returns 1).  Any C >= 1 and L >= 1.  Shapes and layouts as above:
 * value [B,S,M,C], sampling_loc [B,Q,M,L,P,2] (x,y), attn_weight [B,Q,M,L,P], out / grad_output
 * [B,Q,M*C].  im2col_step is only validated (B % min(B, step) == 0).  Semantics of
 * oracle/gdino_ref.py:msda_core: h_im = y*H - 0.5, w_im = x*W - 0.5, a sample outside (-1,H) x (-1,W)
 * and a corner outside the map contribute 0.  The tables cannot be checked on the host: a level whose
 * rows would leave [0, S) (h or w <= 0, start < 0, start + h*w > S) contributes 0 and gets zero
 * gradients, so an inconsistent table gives wrong numbers but never an out-of-bounds access.
 * At f32 with C == 32 the forward gives the same bits as ink_ms_deform_attn_forward.
 *
 * The backward writes all three gradients completely (grad_value [B,S,M,C], grad_sampling_loc
 * [B,Q,M,L,P,2], grad_attn_weight [B,Q,M,L,P]); it zeroes grad_value on `stream` itself, so the
 * caller may pass uninitialised memory.  grad_value is accumulated with float atomics: its last bits
 * depend on arrival order and are NOT reproducible run to run (nor are the reference's); the other
 * two gradients are plain stores and are. */
int ink_ms_deform_attn_forward_dev(const void* value, const int64_t* spatial_shapes,
                                   const int64_t* level_start_index, const void* sampling_loc,
                                   const void* attn_weight, int32_t dtype, int32_t B, int32_t S, int32_t M,
                                   int32_t C, int32_t Q, int32_t L, int32_t P, int32_t im2col_step,
                                   void* out, void* stream);
int ink_ms_deform_attn_backward_dev(const void* value, const int64_t* spatial_shapes,
                                    const int64_t* level_start_index, const void* sampling_loc,
                                    const void* attn_weight, const void* grad_output, int32_t dtype,
                                    int32_t B, int32_t S, int32_t M, int32_t C, int32_t Q, int32_t L,
                                    int32_t P, int32_t im2col_step, void* grad_value,
                                    void* grad_sampling_loc, void* grad_attn_weight, void* stream);

/* Pipeline form of the same op (MultiScaleDeformableAttention.forward, ms_deform_attn.py:282-352,
 * minus the three Linear layers): value f16 [B,S,8,32]; proj f32 [B*Q, ldp] with columns
 * [0,256) = sampling_offsets(query) as (head,level,point,xy) and [256,384) = attention_weights(query)
 * as (head,level,point); softmax over the 16 (level,point) logits, the sampling-location arithmetic
 * (2-d refs: ref + off/(W_l,H_l); 4-d refs: ref_xy + off/4 * ref_wh * 0.5) and the bilinear
 * gather are fused; out f16 [B*Q, 256].  ref: f32, element (b,q) at b*ref_b_stride + q*ref_q_stride,
 * the same for every level (valid_ratios == 1).  shapes_host: int32 [4,2] (h,w), HOST pointer. */
int ink_msda_fused(const void* value_f16, const float* proj, int64_t ldp, const float* ref,
                   int32_t ref_dim, int64_t ref_q_stride, int64_t ref_b_stride,
                   const int32_t* shapes_host, int32_t B, int32_t S, int32_t Q, void* out_f16,
                   void* stream);

/* load_image normalisation (GD/util/inference.py:40-49: /255, -mean, /std) + Swin PatchEmbed 4x4/s4
 * gather (swin_transformer.py:480-489): u8 HWC [h,w,3] -> f16 [ceil(h/4)*ceil(w/4), 64]
 * (48 real columns c*16+ky*4+kx, 16 zero columns).  mean3/std3 are HOST pointers. */
int ink_swin_patchify(const void* image_u8, int32_t h, int32_t w, const float* mean3,
                      const float* std3, void* out_f16, void* stream);

/* PatchMerging (swin_transformer.py:314-340): out[r] = LN(concat of the 4 source rows gather4[r][0..3])
 * in f16 [rows, 4C]; index -1 = zero row (odd-size padding).  C <= 1024. */
int ink_layernorm_merge4(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                         const int32_t* gather4, int32_t rows, int32_t C, void* out_f16, void* stream);

/* nn.GroupNorm(G, C) on NHWC tokens x f32 [B,T,C] (input_proj, groundingdino.py:121-151);
 * stats_ws: f32 [B*G*2] scratch; out f32, batch b written at out + b*out_batch_stride. */
int ink_groupnorm_nhwc(const float* x, int32_t B, int32_t T, int32_t C, int32_t G, const float* gamma,
                       const float* beta, float eps, float* stats_ws, float* out,
                       int64_t out_batch_stride, void* stream);

/* Row gather of f32 rows (batch b reads row idx[b*idx_batch_stride + r] of x + b*x_batch_rows rows;
 * -1 -> zeros) into f16 and/or f32 [B*rows_per_batch, C]: masked_fill of invalid proposals
 * (GD/.../utils.py:111-113) and the top-k gathers of transformer.py:302-316. */
int ink_gather_rows(const float* x, int64_t ldx, int64_t x_batch_rows, const int32_t* idx,
                    int64_t idx_batch_stride, int32_t rows_per_batch, int32_t B, int32_t C,
                    void* out_f16, float* out_f32, void* stream);

/* softmax(scale q k^T [+ blocked -> -inf]) v against n_k <= 16 keys; head h at columns
 * [h*hd,(h+1)*hd); blocked: u8 [n_q, n_k] (1 = not allowed) or NULL.  io_f32 = 0: Q/K/V/O are f16 rows, hd in {32,64};
 * 1: f32 rows, hd in {16,32} (ld* in elements either way; the math is f32 in both).  q_batch_rows (int32 [B] or NULL):
 * first Q row of batch entry b (default b*n_q); keys and the output are dense.  q_add (f32 [n_q, n_heads*hd] or NULL) is
 * added to the query rows by position (the per-position constant pe.W of a projection of x + pe).
 * Q, K, V, O and q_add must be 16-byte aligned and every ld* a multiple of 8 elements (the kernels move 16-byte vectors);
 * anything else returns 1 with nothing launched.
 * Text self-attention (transformer_vanilla.py:114-116), decoder text cross-attention (transformer.py:893-900) and,
 * with f32 rows, the SAM mask decoder's token self-attention and image -> token attention
 * (SA/modeling/transformer.py:151-182: 7 x 7 and 4096 x 7). */
int ink_attn_fewkeys(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                     int32_t B, int32_t n_q, int32_t n_k, int32_t n_heads, int32_t head_dim, float scale,
                     const uint8_t* blocked, const int32_t* q_batch_rows, const float* q_add, int32_t io_f32, void* O,
                     int64_t ldo, void* stream);

/* ink_attn_fewkeys' contract for n_k <= 256 keys on f16 rows (head_dim 32 or 64, f32 math, blocked u8 [n_q, n_k] or
 * NULL, the same alignment rules; no q_batch_rows / q_add): the text attentions of a caption of 17..256 tokens.  A
 * VALU kernel with an online softmax over blocks of 8 keys (csrc/attn_few.hip) - about 0.24 GFLOP per image and decoder
 * layer, not MFMA work.  A fully blocked row gives zeros, not NaN. */
int ink_attn_midkeys(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, int32_t B,
                     int32_t n_q, int32_t n_k, int32_t n_heads, int32_t head_dim, float scale, const uint8_t* blocked,
                     void* O, int64_t ldo, void* stream);

/* BiMultiHeadAttention core (GD/.../fuse_modules.py:168-240), both directions, for 1 <= T <= 256 text tokens on f16 MFMA
 * (csrc/biattn_wide.hip): QV f16 [B*S, 2E] = [v_proj(v) | values_v_proj(v)], KL f16 [B*T, 2E] = [l_proj(l) |
 * values_l_proj(l)], E = 1024 (4 heads x 256), S <= 32768; out_v f16 [B*S, E] (softmax over the text tokens), out_l f16
 * [B*T, E] (softmax over the image tokens).  No score matrix in HBM: the text side is
 * a split over chunks of 1024 image tokens that recomputes the score tile, merged by a fourth kernel; no atomics, the
 * results of image b do not depend on B.  ws: f32 [ink_biattn_wide_workspace(B, S, T)] = with Tp = 32 ceil(T / 32):
 * B*4*(128 Tp + ceil(S/128) Tp + ceil(S/1024) Tp 258) floats.  Returns 1 with nothing launched for a null pointer, T
 * outside 1..256, E != 1024, S outside 1..32768, B outside 1..65535 (the image is a grid dimension; the workspace
 * query refuses the same ranges) or a base that is not 16-byte aligned.  (One more entry point
 * of ABI 9, like ink_swin_attn before it.) */
int ink_biattn_wide_workspace(int32_t B, int32_t S, int32_t T, int64_t* out_floats);
int ink_biattn_wide(const void* QV_f16, const void* KL_f16, int32_t B, int32_t S, int32_t T, int32_t E, float scale,
                    float* ws, void* out_v_f16, void* out_l_f16, void* stream);

/* ink_biattn_wide with ONE TOKEN COUNT PER IMAGE: a batch whose captions differ in length, padded to Tmax rows each.
 * It replaces the attention_mask_l arithmetic of fuse_modules.py:214-218 (masked_fill of the padded text columns with
 * -inf before the image side's softmax); the text side's rows at padded tokens, which nothing reads, become zeros.
 * t_len: int32 [B] ON THE DEVICE; image b's text rows are KL[b*Tmax .. b*Tmax + t_len[b]) and the kernels clamp
 * t_len[b] into 1..Tmax themselves.  The pad rows of KL are never read; the rows t >= t_len[b] of out_l f16 [B*Tmax, E]
 * are written as zeros.  Each workgroup takes its tile count from its own image's count, so that the results of
 * image b are bitwise those of ink_biattn_wide(B = 1, T = t_len[b]) on that image's rows.  ws: f32
 * [ink_biattn_wide_workspace(B, S, Tmax)].  Returns 1 with nothing launched for a null pointer (t_len included), Tmax
 * outside 1..256, and everything ink_biattn_wide refuses.  (Two more entry points of ABI 10: nothing existing
 * changes.) */
int ink_biattn_wide_varlen(const void* QV_f16, const void* KL_f16, int32_t B, int32_t S, int32_t Tmax,
                           const int32_t* t_len /* device, [B] */, int32_t E, float scale, float* ws,
                           void* out_v_f16, void* out_l_f16 /* [B*Tmax, E] */, void* stream);

/* ink_attn_midkeys with a mask and a key count per batch entry: the text attentions of a batch of padded captions.
 * blocked: u8 [n_q, n_k] per entry, blocked_batch_stride BYTES apart (0: one shared matrix, as ink_attn_midkeys; NULL:
 * none, and the stride must be 0) - the per-row self-attention masks bertwarper.py's
 * generate_masks_with_special_tokens_and_transfer_map gives for padded ids (transformer_vanilla.py:114-116).  k_len:
 * int32 [B] ON THE DEVICE or NULL: the keys t >= k_len[b] do not exist for entry b (key_padding_mask of
 * transformer.py:903-909 and of the text enhancer); they are never loaded, so their content, NaN included, reaches no
 * output.  The kernel clamps k_len[b] into 0..n_k; key rows stay at b*n_k + t.  A row with no allowed key gives zeros.
 * Return codes and argument rules are those of ink_attn_midkeys; a negative stride returns 1. */
int ink_attn_midkeys_varlen(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                            int32_t B, int32_t n_q, int32_t n_k, int32_t n_heads, int32_t head_dim, float scale,
                            const uint8_t* blocked, int64_t blocked_batch_stride, const int32_t* k_len,
                            void* O, int64_t ldo, void* stream);

/* ------------------------------------------------------------------------
 * The caption encoder (csrc/text_bert.hip): BERT as GD/.../bertwarper.py:31-166 runs it, for a batch of captions PACKED
 * row after row (caption b owns rows row_start[b] .. row_start[b+1]).  The rest of a layer is ink_gemm_f16 on split-f16
 * operands, ink_layernorm_rows and ink_add_split_f16 (inklayer_amd/text_encoder.py).  (Two more entry points of ABI
 * 10: nothing existing changes.)
 *
 * ink_text_embed_ln - HF BertEmbeddings.forward (word_embeddings(input_ids) + token_type_embeddings(0) +
 * position_embeddings(position_ids), LayerNorm; the position ids are bertwarper.py:224-273's, restarting per phrase):
 *   out[r] = LN(word[ids[r]] + pos[pos_ids[r]] + type_row) * gamma + beta     for R token rows.
 * ids / pos_ids: int32 [R] ON THE DEVICE; the kernel clamps them into 0..V-1 / 0..P-1, so that bad device data cannot
 * index out of range.  word f32 [V, C], pos f32 [P, C], type_row / gamma / beta f32 [C]; C % 4 == 0, C <= 2048; eps is
 * BERT's 1e-12.  One pass writes out_f32 [R, C] (the residual of the first layer) and out_split_f16 [R, 3C], the
 * split-f16 operand in ink_add_split_f16's layout.  Returns 1 with nothing launched for a null pointer, R / V / P < 1,
 * a bad C, or a base that is not 16-byte aligned (ids / pos_ids: 4). */
int ink_text_embed_ln(const int32_t* ids, const int32_t* pos_ids, int32_t R, const float* word, int32_t V,
                      const float* pos, int32_t P, const float* type_row, const float* gamma, const float* beta,
                      float eps, int32_t C, float* out_f32, void* out_split_f16, void* stream);

/* ink_attn_text_f32 - HF BertSelfAttention.forward with the sub-sentence block mask of bertwarper.py:117-126 (the
 * additive -inf mask built from generate_masks_with_special_tokens_and_transfer_map): softmax(scale q k^T, blocked ->
 * -inf) v per caption and head, f32 math throughout.  Q / K / V: f32 rows read IN PLACE from the packed qkv projection
 * (ld = 3 * n_heads * 64), head h at columns [64 h, 64 h + 64); head_dim must be 64, n_heads >= 1.  row_start: int32
 * [B + 1] ON THE DEVICE; at most Tmax <= 256 rows per caption, R rows in all: the kernel clamps every start into 0..R
 * and every count into 0..min(Tmax, R - start).  blocked: u8 [Tmax, Tmax] per caption, blocked_batch_stride BYTES apart
 * (0: one shared matrix; NULL: none, and the stride must be 0), the conventions of ink_attn_midkeys_varlen; a row with
 * no allowed key gives zeros, and a blocked key's rows reach no output.  out_split_f16 [R, >= 3 * n_heads * 64] (row
 * stride ldo halves) receives the context as the split-f16 operand of the output projection: head h fills its 64
 * columns in each of the three segments; out_f32 (row stride ldf; NULL to skip) an f32 copy.  A workgroup takes one
 * (caption, head, 64 queries), stages that head's K and V through LDS in tiles of 64 keys and skips a tile none of its
 * queries may see; all its bounds come from its own caption, so caption b's results are bitwise those of a B = 1
 * launch on that caption alone.  Returns 1 with nothing launched for a null pointer, head_dim != 64, B outside
 * 1..65535, Tmax outside 1..256, R < 1, ldq / ldk / ldv / ldf not a multiple of 4 or ldo not a multiple of 8, a
 * negative stride, or a base that is not 16-byte aligned (row_start: 4). */
int ink_attn_text_f32(const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* V, int64_t ldv,
                      const int32_t* row_start /* device, [B + 1] */, int32_t B, int32_t R, int32_t Tmax,
                      int32_t n_heads, int32_t head_dim, float scale, const uint8_t* blocked,
                      int64_t blocked_batch_stride, void* out_split_f16, int64_t ldo, float* out_f32, int64_t ldf,
                      void* stream);

/* softmax(scale q k^T) v for n_q <= 16 queries per batch entry against MANY keys (SAM decoder tokens ->
 * image: 7..16 x 4096, SA/modeling/transformer.py:163-168) on f32 rows: head h at columns [h*hd,(h+1)*hd), head_dim
 * must be 16 and n_heads a multiple of 4; q_batch_rows / kv_batch_rows as in InkAttn; O dense [n_batch*n_q, ..].
 * k_add (f32 [n_k, n_heads*hd] or NULL) is added to the key rows by key position.
 * Q, K, V, O and k_add must be 16-byte aligned and every ld* a multiple of 8 elements (the kernel moves 16-byte vectors);
 * anything else returns 1 with nothing launched. */
int ink_attn_fewq(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                  int32_t n_batch, int32_t n_q, int32_t n_k, int32_t n_heads, int32_t head_dim, float scale,
                  const int32_t* q_batch_rows, const int32_t* kv_batch_rows, const float* k_add, void* O, int64_t ldo,
                  void* stream);

/* Column (max, sum-exp) over the S rows of B score matrices [S, HT] f32 (HT <= 16): stats f32 [B, HT, 2];
 * part_ws f32 [B * ceil(S / 512) * HT * 2].  The text-side softmax statistics of the fusion layer. */
int ink_biattn_colstats(const float* scores, int32_t B, int32_t S, int32_t HT, float* part_ws, float* stats, void* stream);

/* BiAttentionBlock (GD/.../fuse_modules.py:146-295) with the <= 4 text tokens of InkLayer's fixed caption FOLDED through
 * it: the image tokens v f32 [B*S, 256] are updated IN PLACE to  LN_v(v) + gamma_v * out_v_proj(attention over text)  and
 * out_l f16 [B*T, 1024] receives the text-side attention output (operand of out_l_proj), without ever forming the per-token
 * q / value_v projections (256 -> 2 x 1024) or the 1024 -> 256 image output projection - see csrc/fusion_fold.hip for
 * the algebra.  text_k / text_vl: f32 [B*T, >= 1024] (row stride ld_text) = l_proj / values_l_proj of LN_l(l);
 * Wq / Wvv f16 [1024, 256] (v_proj / values_v_proj weights), bq / bvv f32 [1024]; Wo f16 [256, 1024], bo f32 [256]
 * (out_v_proj); scale = 256^-0.5.  ws: f32[ink_fusion_fold_workspace(B, S)].  S <= 32768.  Optional (NULL to skip): out16 f16
 * [B*S, 256] = f16(updated v) and out16_pos = f16(updated v + pos[s]) with pos f32 [S, 256] - the operands of the
 * deformable attention's value / sampling projections (transformer.py:780-789), written in the same pass. */
int ink_fusion_fold_workspace(int32_t B, int32_t S, int64_t* out_floats);
int ink_fusion_fold(float* v_f32, int32_t B, int32_t S, const float* lnv_g, const float* lnv_b, float eps,
                    const float* text_k_f32, const float* text_vl_f32, int64_t ld_text, int32_t T, const void* Wq_f16,
                    const float* bq, const void* Wvv_f16, const float* bvv, const void* Wo_f16, const float* bo,
                    const float* gamma_v, float scale, float* ws, void* out_l_f16, const float* pos, void* out16_pos,
                    void* out16, void* stream);

/* Tail of the SAM mask decoder in one kernel (csrc/upscale_tail.hip): LayerNorm2d + GELU + the second ConvTranspose2d
 * (k2 s2 = a [64 -> 4 x 32] projection per row) + GELU + the hyper-network product of n_masks in {1, 3, 4}
 * mask tokens per box (SA/modeling/mask_decoder.py:54-60, 138-145; the upscaling is computed once per row and shared by
 * the masks, and mask m of a 4-mask call equals a 1-mask call with hyper vector m bit for bit).  u0 f32: the first transposed convolution's output, 4 x 64 floats per
 * (box, token) at token stride ld_tok (>= 256 floats: it may be a column block of a wider projection), row (token, s1); ln_g / ln_b f32 [64] (output_upscaling.1), eps 1e-6; blob: output_upscaling.3.weight as the
 * split-f16 matrix [128, 192] (rows (s2, c), see ink_add_split_f16) packed by ink_sam_upscale_pack (48 KiB); b3 f32 [128]
 * (the bias repeated per sub-pixel); hyper f32 [n, n_masks, 32]; low f32 [n, n_masks, 4g, 4g].
 * (g*g*4) % 32 == 0. */
int ink_sam_upscale_pack(const void* ws_f16, void* blob_f16, void* stream);
int ink_sam_upscale_tail(const float* u0, int64_t ld_tok, int32_t n, int32_t g, const float* ln_g, const float* ln_b, float eps,
                         const void* blob_f16, const float* b3, const float* hyper, int32_t n_masks, float* low,
                         void* stream);

/* Image-side tail of a layer of SAM's two-way transformer in one kernel (csrc/proj_ln.hip):
 *     out = LayerNorm(res + a W^T + bias)         a f32 [rows, 128] (the image->token attention's output), 256 columns
 * = cross_attn_image_to_token.out_proj + the residual + norm4 (SA/modeling/transformer.py:175-182).  The projection runs
 * on split-f16 operands (built in registers from a; blob = the weight as the split-f16 matrix [256, 384] packed by
 * ink_proj256_ln_pack, 192 KiB).  res f32 [.., 256]: row r, or - res_batch_rows given - row res_batch_rows[r /
 * rows_per_batch] + r % rows_per_batch of a tensor shared by the boxes of an image.  Outputs (either may be NULL): out_f32
 * [rows, 256] and out_split_f16 [rows, 768], the split-f16 operand [hi | lo*64 | hi/64] of the next projection. */
int ink_proj256_ln_pack(const void* ws_f16, void* blob_f16, void* stream);
int ink_proj256_ln(const float* a_f32, const void* blob_f16, const float* bias, const float* res_f32,
                   const int32_t* res_batch_rows, int32_t rows_per_batch, const float* ln_g, const float* ln_b, float eps,
                   int64_t rows, float* out_f32, void* out_split_f16, void* stream);

/* Feed-forward block of the deformable encoder layer, fused (csrc/ffn_fused.hip):
 *     out = LayerNorm(res + linear2(relu(linear1(x))))      d_model 256, d_ffn = hid (multiple of 64, <= 2048)
 * = DeformableTransformerEncoderLayer.forward_ffn + norm2 (GD/models/GroundingDINO/transformer.py:780-799).  x f16 [M, 256]
 * (row stride ldx) is the GEMM operand (f16 of the layer's input), res f32 [M, 256] the same rows in f32 (the residual);
 * out f32 [M, 256] may alias res.  The hidden activations are rounded to f16 between the two products, as in the two-GEMM
 * form.  blob: the weights packed by ink_ffn256_pack (ink_ffn256_pack_bytes(hid) bytes, 16-B aligned) from linear1.weight
 * f16 [hid, 256], linear1.bias f32 [hid] (carried as an f16 hi + lo pair in a 17th k-step, i.e. to 2^-22) and
 * linear2.weight f16 [256, hid]: per 64 hidden units the LDS image the kernel streams - 1-KiB MFMA operand blocks,
 * linear2's columns permuted inside 16-blocks to the order phase A leaves them in registers.  b2: linear2.bias. */
int ink_ffn256_pack_bytes(int32_t hid, int32_t with_pre, int64_t* out_bytes);
int ink_ffn256_pack(const void* w1_f16, const float* b1, const void* w2_f16, int32_t hid, const void* wpre_f16, void* blob,
                    void* stream);
int ink_ffn256_fused(const void* x_f16, int64_t ldx, const float* res_f32, const void* blob, const float* b2,
                     const float* ln_g, const float* ln_b, float eps, int32_t M, int32_t hid, const float* pre_bias,
                     const float* pre_ln_g, const float* pre_ln_b, float* out_f32, void* stream);
/* With a PRECEDING projection (wpre_f16 f16 [256, 256] given to the pack, pre_bias / pre_ln_g / pre_ln_b f32 [256] to the
 * call; all NULL = the plain form above): x is the input of that projection and the kernel computes
 *     s = LayerNorm_pre(res + x wpre^T + pre_bias);   out = LayerNorm(s + linear2(relu(linear1(f16(s)))))
 * = the deformable attention's output projection + residual + norm1 + the feed-forward block + norm2 of
 * DeformableTransformerEncoderLayer.forward (transformer.py:780-799) in one launch; s never leaves the registers. */

/* Two-stage query selection (transformer.py:293-300): indices of the K largest max_t logits[b,s,t],
 * descending, ties -> lower index.  logits f32 [B,S,T]; out_idx int32 [B,K].  S <= 16384 is one LDS
 * bitonic sort per image; larger S (800x1333 inputs give 22223 tokens) sorts ceil(S/16384) equal chunks and
 * merges their K best: cand_ws must then hold B * nchunk * K uint64. */
int ink_topk_rowmax(const float* logits, int32_t B, int32_t S, int32_t T, int32_t K, int32_t* out_idx,
                    float* out_val, void* cand_ws, void* stream);

/* gen_sineembed_for_position (GD/.../utils.py:204-230) for boxes ref f32 [N,4] -> f16 [N,512];
 * dim_t f32 [128] = 10000^(2*(i//2)/128). */
int ink_sine_embed4(const float* ref, const float* dim_t, int32_t N, void* out_f16, void* stream);

/* out = sigmoid(delta[:, :4] + inverse_sigmoid(ref))  (transformer.py:716-722, util/misc.py:704-708);
 * ref_is_logit != 0: ref is already un-sigmoided (two-stage anchors, transformer.py:296-305). */
int ink_box_refine(const float* delta, int64_t ldd, const float* ref, int32_t N, int32_t ref_is_logit,
                   float* out, void* stream);

/* Closed-set class scoring (PostProcessCocoGrounding.forward, GD/demo/test_ap_on_coco.py:99-106; the given-phrase mode
 * of GD/demo/inference_on_a_image.py:117-124):
 *     out[b, q, c] = sum_t sigmoid(logits[b, q, t]) * pos_map[c, t]          f32 [B, nq, C]
 * logits f32 [B, nq, T], row (b, q) at logits + (b * nq + q) * ld_row, ld_row >= T, T <= 256 and in no way aligned;
 * pos_map f32 [C, T] shared by the images (pm_image_stride == 0) or [B, C, T] with image b's map at
 * pos_map + b * pm_image_stride (>= C * T; rows of classes an image does not have are zero or cut off by n_cls);
 * n_cls int32 [B] or NULL: classes c >= n_cls[b] of image b score -1.0, below every real score (those are >= 0).
 * A -inf logit contributes exactly 0 and a +inf logit exactly pos_map[c, t]; no NaN-free input makes a NaN.  The sum
 * runs in f32 in an order that depends on t alone (four terms per lane upwards, then a 64-lane butterfly), so zero
 * terms - pad columns, entries outside a class's span - change no bit, and an image's scores do not depend on B, on
 * the other images or on how far T is padded.  All pointers 4-byte aligned; B <= 65535; nq * C < 2^31. */
int ink_class_scores(const float* logits, int64_t ld_row, const float* pos_map, int64_t pm_image_stride,
                     const int32_t* n_cls, int32_t B, int32_t nq, int32_t T, int32_t C, float* out, void* stream);

/* The boxes of the selected (query, class) pairs (test_ap_on_coco.py:118-132): idx int32 [B, K] = query * Cmax + class
 * (ink_topk_rowmax over the scores viewed as [B, nq * Cmax, 1]); boxes f32 [B, nq, 4] cxcywh; scale_wh f32 [B, 2] =
 * (w, h) of each image ((1, 1): normalised).  out_boxes f32 [B, K, 4] = (cx - 0.5 w, cy - 0.5 h, cx + 0.5 w, cy + 0.5 h)
 * * (W, H, W, H) (box_ops.box_cxcywh_to_xyxy, then the scale), labels int32 [B, K] = idx % Cmax, query int32 [B, K] =
 * idx / Cmax.  An index outside [0, nq * Cmax) reads nothing: zeros, label and query -1.  boxes / out_boxes 16-byte
 * aligned; B * K <= 2^30. */
int ink_select_boxes(const int32_t* idx, const float* boxes, const float* scale_wh, int32_t B, int32_t K, int32_t nq,
                     int32_t Cmax, float* out_boxes, int32_t* labels, int32_t* query, void* stream);

/* ------------------------------------------------------------------------
 * Mask hand-off stage of the refinement, on resident masks.  Integer / byte work, bit-exact with the
 * reference's cv2 results.
 *
 * ink_mask_cleanup = clean_up_mask of InkLayer/refinement/mask_cleaner.py:11-36 for n masks at once:
 *   cv2.threshold(m, 127, 255) -> cv2.morphologyEx(MORPH_CLOSE, k x k rect, k odd = calculate_kernel_size(shape),
 *   mask_cleaner.py:6-9) -> cv2.connectedComponentsWithStats(connectivity=8) -> keep components with
 *   area > area_threshold (500) OR max(w,h) / (min(w,h) + 1e-5) > aspect_threshold (1.1).
 * masks_u8 / out_u8: [n, H, W] uint8 (any value > 127 is foreground on input; 0 / 255 on output), the masks stay in
 * HBM instead of travelling through masks/mask_i.png -> masks_cleaned/mask_i.png (runner.py:57-60,69).
 * tmp_a / tmp_b: [n, H, W] uint8 scratch (tmp_a 8-byte aligned); workspace: int32[ink_mask_cleanup_workspace_ints(n, H,
 * W, k)].  8 <= W <= 16383, H <= 16383; a refused call launches nothing. */
int ink_mask_cleanup_workspace_ints(int32_t n, int32_t H, int32_t W, int32_t k, int64_t* out_ints);
int ink_mask_cleanup(const void* masks_u8, int32_t n, int32_t H, int32_t W, int32_t k, int32_t area_threshold,
                     double aspect_threshold, void* tmp_a_u8, void* tmp_b_u8, int32_t* workspace, void* out_u8,
                     void* stream);

/* Pair table of the sketch NMS (content_iou, InkLayer/refinement/nms_sketch.py:186-234, which re-opens the sketch and
 * two mask PNGs PER PAIR): refined_m = (mask_m > 0) AND (PIL-luma(sketch) < 250) (refine_mask_to_sketch_regions,
 * nms_sketch.py:62-78); counts[i, j] = (|refined_i AND refined_j|, |refined_i OR refined_j|) as int32 [n, n, 2].
 * sketch_rgb_u8: [H, W, 3] (the masks have the sketch's size on this path); bits_ws: uint64[n * ceil(H*W/64)]. */
int ink_mask_sketch_iou_counts(const void* masks_u8, const void* sketch_rgb_u8, int32_t n, int32_t H, int32_t W,
                               void* bits_ws_u64, int32_t* counts, void* stream);

/* ------------------------------------------------------------------------
 * SamAutomaticMaskGenerator's tail on low-res logits (SA/automatic_mask_generator.py:266-321, SA/utils/amg.py).
 * COLUMN-MAJOR BIT PLANES: Hp = ceil(H / 64) uint64 words per column, bit b of word w of column x = pixel (64 w + b, x),
 * bits of rows >= H are 0; m planes are [m, W, Hp] - the order mask_to_rle_pytorch walks.  H, W <= 16383.
 *
 * ink_sam_amg_stats: for the masks index[0..m) of low f32 [n, S, S] (index NULL: masks 0..m; m_dev non-NULL: a device
 * int32, workgroups of masks >= *m_dev do nothing, so a filter made on the device needs no host round trip), with
 * v = Sam.postprocess_masks(low) resized to crop_h x crop_w - bit-identical to what ink_sam_postprocess writes to
 * out_logits for the same sizes, and never stored unless out_logits (f32 [m, crop_h, crop_w], test hook) is given:
 *   table int32 [m, 8] = count(v > thr + offset), count(v > thr - offset) (calculate_stability_score, amg.py:156-176),
 *     count(v > thr), then x_min, y_min, x_max, y_max of v > thr in crop coordinates (batched_mask_to_box,
 *     amg.py:303-346: inclusive maxima, 0 0 0 0 for an empty mask), 0;
 *   planes uint64 [m, orig_w, ceil(orig_h / 64)] = v > thr placed at (x0, y0) of the orig_h x orig_w frame, zeros
 *     outside the crop (uncrop_masks, amg.py:255-264).
 * thr and offset are doubles because the reference's are Python floats: each cut-off (thr, thr + offset, thr - offset) is
 * made in double and rounded to f32 once, as torch does for `tensor > python_float`.
 * The table and, for a true crop, the planes are zeroed on the stream first. */
int ink_sam_amg_stats(const float* low, int32_t n, const int32_t* index, int32_t m, const int32_t* m_dev, int32_t S,
                      int32_t L, int32_t in_h, int32_t in_w, int32_t crop_h, int32_t crop_w, double thr, double offset,
                      int32_t x0, int32_t y0, int32_t orig_h, int32_t orig_w, int32_t* table, void* planes_u64,
                      float* out_logits, void* stream);

/* mask_to_rle_pytorch (amg.py:107-135) for the planes select[0..k) (select NULL: planes 0..k) of H x W images:
 * ink_mask_rle_counts writes the number of counts of each mask (n_counts int32 [k]); ink_mask_rle_write writes the counts
 * themselves (column-major runs, the first one the leading zero run, hence 0 when the mask starts with a one) to
 * counts + offsets[i] (offsets int32 [k] = the caller's exclusive scan of n_counts). */
int ink_mask_rle_counts(const void* planes_u64, const int32_t* select, int32_t k, int32_t H, int32_t W,
                        int32_t* n_counts, void* stream);
int ink_mask_rle_write(const void* planes_u64, const int32_t* select, int32_t k, int32_t H, int32_t W,
                       const int32_t* offsets, int32_t* counts, void* stream);

/* remove_small_regions (amg.py:267-291) for k column-major planes of H x W images, one mode per call: holes != 0 fills the
 * 8-connected components of the COMPLEMENT with area < min_area; holes == 0 removes the components of the mask with
 * area < min_area, and if every one is that small keeps the largest (of equal areas the one whose first pixel comes first
 * in raster order: cv2.connectedComponentsWithStats' label order).  changed int32 [k] = 1 where a component below
 * min_area existed (the reference's flag), else 0.  tmp_planes: k planes of scratch; out_planes may be planes itself;
 * workspace: int32[ink_mask_small_regions_workspace_ints(k, H, W)], sized for the true run bound ceil(H / 2) per column,
 * so no mask can overflow it. */
int ink_mask_small_regions_workspace_ints(int32_t k, int32_t H, int32_t W, int64_t* out_ints);
int ink_mask_small_regions(const void* planes_u64, int32_t k, int32_t H, int32_t W, int32_t min_area, int32_t holes,
                           void* tmp_planes_u64, int32_t* workspace, void* out_planes_u64, int32_t* changed, void* stream);

/* torchvision.ops.nms for one category (batched_nms with idxs == 0, automatic_mask_generator.py:214-220, 251-257,
 * 357-362): boxes f32 [n, 4] xyxy, area = (x2 - x1)(y2 - y1), iou = inter / (a_i + a_j - inter) in f32, a box is
 * suppressed by a kept box of higher rank when iou > iou_threshold; rank = descending score, TIES TO THE LOWER INDEX
 * (torchvision leaves the order of ties open).  Scores must not be NaN.  keep int32 [n] = the kept indices in rank
 * order, *n_keep their number.  n <= 4096 (else return 1); workspace: uint64[n * (ceil(n / 64) + 3)], 16-byte aligned. */
int ink_box_nms(const float* boxes, const float* scores, int32_t n, float iou_threshold, void* workspace_u64,
                int32_t* keep, int32_t* n_keep, void* stream);

/* ------------------------------------------------------------------------
 * Refinement stage on resident masks: depth ordering support, disjoint parsing, mask growth, box
 * assignment support, the "unlabeled" extra mask.  Integer / bit work, bit-exact with the reference.
 * Binary images are ROW-ALIGNED BIT PLANES: Wp = ceil(W / 64) uint64 words per row, bit b of word w of row y = pixel
 * (y, 64 w + b), tail bits 0; n planes are [n, H, Wp].  Mask sets after the disjoint parsing are ONE uint8 label image
 * [H, W] (label l = mask index l - 1, 0 = no mask; at most 254 masks).  H, W <= 16383.
 *
 * ink_refine_sketch_planes: sketch RGB u8 [H, W, 3] -> 4 planes
 *   0: sketch_to_01binary of the cv2 BGR image (InkLayer/refinement/utils.py:3-9): blue <= max(all bytes) / 2
 *   1: PIL luma <  250 (refiner.py:106-110)        2: PIL luma <= 250 (refiner.py:134, 246)
 *   3: cv2 gray <  250 (refiner.py:302-303)        max_ws: int32[1] scratch. */
int ink_refine_sketch_planes(const void* rgb_u8, int32_t H, int32_t W, void* planes4_u64, int32_t* max_ws, void* stream);

/* uint8 images [n, H, W] -> planes (pixel > thresh). */
int ink_bitplane_pack(const void* img_u8, int32_t n, int32_t H, int32_t W, int32_t thresh, void* planes_u64, void* stream);

/* get_mask_depth_score's inputs (depth_sort.py:72-89): vals[p] = depth[pts[p]] and inside[m, p] = mask m covers sample p
 * (uint8 [n, P]); pts_yx int32 [P, 2] (y, x).  The binned mode itself is a few hundred numbers: host. */
int ink_refine_depth_samples(const void* mask_planes, int32_t n, const float* depth, const int32_t* pts_yx, int32_t P,
                             int32_t H, int32_t W, float* vals, void* inside_u8, void* stream);

/* All pair / per-mask counts the ordering and the disjoint parsing need, in one pass over the planes:
 *   D_m = cv2.dilate(mask_m & plane 0, 3x3 ellipse) (depth_sort.py:193-197)
 *   pair[i, j] = (|M_i & M_j| over the image (refiner.py:71-74), |D_i & D_j| inside rect[i, j] (depth_sort.py:222-231))
 *   per_mask[m] = (|M_m| (refiner.py:41), |D_m| (depth_sort.py:200), |M_m & plane 1| (refiner.py:108-110))
 *   sketch_area = |plane 1| (refiner.py:106)
 * rect int32 [n, n, 4] = (y0, y1, x0, x1): the pair's box intersection as RESOLVED numpy slice bounds (half open,
 * inside the image; the host applies numpy's rules for negative / oversized indices).  dil_ws: n planes of scratch.
 * pair int32 [n, n, 2], per_mask int32 [n, 3]. */
int ink_refine_pair_tables(const void* mask_planes, const void* sketch_planes4, int32_t n, int32_t H, int32_t W,
                           const int32_t* rect, void* dil_ws_planes, int32_t* pair, int32_t* per_mask,
                           int32_t* sketch_area, void* stream);

/* composite_and_parse_masks' layering (refiner.py:44-47): label = 1 + the first rank r whose mask order[r] covers the
 * pixel (order[r] < 0: rank emptied by the "covers the whole sketch" rule, refiner.py:104-112); hist256[l] = pixels. */
int ink_refine_composite(const void* mask_planes, const int32_t* order, int32_t n_ranks, int32_t H, int32_t W,
                         void* label_u8, int32_t* hist256, void* stream);

/* out = clean_delicate_mask (refiner.py:21-33) of every mask of map256[label]: a pixel with at most one 8-neighbour of
 * its own (mapped) label is cleared.  map256: uint8[256] on the device (0 drops a label). */
int ink_refine_relabel_clean(const void* label_u8, const void* map256_u8, int32_t H, int32_t W, void* out_label_u8,
                             void* stream);

/* refine_masks_with_watershed (refiner.py:129-196) on the label image: unlabeled stroke pixels (plane 2, label 0),
 * their closing by disk(3), its 4-connected components of more than 50 pixels ("large regions"), masks within disk(3)
 * of one grow by disk(3) (flags256[l] = 1), the others by disk(2); where several masks reach a pixel the largest label
 * wins; everything restricted to plane 2.  Also returns what refine_masks_with_boxes needs: bbox256x4[l] = (xmin, ymin,
 * xmax, ymax) of grown mask l ((W, H, -1, -1) if empty) and the still unlabeled stroke pixels in raster order
 * (unl_yx int32 [unl_cap, 2], *unl_count = their number, possibly > unl_cap).
 * planes_ws / cc_ws sizes: ink_refine_grow_workspace. */
int ink_refine_grow_workspace(int32_t H, int32_t W, int64_t* plane_words, int64_t* cc_ints);
int ink_refine_grow(const void* label_u8, const void* sketch_planes4, int32_t H, int32_t W, void* planes_ws,
                    int32_t* cc_ws, int32_t* flags256, void* out_label_u8, int32_t* bbox256x4, int32_t* unl_yx,
                    int32_t unl_cap, int32_t* unl_count, void* stream);

/* d2[q, l] = squared distance from pixel q_yx[q] to the nearest pixel of label l for the labels in cand (4 uint64 per
 * query = a 256-bit set), 0x7fffffff where the label has no pixel (`np.min(distances)` of refiner.py:277-281). */
int ink_refine_query_dists(const void* label_u8, const int32_t* q_yx, const void* cand256_bits, int32_t Q, int32_t H,
                           int32_t W, int32_t* d2_Qx256, void* stream);

/* Applies the assignments (y, x, label) of the raster-order loop to the label image (in place), then
 * create_unlabeled_mask (refiner.py:301-337): plane 3 minus the labelled pixels, cv2 MORPH_OPEN 3x3, cv2.dilate 2x2
 * -> extra_plane, *extra_count = its pixel count.  planes_ws3: 3 planes of scratch. */
int ink_refine_finalize(void* label_u8, const int32_t* assign_yxl, int32_t A, const void* sketch_planes4, int32_t H,
                        int32_t W, void* planes_ws3, void* extra_plane, int32_t* extra_count, void* stream);

/* HOST functions (host pointers, no GPU work): the two sequential algorithms of the stage.
 * ink_host_sparse_sample = sparse_sketch_sample (depth_sort.py:49-68) of the sketch (RGB u8 [H, W, 3]): greedy
 * row-major thinning of the plane-0 pixels with radius 0.01 H; out_yx int32 [cap, 2], *count = samples found.
 * ink_host_assign_unlabeled = the pixel loop of refine_masks_with_boxes (refiner.py:262-295): q_yx the unlabeled stroke
 * pixels in raster order, boxes int32 [nb, 4] (inclusive), box2mask[nb] (-1: unmatched), d2 int32 [Q, 256] from
 * ink_refine_query_dists, nonempty uint8 [n_masks]; out_label[q] = 1 + mask index, 0 = stays unlabeled. */
int ink_host_sparse_sample(const uint8_t* rgb_u8, int32_t H, int32_t W, int32_t* out_yx, int32_t cap, int32_t* count);
int ink_host_assign_unlabeled(const int32_t* q_yx, int32_t Q, const int32_t* boxes, int32_t nb, const int32_t* box2mask,
                              const int32_t* d2, const uint8_t* nonempty, int32_t n_masks, int32_t* out_label);

/* ------------------------------------------------------------------------
 * Depth-Anything-V2 (ViT-S / ViT-B / ViT-L) pixel-side ops (the dense layers reuse ink_gemm_f16 / ink_flash_attn /
 * ink_layernorm_rows).
 *
 * ink_depth_patchify = DepthAnythingV2.image2tensor (DA/dpt.py:199-221: BGR->RGB, /255, cv2.resize INTER_CUBIC to
 * (nw, nh), (x - mean) / std) fused with the 14x14 / s14 patch gather of DA/dinov2_layers/patch_embed.py:
 * image_u8 [H, W, 3] -> split-f16 im2col rows [ (nh/P)*(nw/P), 3*KP ], KP = 3*P*P rounded up to a multiple of 32
 * (zero columns), column = c*P*P + ky*P + kx.  chan_reverse != 0 reads channel 2-c (cv2.imread's BGR order).
 * mean3 / std3 are HOST pointers.  float64 arithmetic like cv2 on a CV_64F image. */
int ink_depth_patchify(const void* image_u8, int32_t H, int32_t W, int32_t nh, int32_t nw, int32_t P, int32_t KP,
                       const double* mean3, const double* std3, int32_t chan_reverse, void* out_f16, void* stream);

/* F.interpolate(mode="bilinear", align_corners=True) on an NHWC f32 map [B, h, w, C] -> [B, H, W, C] (f32 and/or
 * f16 copy): the up-samplings of FeatureFusionBlock (DA/util/blocks.py:136-146), of DPTHead.forward
 * (DA/dpt.py:146) and of infer_image (DA/dpt.py:195).  C % 4 == 0 or C < 4. */
int ink_resize_bilinear_ac_nhwc(const float* in, int32_t B, int32_t h, int32_t w, int32_t C, int32_t H, int32_t W,
                                float* out_f32, void* out_f16, void* stream);

/* Direct (implicit-GEMM) 3x3 / pad 1 convolution of an NHWC f16 map, stride 1 or 2; the im2col matrix is never
 * written.  With OH = (H - 1) / stride + 1, OW likewise and M = B*OH*OW:
 *   out[(b,oy,ox), n] = residual[(b,oy,ox), n]
 *                       + act( sum_{ky,kx,c} relu_in?( in[b, oy*stride+ky-1, ox*stride+kx-1, c] ) * wt[n, (ky*3+kx)*C + c]
 *                              + bias[n] )
 * in f16 [B*H*W, C]; wt f16 [N, 9*C] (a Conv2d weight [N, C, 3, 3] permuted to (n, ky, kx, c)); bias f32 [N] or NULL;
 * relu_in 0 / 1; act INK_ACT_NONE or INK_ACT_RELU; residual f32 [M, N] or NULL; out f32 (out_f16 = 0) or f16 (1) [M, N].
 * Replaces the convolutions of the DPT head without their im2col matrices: ResidualConvUnit (DA/util/blocks.py:59-84:
 * relu_in + bias + ReLU for conv1, bias + residual for conv2), the stride-2 resize conv (DA/dpt.py:72-77), and
 * layer*_rn / output_conv1 / output_conv2 (DA/dpt.py:92-110).
 * Returns INK_ERR_ARG with nothing launched unless C % 32 == 0, N % 4 == 0, stride is 1 or 2, every size is positive,
 * M fits an int32, and in / wt / out / residual / bias are 16-byte aligned.  Added without changing any entry point. */
int ink_conv3x3_f16(const void* in_f16, int32_t B, int32_t H, int32_t W, int32_t C, const void* wt_f16, int32_t N,
                    const float* bias, int32_t stride, int32_t relu_in, int32_t act, const float* residual, void* out,
                    int32_t out_f16, void* stream);

/* ------------------------------------------------------------------------
 * Layer assembly: the reference's inpainting stage around the diffusion model.  Binary images are
 * row-aligned bit planes [n, H, ceil(W / 64)] uint64 (bit b of word w = pixel 64 w + b), n <= 254, H, W <= 16383.
 * All results are integers and bit-exact against tests/layers_ref.py.  These entry points were added without changing
 * any existing one.
 *
 * ink_layers_otsu_planes: grey images uint8 [n, H, W] -> hist int32 [n, 256] of v (or 255 - v when invert != 0:
 * cv2.bitwise_not, fill_object_bg_mask.py:63-65), Otsu's threshold per image from the 256 counts in float64 as cv2
 * evaluates it (first maximum, strict >; fill_object_bg_mask.py:68-69) -> thresh int32 [n], planes = v > thresh. */
int ink_layers_otsu_planes(const void* gray_u8, int32_t n, int32_t H, int32_t W, int32_t invert, int32_t* hist,
                           int32_t* thresh, void* out_planes, void* stream);

/* cv2.dilate(planes, getStructuringElement(MORPH_ELLIPSE, (k, k)), iterations) for k = 3 (a cross) or 5 (rows of half
 * width 0, 2, 2, 2, 0); pixels outside the image never count (fill_object_bg_mask.py:71-73, 84).  tmp_planes: n planes. */
int ink_layers_dilate(const void* planes, int32_t n, int32_t H, int32_t W, int32_t kernel_size, int32_t iterations,
                      void* tmp_planes, void* out_planes, void* stream);

/* flags[p] = 1 iff plane p has a pixel in the first / last `band` rows or columns (fill_object_bg_mask.py:76-81). */
int ink_layers_border_band(const void* planes, int32_t n, int32_t H, int32_t W, int32_t band, int32_t* flags,
                           void* stream);

/* Component passes of get_mask.  mode 0: out = the silhouette ~flooded | planes, flooded = planes with the 4-connected
 * background component holding pixel (0, 0) set (cv2.floodFill from (0, 0), fill_object_bg_mask.py:91-93).  mode 1: out = planes with every hole filled
 * (fill_enclosed_regions, :4-20; a hole = a 4-connected background component that does not reach the image edge).
 * mode 2: fill_holes_not_touching_border (:22-47): a hole is filled, with everything it surrounds, when its box grown by
 * one stays off the image edge and its contour area is >= 50.  mode 3: the 8-connected component of largest contour
 * area with what it surrounds (:96-100; equal areas: the one whose first pixel comes last in raster order); its input
 * must hold no enclosed background, as a flooded silhouette does.  Contour area = polygon through the pixel centres of
 * the followed border, evaluated in closed form per 2x2 cell.  In mode 2 a small hole that surrounds foreground islands
 * may stay undecided: workspace[1] = number of such holes, workspace[2 + 8 k ..] = (plane, xmin, xmax, ymin, ymax,
 * twice the area of the hole's own cells, y and x of the hole's first pixel) for the first 64; they are left unfilled for the caller to resolve.
 * workspace[0] != 0: run table overflow (cannot happen with the queried size).  tmp_planes3: 3 n planes. */
int ink_layers_components_workspace_ints(int32_t n, int32_t H, int32_t W, int64_t* out_ints);
int ink_layers_components(const void* planes, int32_t n, int32_t H, int32_t W, int32_t mode, void* tmp_planes3,
                          int32_t* workspace, void* out_planes, void* stream);

/* cv2.distanceTransform(mask, DIST_L2, 5) as int32 16.16 fixed point [n, H, W] (weights 65536, 91750, 143976; zero
 * pixels inside the image only; 0x1fffffff where no zero pixel is reachable), then fill_object_bg_mask.py:103-107:
 * min_out[p] = smallest distance over the pixels of stroke plane p, shrink_out[p] = max(0, floor(float32(min) / 65536)
 * - safety_margin), out plane = shrink > 0 ? float32(dist) / 65536 >= shrink : mask.  Tiled relaxation repeated until
 * nothing below min + 1 pixel changes any more (full != 0: until nothing changes, so that `dist` is exact everywhere;
 * otherwise it is exact below that bound and an upper bound above it). */
int ink_layers_chamfer_workspace_ints(int32_t n, int32_t H, int32_t W, int64_t* out_ints);
int ink_layers_chamfer(const void* mask_planes, const void* stroke_planes, int32_t n, int32_t H, int32_t W,
                       int32_t safety_margin, int32_t full, int32_t* dist, int32_t* workspace, int32_t* min_out,
                       int32_t* shrink_out, void* out_planes, void* stream);

/* bbox int32 [n, 4] = mask_to_bbox (util.py:198-204: pixels > 127, INCLUSIVE maxima; (W, H, -1, -1) when empty);
 * overlap int32 [n, n]: [i, j] = 1 iff j < i and mask i (> 0) has a pixel inside box j sliced EXCLUSIVELY
 * (util.py:39-55, 148-157). */
int ink_layers_mask_tables(const void* masks_u8, int32_t n, int32_t H, int32_t W, int32_t* bbox, int32_t* overlap,
                           void* stream);

/* Per layer i (util.py:31-34, 94-104, 242-260): sketch_layers uint8 [n, H, W, 3] = the sketch's (B, G, R) inside mask i
 * and 255 outside; edit_masks uint8 [n, H, W] = 0 / 255: OR of bg_planes[j] over overlap[i, j], inside box i sliced
 * exclusively, minus mask i; debug uint8 [n, H, W, 3]: 255 on the mask, (0, 0, 255) on the edit mask. */
int ink_layers_assemble(const void* sketch_rgb_u8, const void* masks_u8, const void* bg_planes, const int32_t* bbox,
                        const int32_t* overlap, int32_t n, int32_t H, int32_t W, void* sketch_layers_u8,
                        void* edit_masks_u8, void* debug_u8, void* stream);

/* composite_original_sketch_onto_inpainted (util.py:101, 109-133): out = inpainted (R, G, B), replaced by the sketch
 * layer's pixel swapped back to (R, G, B) wherever one of its channels is < 255. */
int ink_layers_composite(const void* inpainted_rgb_u8, const void* sketch_layer_u8, int32_t H, int32_t W,
                         void* out_rgb_u8, void* stream);

/* cv2.imread(IMREAD_GRAYSCALE) of 8-bit RGB pixels [n, H, W, 3] -> [n, H, W] (fill_object_bg_mask.py:63, 136). */
int ink_layers_gray(const void* rgb_u8, int32_t n, int32_t H, int32_t W, void* gray_u8, void* stream);

/* create_rgba_with_background_mask (fill_object_bg_mask.py:141, 165-177): rgba uint8 [n, H, W, 4]: alpha = 255 where
 * grey < 240 or the background plane is set; colour = grey on those sketch pixels, else 255 on the background, else 0. */
int ink_layers_rgba(const void* gray_u8, const void* bg_planes, int32_t n, int32_t H, int32_t W, void* rgba_u8,
                    void* stream);

/* ------------------------------------------------------------------------
 * Inpainting: pre- and post-processing around the diffusion pipe (csrc/inpaint_ops.hip).  Images are
 * uint8 [H, W, 3] (R, G, B) and uint8 [H, W] on the device.  Every table of exponentials is computed on the host in
 * double precision, rounded once to the stated type and passed in; the kernels do + - x /, compares and conversions in
 * a fixed order and equal tests/inpaint_ref.py bit for bit.  The stencil entry points need H, W >= 3.  The stage's
 * Lanczos and bicubic resizes of images and masks are ink_resize_u8.
 * ------------------------------------------------------------------------ */

/* ImageEnhance.Contrast(image).enhance(factor) (inpaint_ControlNet.py:51-54): mean = round-half-up mean of Pillow's L
 * image from an integer sum kept on the device (sum_u64: 8 bytes of workspace), then
 * clip(float(mean) + factor * float(v - mean)) in f32, truncated. */
int ink_inp_contrast(const void* rgb_u8, int32_t H, int32_t W, float factor, void* sum_u64, void* out_rgb_u8,
                     void* stream);

/* cv2.bilateralFilter(rgb, 5, 50, 50) (inpaint_ControlNet.py:56-63): 13 taps of the radius-2 disc in row-major order,
 * reflect-101; tables: f32 [13 + 768] = the space weights of the taps, then the colour weights by |db| + |dg| + |dr|.
 * w = space * colour, sums in f32 in tap order, out = rint(sum * (1 / wsum)).  Not in place. */
int ink_inp_bilateral(const void* rgb_u8, int32_t H, int32_t W, const float* tables, void* out_rgb_u8, void* stream);

/* preprocess_mask (inpaint_ControlNet.py:67-75): dilate_iterations x cv2.dilate with a 3x3 block of ones, then (blur = 1)
 * cv2.GaussianBlur((3, 3), 0) = ([1 2 1]^T [1 2 1] . p + 8) >> 4 with a reflect-101 border.  tmp2_u8: 2 H W bytes.
 * At least one of the two steps must be asked for; not in place. */
int ink_inp_mask_prepare(const void* mask_u8, int32_t H, int32_t W, int32_t dilate_iterations, int32_t blur,
                         void* tmp2_u8, void* out_u8, void* stream);

/* make_inpaint_condition (inpaint_ControlNet.py:77-90): f32 [3, H, W] planar = v / 255, -1 where mask >= 128. */
int ink_inp_condition(const void* rgb_u8, const void* mask_u8, int32_t H, int32_t W, float* out_f32, void* stream);

/* _adaptive_threshold_blend, first half (inpaint_ControlNet.py:99-116): cv2 grey, its 11x11 Gaussian (sigma 2) in f32
 * with a replicated border (taps11: f32 [11]; rows left to right, columns from the centre outwards; tmp_f32 [H, W]),
 * rounded half-even to u8 = mean; thresh = 255 where grey > mean - 2, else 0; clean = 255 where thresh, else the pixel. */
int ink_inp_cleanup(const void* result_rgb_u8, int32_t H, int32_t W, const float* taps11, float* tmp_f32,
                    void* thresh_u8, void* clean_rgb_u8, void* stream);

/* _adaptive_threshold_blend, second half (inpaint_ControlNet.py:118-124) in f64: soft = clip(3x3 Gaussian (sigma 1) of
 * mask / 255, 0, 1), reflect-101, taps2: f64 [2] = centre and side weight, tmp_f64 [H, W];
 * out = trunc(clean * soft + original * (1 - soft)). */
int ink_inp_soft_blend(const void* clean_rgb_u8, const void* original_rgb_u8, const void* mask_u8, int32_t H, int32_t W,
                       const double* taps2, double* tmp_f64, void* out_rgb_u8, void* stream);

/* image.convert("L") (out_channels 1) and .convert("L").convert("RGB") (3) (inpaint_ControlNet.py:181,
 * inpaint_SDXL.py:32): (19595 R + 38470 G + 7471 B + 0x8000) >> 16. */
int ink_inp_luma(const void* rgb_u8, int32_t H, int32_t W, int32_t out_channels, void* out_u8, void* stream);

/* ImageFilter.UnsharpMask with a blur radius whose box radius is below 1 (inpaint_ControlNet.py:182: radius 0.5):
 * three box passes along x and three along y, (ww p + fw (p[-1] + p[+1]) + 2^23) >> 24 each stored as u8, replicated
 * border; then d = in - blur, out = clip(in + d * percent / 100) where |d| > threshold (C division), else in.
 * fw must be (2^24 - ww) / 2; tmp2_u8: 2 H W channels bytes. */
int ink_inp_unsharp(const void* img_u8, int32_t H, int32_t W, int32_t channels, uint32_t ww, uint32_t fw,
                    int32_t percent, int32_t threshold, void* tmp2_u8, void* out_u8, void* stream);

/* The RGBA layer of inpaint_single_layer.py:74-78: the result with alpha 255 where mask > 128, zeros elsewhere. */
int ink_inp_rgba_cut(const void* rgb_u8, const void* mask_u8, int32_t H, int32_t W, void* rgba_u8, void* stream);

/* ------------------------------------------------------------------------
 * Visualisation: the coloured sketch (csrc/visualize.hip).  The sketch is uint8 [H, W, 3] (R, G, B;
 * channels 3) or uint8 [H, W] (channels 1), grey = cv2.cvtColor(COLOR_RGB2GRAY) = (4899 R + 9617 G + 1868 B + 8192)
 * >> 14, or the single channel as it is (InkLayer/utils/visualization.py:79-85).  No pointer needs any alignment.
 * ------------------------------------------------------------------------ */

/* *gray_min = the smallest grey over the stroke pixels (grey < 250, visualization.py:92), 0x7f7f7f7f when the image has
 * none.  The word is reset on the stream before the kernel, so one buffer serves call after call; the host never
 * reads it: ink_vis_colour takes it from the device (max_stroke_opacity > 0.1, visualization.py:103-109, <=> it is
 * <= 229). */
int ink_vis_gray_min(const void* sketch_u8, int32_t channels, int32_t H, int32_t W, int32_t* gray_min, void* stream);

/* color_sketch_by_masks (visualization.py:63-167) as a table look-up: out uint8 [H, W, 3] = white where grey >= 250
 * (whatever the masks say), else tables[v][row][grey] with v = 0 when *gray_min <= 229 (power-law opacity, :109-118)
 * and 1 otherwise (:119-125), row = the index of the LAST mask holding the pixel (:131-150) or n for a stroke in no
 * mask (:152-165, 169-180).  by_label == 0: masks_or_label = uint8 [n, H, W], non-zero = inside (may be null when
 * n == 0); by_label != 0: uint8 [H, W], 0 = no mask, l = mask l - 1, a label above n counts as 0, n <= 255.
 * tables: uint8 [2, n + 1, 256, 3], built on the host (inklayer_amd/visualize.py::colour_tables). */
int ink_vis_colour(const void* sketch_u8, int32_t channels, const void* masks_or_label_u8, int32_t n, int32_t by_label,
                   const void* tables_u8, const int32_t* gray_min, int32_t H, int32_t W, void* out_rgb_u8,
                   void* stream);

/* ------------------------------------------------------------------------
 * Evaluation: counting predictions against a ground-truth label image (csrc/evaluate.hip).  All results are
 * integers and do not depend on the order of the pixels.  H W < 2^31; no pointer needs more than its element's
 * alignment (the byte images none).  Every output is cleared on the stream by the call itself.
 * ------------------------------------------------------------------------ */

/* The distinct values of a label image and each pixel's index among them.  labels: [H, W] of elem_size 1 (uint8), 2
 * (uint16) or 4 (int32) bytes, values 0 .. 65535.  workspace: 4096 uint32 (presence bitmap and its word prefix counts).
 * info[0] = U, the number of distinct values; info[1] != 0 when some value is negative or above 65535 (such a pixel gets
 * rank 0 and the results are not to be used).  values: the sorted table, the first min(U, values_cap) entries.
 * rank: uint16 [H, W], rank[y, x] = index of labels[y, x] in the table. */
int ink_eval_label_ranks(const void* labels, int32_t elem_size, int32_t H, int32_t W, uint32_t* workspace,
                         int32_t* values, int32_t values_cap, int32_t* info, uint16_t* rank, void* stream);

/* table int32 [n + 1, U]: table[i, u] = number of counted pixels inside prediction i whose rank is u; row n counts every
 * counted pixel (the ground-truth areas).  by_label == 0: pred_u8 = uint8 [n, H, W], non-zero = inside, masks may overlap
 * (may be null when n == 0); by_label != 0: uint8 [H, W], l = mask l - 1, 0 and labels above n = no mask, n <= 255.
 * 1 <= U <= 256; a pixel whose rank is >= U is left out.  stroke_only != 0: only pixels whose grey is below 250 count,
 * sketch_u8 = uint8 [H, W, 3] (R, G, B; channels 3, grey as ink_vis_gray_min) or [H, W] (channels 1); otherwise the
 * sketch is not read. */
int ink_eval_contingency(const void* pred_u8, int32_t n, int32_t by_label, const void* rank_u16, int32_t U,
                         const void* sketch_u8, int32_t channels, int32_t stroke_only, int32_t H, int32_t W,
                         int32_t* table, void* stream);

/* boxes int32 [U, 4]: xmin, ymin, xmax, ymax (inclusive) of the pixels of every rank; (INT_MAX, INT_MAX, -1, -1) for a
 * rank without pixels.  1 <= U <= 256. */
int ink_eval_label_boxes(const void* rank_u16, int32_t U, int32_t H, int32_t W, int32_t* boxes, void* stream);

/* out uint8 [H, W, 3] = colors[rank] with colors uint8 [U, 3] (white for a rank >= U): the ground-truth picture of
 * InkScenes/read_GT_mat_file.py:40-70.  1 <= U <= 256. */
int ink_eval_paint_labels(const void* rank_u16, const void* colors_u8, int32_t U, int32_t H, int32_t W, void* out_rgb_u8,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INKLAYER_HIP_H */

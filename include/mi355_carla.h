/* mi355_carla.h — C ABI of libmi355_carla.so: the MI355X (gfx950 / CDNA4) implementation of the
 * ConvVAE + PPO hot path of bitsauce/Carla-ppo.
 *
 * The reference has no FFI layer (pure Python on TensorFlow 1.13); the boundary it exposes is the Python class
 * surface of vae/models.py and ppo.py.  Those classes are re-implemented in carla-ppo_amd/{vae/models.py,ppo.py,utils.py}
 * and call ONLY the functions below through ctypes.  Each entry cites the reference op(s) it replaces
 * (file:line relative to the reference checkout).
 *
 * Conventions
 *   - plain C; raw DEVICE pointers (from torch tensors' data_ptr()) and sizes; no torch types.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); every call is asynchronous on it.
 *   - return value: 0 = ok, negative = error (MI_ERR_*); message via mi_last_error() (thread local).
 *   - no allocation inside the library: all buffers/workspaces are passed in (sizes via *_floats / *_bytes queries).
 *   - dtype: 0 = fp32 storage + v_mfma_f32_32x32x2_f32 (parity mode), 1 = bf16 storage + v_mfma_f32_32x32x16_bf16
 *     (throughput mode; fp32 accumulate, fp32 master weights / grads / optimiser state), 2 = SPLIT storage ("bf16x3" precision): every
 *     activation / weight element is 4 bytes = two bf16 halves hi + lo of one value (hi = bf16(x), lo = bf16(x - hi); word = hi << 16 | lo),
 *     products formed on the bf16 MFMA pipe as a.b + a.swap16(b) (all four partial products, fp32 accumulate): 16-17 significand bits per
 *     operand at a quarter of the exact-fp32 MFMA time -- the fast mode that meets the 1e-4 tolerance.  Same sizes / alignments as dtype 0.
 *   - layouts are TensorFlow's: activations NHWC, conv kernels HWIO [kh,kw,in,out], transposed-conv kernels
 *     [kh,kw,out,in], dense kernels [in,out].  All convolutions are stride 2, VALID.
 *
 * The binding is generated from THIS file: carla-ppo_amd/mi355/lib.py parses the prototypes below.
 */
#ifndef MI355_CARLA_H
#define MI355_CARLA_H

#ifdef __cplusplus
extern "C" {
#endif

#define MI_F32 0
#define MI_BF16 1
#define MI_BF16X3 2

#define MI_OK 0
#define MI_ERR_ARG (-1)
#define MI_ERR_SHAPE (-2)
#define MI_ERR_LAUNCH (-3)
#define MI_ERR_STATE (-4)


/* ---- engine descriptors (all 4-byte fields; mirrored as ctypes.Structure in carla-ppo_amd/mi355/lib.py) ---- */
typedef struct MiVaeDesc {
    int dtype;          /* MI_F32 | MI_BF16 | MI_BF16X3 */
    int max_batch;      /* largest per-GPU minibatch the workspace is sized for */
    int ih, iw, cin;    /* source frame shape (80,160,3) — NHWC */
    int ct;             /* target depth: 3 (rgb) or 1 (segmentation) */
    int z_dim;
    int loss_kind;      /* 0 bce_loss, 1 bce_loss_v2, 2 mse_loss (vae/models.py:11-22) */
    float beta;
    float kl_tolerance;
    int inference_only; /* != 0: no backward pass will ever run on this engine (VAE(training=False): rollout / evaluation / encode): the workspace carries the regions of
                         * forward passes only -- no gradient tensors, ReLU bit words or filter-gradient scratch, and no conv1 activation where conv1 + conv2 run as the fused
                         * encoder head (bf16, B = 512: 298 MB instead of 808); mi_vae_create then wants grads == NULL, and mi_vae_forward(want_grad = 1) is a forward without
                         * gradient.  0 (the zero-initialised default): a training engine */
} MiVaeDesc;

/* MlpVAE (vae/models.py:271-299): dense encoder / decoder around the same latent block; up to MI_MLP_MAX_HIDDEN hidden layers per side */
#define MI_MLP_MAX_HIDDEN 4
typedef struct MiMlpVaeDesc {
    int dtype;          /* MI_F32 | MI_BF16 */
    int max_batch;
    int source_size;    /* prod(source_shape), e.g. 80*160*3 = 38400 */
    int target_size;    /* prod(target_shape) */
    int z_dim;
    int n_enc, n_dec;   /* hidden layers: encoder_sizes (512, 256) -> 2, decoder_sizes (256, 512) -> 2; the output layer to target_size is implied */
    int enc[MI_MLP_MAX_HIDDEN];
    int dec[MI_MLP_MAX_HIDDEN];
    int loss_kind;      /* 0 bce_loss, 1 bce_loss_v2, 2 mse_loss */
    int with_optimizer; /* 0: inference-only engine (no gradient buffers in the workspace) */
    float beta;
    float kl_tolerance;
} MiMlpVaeDesc;

typedef struct MiPpoDesc {
    int max_batch;
    int input_dim;      /* z_dim + measurements = 67 (train.py:85) */
    int num_actions;    /* 2 */
    int h1, h2;         /* (500, 300) for both pi and V trunks (ppo.py:18) */
    float clip_eps;     /* epsilon */
    float value_scale;
    float entropy_scale;
} MiPpoDesc;

/* ---- library ---- */
const char* mi_last_error(void);
int mi_abi_version(void);
int mi_device_info(int device, int* cu_count, int* wave_size, char* arch, int arch_len);
/* CRC-32C of a HOST buffer (running value in, 0 to start): the checksum of the reference's TensorFlow bundle checkpoints
 * (tf.train.Saver files written / read by vae/models.py:154,172-186 and ppo.py:184,202-216); used by mi355/tf_bundle.py.  Returns the crc. */
unsigned int mi_crc32c(unsigned int crc, const void* data, long long n);
/* Box calibration (round 5; SURVEY 8d "confirm on the box"; no reference counterpart): what THIS GPU sustains right now on the two resources the rooflines are priced
 * against -- bench.py prints it as "box" next to every datasheet fraction.  scratch: device buffer, >= 64 MiB, ideally mi_device_probe_scratch_bytes() (6 x the
 * Infinity Cache); millis: length of each of the three MFMA launches (1..50).  SYNCHRONOUS (HIP events).  out8: 0 sustained v_mfma_f32_32x32x16_bf16 rate in TFLOP/s
 * (mean of launches 2 and 3), 1 shader clock during them in MHz (s_memtime / s_memrealtime), 2 / 3 the same for the FIRST launch (clocks as the caller left them),
 * 4 HBM streaming read TB/s, 5 HBM copy TB/s (read + written bytes), 6 compute units, 7 bytes the HBM probes walked. */
long long mi_device_probe_scratch_bytes(void);
int mi_device_probe(void* stream, void* scratch, long long scratch_bytes, int millis, float* out8);
/* Kernel-selection knobs (process-global, not part of the reference surface; defaults come from the environment variables of
 * the same meaning).  key 0: gemm2 LDS-DMA tiles on/off (MI355_GEMM2); key 1: minimum block count for the raw-staged
 * tapconv kernel, -1 = never (MI355_TAPCONV / MI355_TAPCONV_MINBLOCKS); key 2: debug, drop the wgrad_kernel atomics;
 * key 3: raw-staged bf16 weight-gradient kernel on/off (MI355_TAPWGRAD); key 4: narrow-layer kernels on/off (MI355_NARROW);
 * key 5: tapconv tile (0 auto, 1 = 256 positions / 1 block per CU, 2 = 128 positions / 2 blocks per CU);
 * key 6: tapconv epilogue (1 = registers -> 16-byte stores through a half-wave swap, 0 = LDS-staged coalesced stores);
 * key 7: tapwgrad wave layout for 2x2-tap layers (1 = wave per (tap, position half), 0 = wave per (tap, output tile));
 * key 8: tapconv grid, EXPERIMENTAL (0 = one block per tile, 1 = persistent blocks walking contiguous tile ranges, N > 1 = at most N
 * of them per output column; MI355_TAP_PERSIST);
 * key 9: tapwgrad target block count (position splits x block columns; default 256 = one block per CU); key 10: waves per block of
 * the narrow filter-gradient kernel (4 | 8 | 12); key 11: target block count of the dense filter gradients;
 * key 12: tapconv ReluGrad-mask prefetch in the last main-loop step on/off;
 * key 13: register-weight kernel of the thin gather-form layers (rwconv.hip: deconv3 fwd, conv2 dgrad): 0 off, 1 auto (grids that fill the
 * chip), 2 whenever the layer is eligible (MI355_RWCONV); key 14: the column-walk filter-gradient kernel of deconv3 on/off;
 * key 15: register-weight kernel of the conv-form layers (rwconv.hip): 0 off, 1 deconv3 dgrad (32 -> 64 channels, k = 5), 2 also conv2 fwd (k = 4),
 * 3 also the 64 -> 128 channel k = 4 shape, conv3 fwd / deconv2 dgrad (default; MI355_RWCONV_CONV); subject to key 13's off / auto / always; key 16: persistent blocks per XCD of the
 * register-weight kernels, 0 = as many as stay resident (tests use 1: every block then walks several chunks); key 22: the LDS-free one-wave-per-tile dense filter
 * gradient of round 5 (csrc/dwgs_tile.hpp; MI355_DWGS) on / off; key 23 (debug): ablation mask of the fused encoder-head forward kernel's timing instantiation
 * (tools/enc12_ablate.py; any bit set = wrong results; 0 = the product kernel).  Returns the previous value. */
int mi_set_tuning(int key, int value);
/* Per calling thread, default 0 (returns the previous setting).  != 0: a raw-staged filter gradient (mi_conv2d_nhwc_wgrad_ws / mi_deconv2d_nhwc_wgrad_ws on bf16 tensors) whose
 * positions fit ONE split sums the partial rows of its bias gradient through the first bytes of the caller's scratch in a fixed order instead of fp32 atomics: two runs are
 * bitwise equal.  The switch of layer-op calls from outside: the ConvVAE engine's backward pass asks for the same in its own calls and leaves it alone; 0 leaves a scratch that holds no slabs untouched. */
int mi_tapwgrad_bias_rows(int on);
/* debug only: s_memtime stamps of the tapconv kernel (32 int64 per wave per block) into a caller-provided device buffer; NULL = off */
int mi_debug_set_trace(void* dev_ptr, int capacity_entries);

/* ---- convolution family (implicit-GEMM on MFMA, LDS-staged tiles) ---- */
/* tf.layers.conv2d k x k, s2, VALID + BiasAdd + Relu — vae/models.py:250-253.  x may be frames gathered through frame_idx: x_is_f32 = 1 fp32
 * frames, 2 = raw uint8 camera frames (value k / 255, the host preprocessing of vae/train_vae.py:15-18 done in registers; bf16 narrow-layer kernel only). */
int mi_conv2d_nhwc_fwd(void* stream, int dtype, const void* x, const int* frame_idx, int x_is_f32, int B, int IH, int IW, int Cin, const void* w, int w_transposed, const float* bias, int KH, int KW, int Cout, int relu, void* out);
/* ReLU bit words (bf16 engine): a forward kernel can also write, per output pixel and group of 16 channels, one uint32 whose bit i (i < 8) says
 * "channel 16 j + 2 i > 0" and bit 16 + i "channel 16 j + 2 i + 1 > 0"; the ReluGrad of the next layer's input gradient then reads those words
 * (1/16 of the bytes) instead of the activation tensor.  relu_bits: [B*OH*OW][Cout/16] uint32, *wrote_bits = 1 when the kernel produced them. */
int mi_conv2d_nhwc_fwd_bits(void* stream, int dtype, const void* x, const int* frame_idx, int x_is_f32, int B, int IH, int IW, int Cin, const void* w, int w_transposed, const float* bias, int KH, int KW, int Cout, int relu, void* out, void* relu_bits, int* wrote_bits);
int mi_conv2d_nhwc_dgrad_bits(void* stream, int dtype, const void* dy, int B, int OH, int OW, int Cout, const void* w, int KH, int KW, int Cin, int IH, int IW, const void* mask, const void* mask_bits, void* dx);
int mi_deconv2d_nhwc_fwd_bits(void* stream, int dtype, const void* x, int B, int IH, int IW, int Cin, const void* w, const float* bias, int KH, int KW, int Cout, int relu, void* out, void* relu_bits, int* wrote_bits);
int mi_deconv2d_nhwc_dgrad_bits(void* stream, int dtype, const void* dy, int B, int OH, int OW, int Cout, const void* w, int w_transposed, int KH, int KW, int Cin, const void* mask, const void* mask_bits, void* dx);
/* Conv2DBackpropInput (+ fused ReluGrad of the layer below through `mask`) — backward of vae/models.py:250-253 */
int mi_conv2d_nhwc_dgrad(void* stream, int dtype, const void* dy, int B, int OH, int OW, int Cout, const void* w, int KH, int KW, int Cin, int IH, int IW, const void* mask, void* dx);
/* Conv2DBackpropFilter: dw += im2col(x)^T dy.  NON-DETERMINISTIC summation order: the position splits meet in fp32 atomics (two runs may differ in the last bits);
 * the _ws form below (caller scratch) is the deterministic one and the only one the engines use */
int mi_conv2d_nhwc_wgrad(void* stream, int dtype, const void* x, const int* frame_idx, int x_is_f32, int B, int IH, int IW, int Cin, const void* dy, int KH, int KW, int Cout, float* dw);
/* same, with caller scratch for the split reduction (every kernel generation and storage type: per-split partial sums added in a fixed order, no atomics,
 * bitwise reproducible; 64 MiB covers every layer of the model at any batch size; may be NULL) and, when dbias != NULL,
 * the BiasAddGrad of the same layer (dbias[n] += sum dy) fused into the kernel where it is eligible, else run as mi_colsum */
int mi_conv2d_nhwc_wgrad_ws(void* stream, int dtype, const void* x, const int* frame_idx, int x_is_f32, int B, int IH, int IW, int Cin, const void* dy, int KH, int KW, int Cout, float* dw, void* scratch, long long scratch_bytes, float* dbias);
/* tf.layers.conv2d_transpose k x k, s2, VALID + BiasAdd (+ Relu) — vae/models.py:261-264 */
int mi_deconv2d_nhwc_fwd(void* stream, int dtype, const void* x, int B, int IH, int IW, int Cin, const void* w, const float* bias, int KH, int KW, int Cout, int relu, void* out);
/* conv2d_transpose into the 1- or 3-channel logits WITH the reconstruction loss of vae/models.py:11-22,123-128 fused into its epilogue
 * (labels: fp32 target frames [*, OH*OW*Cout], optional gather through frame_idx): writes logits, dlogits (NULL = loss only), one loss
 * partial per block into loss_partial[] and 4 floats of per-channel dlogits sums per block into bias_partial[].  *n_partial = number of
 * blocks written, or 0 when the layer is not eligible for the fused kernel (nothing was launched: call the two ops separately). */
int mi_deconv2d_nhwc_fwd_bce(void* stream, int dtype, const void* x, int B, int IH, int IW, int Cin, const void* w, const float* bias, int KH, int KW, int Cout, void* logits, const float* labels, const int* frame_idx, long long label_stride, int loss_kind, float inv_batch, void* dlogits, float* loss_partial, float* bias_partial, int partial_capacity, int* n_partial);
/* same; labels_u8 != 0: labels are raw uint8 frames (label_stride in bytes), normalised to exactly float32(k) / float32(255) in registers; logits == NULL: the logits are not stored */
int mi_deconv2d_nhwc_fwd_bce_u8(void* stream, int dtype, const void* x, int B, int IH, int IW, int Cin, const void* w, const float* bias, int KH, int KW, int Cout, void* logits, const void* labels_any, int labels_u8, const int* frame_idx, long long label_stride, int loss_kind, float inv_batch, void* dlogits, float* loss_partial, float* bias_partial, int partial_capacity, int* n_partial);
/* The decoder tail of a TRAINING step in one launch (round 3): conv2d_transpose into the 3-channel logits (vae/models.py:264), the reconstruction loss of
 * vae/models.py:11-22,123-128, and both gradients of that layer behind tf.gradients (vae/models.py:142: Conv2D of dlogits + ReluGrad -> dx, the gradient
 * wrt the previous layer's pre-activation; Conv2DBackpropFilter -> dw +=) -- logits and dlogits never leave the chip.  x: [B,IH,IW,32] (post-ReLU: it is
 * its own ReluGrad mask); w: [kh,kw,out,in]; w_t: the K-contiguous copy [in][kh*kw*out]; labels as mi_deconv2d_nhwc_fwd_bce_u8; loss_partial[] /
 * bias_partial[][4] per block as there; scratch >= mi_deconv2d_tail_blocks() * 6144 bytes.  *n_partial = blocks written, or 0 when the layer is not
 * eligible (bf16 storage, 32 -> 3 channels, k = 4 only; nothing was launched: use the separate ops). */
int mi_deconv2d_tail_blocks(void);
int mi_deconv2d_tail_fused(void* stream, int dtype, const void* x, int B, int IH, int IW, int Cin, const void* w, const void* w_t, const float* bias, int KH, int KW, int Cout, const void* labels, int labels_u8, const int* frame_idx, long long label_stride, int loss_kind, float inv_batch, void* dx, float* dw, float* loss_partial, float* bias_partial, int partial_capacity, int* n_partial, void* scratch, long long scratch_bytes, int reduce_now);
/* reduce_now = 0 above leaves the per-block filter-gradient partial sums in scratch; this adds them to dw (anywhere behind that launch on the same
 * stream order and in front of the optimiser step) */
int mi_deconv2d_tail_reduce(void* stream, const void* scratch, int n_partial, float* dw);
/* The encoder head of a backward pass in ONE launch (csrc/enchead_tile.hpp; replaces Conv2DBackpropInput of conv2 + Conv2DBackpropFilter / BiasAddGrad of conv1,
 * vae/models.py:250-251 behind :142): frames [*, FH, FW, 3] (frames_fmt 1 = fp32, 2 = uint8 camera bytes; optionally gathered through frame_idx) -conv1 k4 s2-> 32 ch
 * -conv2 k4 s2-> 64 ch; dy2 = gradient wrt conv2's pre-activation [B, OH, OW, 64], w2 = conv2's kernel [4][4][32][64], bits_act1 = ReLU bit words of conv1's output.
 * dw1 [4][4][3][32] += , db1 [32] += .  The gradient of conv1's output is never written.  *n_blocks = 0: not eligible (nothing launched; call
 * mi_conv2d_nhwc_dgrad_bits and mi_conv2d_nhwc_wgrad_ws).  scratch: >= mi_conv2d_head_bwd_blocks() * 8320 bytes. */
int mi_conv2d_head_bwd_blocks(void);
int mi_conv2d_head_bwd_fused(void* stream, int dtype, const void* frames, int frames_fmt, const int* frame_idx, int B, int FH, int FW, const void* dy2, const void* w2, const void* bits_act1, float* dw1, float* db1, void* scratch, long long scratch_bytes, int* n_blocks);
/* The encoder head of a FORWARD pass in ONE launch (round 5, csrc/enc12_tile.hpp; replaces the two tf.layers.conv2d of vae/models.py:250-251): frames
 * [*, 80, 160, 3] as uint8 camera bytes (frames_fmt 2) or float32 (1), optionally gathered through frame_idx, -conv1 k4 s2 + bias + ReLU-> act1 [B, 39, 79, 32] kept in LDS -conv2 k4 s2 + bias + ReLU-> act2
 * [B, 18, 38, 64].  w1_t / w2_t: the K-contiguous kernel copies [32][48] / [64][512] (mi_transpose_weights).  act1 and (relu_bits1 != NULL) its ReLU bit words are still
 * written, bit for bit as mi_conv2d_nhwc_fwd_bits writes them (the backward pass reads them); act2 = conv2 of that activation.  act1 == NULL: the INFERENCE form (a forward
 * pass with no backward pass behind it) -- conv1's activation never leaves LDS, act2 is bit for bit what the training form writes; relu_bits1 must then be NULL too
 * (MI_ERR_ARG otherwise).  *launched = 0: not eligible (bf16 storage, this geometry only; nothing was launched: call mi_conv2d_nhwc_fwd_bits and mi_conv2d_nhwc_fwd). */
int mi_conv2d_enc12_fwd(void* stream, int dtype, const void* frames, int frames_fmt, const int* frame_idx, int B, int FH, int FW, const void* w1_t, const float* b1, const void* w2_t, const float* b2, void* act1, void* relu_bits1, void* act2, int* launched);
/* The four SMALL-GRID layers of the ConvVAE on the activation-resident kernels (round 4, csrc/ares_tile.hpp): a block keeps the whole inputs of a group of frames
 * in LDS and streams fragment-ordered weights through registers.  form 0 (conv form, k4 s2, [B,8,18,128] -> [B,3,8,256]): conv4 forward (vae/models.py:253) and
 * deconv1's input gradient (Conv2D of dy behind :142); form 1 (gather form, [B,3,8,256] -> [B,8,18,128]): deconv1 forward (:261) and conv4's input gradient
 * (Conv2DBackpropInput).  mi_ares_pack_weights rewrites a [4][4][128][256] fp32 master kernel into the form's fragment order (mi_ares_weight_bytes() of bf16;
 * once per optimiser step); mi_ares_conv: out = mask(relu?(op(x) + bias)), *launched = 0 when the call is not eligible (bf16 storage and this geometry only;
 * nothing was launched: use the general ops above / below). */
long long mi_ares_weight_bytes(void);
int mi_ares_pack_weights(void* stream, int form, const float* w_fp32, void* wf_out);
/* the four copies the VAE engine keeps, in one launch: wf0 conv4 forward (form 0 of conv4's kernel), wf1 conv4 input gradient (form 1 of it), wf2 deconv1 forward (form 1 of
 * deconv1's kernel), wf3 deconv1 input gradient (form 0 of it) */
int mi_ares_pack_weights4(void* stream, const float* conv4_w, const float* deconv1_w, void* wf0, void* wf1, void* wf2, void* wf3);
/* form 2 of mi_ares_conv / mi_ares_pack_weights: the MID-layer gather form, [B,8,18,128] -> [B,18,38,64] (deconv2 forward, vae/models.py:262, and conv3's input
 * gradient): w is [4][4][64][128] read as [kh][kw][n][c] (deconv2's [kh,kw,out,in] kernel, or conv3's HWIO kernel); its fragment copy is 256 KB.
 * mi_ares_pack_weights6 = mi_ares_pack_weights4 + those two copies (conv3_w -> wf4, deconv2_w -> wf5; either pair may be NULL) in one launch. */
int mi_ares_pack_weights6(void* stream, const float* conv4_w, const float* deconv1_w, const float* conv3_w, const float* deconv2_w, void* wf0, void* wf1, void* wf2, void* wf3, void* wf4, void* wf5);
/* round 6: ... plus the conv-form copies of the same two mid-layer kernels for the register-weight kernel (form 3: the order rwconv_conv_kernel<4, 2> loads its 64 weight fragments in, 256 KB
 * each): conv3_w -> wf6 (conv3 forward, vae/models.py:252), deconv2_w -> wf7 (deconv2's input gradient, Conv2D of dy behind :262).  NULL pairs are skipped. */
int mi_ares_pack_weights8(void* stream, const float* conv4_w, const float* deconv1_w, const float* conv3_w, const float* deconv2_w, void* wf0, void* wf1, void* wf2, void* wf3, void* wf4, void* wf5, void* wf6, void* wf7);
/* Announces `wf` for the calling thread's NEXT call of mi_conv2d_nhwc_fwd[_bits], mi_deconv2d_nhwc_fwd[_bits], mi_deconv2d_nhwc_dgrad[_bits] or mi_conv2d_enc12_fwd.  That call
 * always clears the announcement, whether it launches anything or not; if it runs the register-weight kernel below, that kernel reads its weights from `wf` instead of the
 * K-contiguous copy: 1 KB contiguous per wave load in the kernel's prologue (the K-contiguous copy gives 16 B per lane at a 1-2 KB lane stride).  Which form `wf` must hold
 * follows from the call:
 *   form 3 (above)  mi_conv2d_nhwc_fwd[_bits] of a 64 -> 128 channel k = 4 layer (conv3), mi_deconv2d_nhwc_dgrad[_bits] of a 128 -> 64 channel one (deconv2)
 *   form 4          mi_deconv2d_nhwc_fwd of the k = 5, 64 -> 32 channel layer (deconv3, vae/models.py:263): mi_ares_pack_weights(form 4) of its [5][5][32][64] kernel,
 *                   144 fragments of 1 KB ordered (output-parity class, tap of the 3 x 3 class window, 16-channel K step); fragments of taps outside the 5 x 5 kernel are never read
 *   form 6          mi_deconv2d_nhwc_dgrad[_bits] of the k = 5, 32 -> 64 channel layer (deconv3's input gradient): mi_ares_pack_weights(form 6) of deconv3's kernel read as [800][64],
 *                   2 x 50 fragments (32-wide output tile, the 50 live (tap, k-step) pairs of the 3 x 3 slot taps in the prologue's order)
 *   form 5          mi_conv2d_enc12_fwd: conv2's [4][4][32][64] HWIO kernel (vae/models.py:251), mi_ares_pack_weights(form 5), 64 fragments (32-wide output half, K step)
 * NULL clears.  Same values in the same registers: results are bit-identical either way. */
int mi_rwconv_next_weights_fragment_ordered(const void* wf);
int mi_ares_conv(void* stream, int dtype, int form, const void* x, int B, const void* wf, const float* bias, int relu, const void* mask, void* out, int* launched);
/* backward of conv2d_transpose wrt its input (= a plain s2 conv of dy) with fused ReluGrad mask */
int mi_deconv2d_nhwc_dgrad(void* stream, int dtype, const void* dy, int B, int OH, int OW, int Cout, const void* w, int w_transposed, int KH, int KW, int Cin, const void* mask, void* dx);
/* backward of conv2d_transpose wrt its kernel: dw[kh,kw,co,ci] += im2col(dy)^T x.  The form WITHOUT scratch is NON-DETERMINISTIC (fp32 atomics across the position
 * splits); the _ws form is the deterministic one (per-split partial sums added in a fixed order) */
int mi_deconv2d_nhwc_wgrad(void* stream, int dtype, const void* dy, int B, int OH, int OW, int Cout, const void* x, int KH, int KW, int Cin, float* dw);
int mi_deconv2d_nhwc_wgrad_ws(void* stream, int dtype, const void* dy, int B, int OH, int OW, int Cout, const void* x, int KH, int KW, int Cin, float* dw, void* scratch, long long scratch_bytes, float* dbias);
/* tf.layers.dense (MatMul + BiasAdd + Relu) and its input gradient — vae/models.py:97-98,259; utils.py:25-28; ppo.py:43-55.
 * w_layout 0: W[K,N]; 1: W[N,K] (x * W^T).  nsplit > 1: split-K raw fp32 slabs out[nsplit][M][N]. */
int mi_gemm_bias_act(void* stream, int dtype, const void* a, int M, int K, const void* w, int w_layout, int N, const float* bias, int relu, const void* mask, void* out, int out_f32, int nsplit);
/* the finishing pass of a split-K dense layer: out[m,n] = mask(act(sum_s slabs[s][m][n] + bias[n])) -- the bias / ReLU / ReluGrad epilogue mi_gemm_bias_act
 * cannot apply to raw slabs (MlpVAE, vae/models.py:271-299: the 38400-long reductions of its first layer and of its last layer's input gradient) */
int mi_splitk_finish(void* stream, int dtype, const float* slabs, int nsplit, int M, int N, const float* bias, int relu, const void* mask, void* out, int out_f32);
/* dense kernel gradient dw[K,N] += a^T dy (MatMul's weight gradient behind tf.gradients -- vae/models.py:142, ppo.py:143-144).  NON-DETERMINISTIC summation order: the row splits meet in fp32 atomics; use the _ws forms below */
int mi_gemm_wgrad(void* stream, int dtype, const void* a, const void* dy, int M, int K, int N, float* dw);
/* same with caller scratch (>= mi_gemm_wgrad_scratch_bytes; may be NULL = the form above): every row split stores its partial sums and one pass adds them to dw
 * in a fixed order -- two runs are bitwise equal (round 4; the parity engines use only this form) */
long long mi_gemm_wgrad_scratch_bytes(int dtype, int M, int K, int N);
int mi_gemm_wgrad_ws(void* stream, int dtype, const void* a, const void* dy, int M, int K, int N, float* dw, void* scratch, long long scratch_bytes);
/* same + the layer's BiasAddGrad in the same launch: dbias[n] += sum_m dy[m,n] (a column of ones appended to `a` inside the kernel's loader; dbias may be NULL) */
int mi_gemm_wgrad_bias_ws(void* stream, int dtype, const void* a, const void* dy, int M, int K, int N, float* dw, float* dbias, void* scratch, long long scratch_bytes);
/* round 6: TWO such gradients as ONE launch -- exactly what the two single calls compute (problem 0, then problem 1), bit for bit: the ConvVAE's backward pass ends with dense1's
 * (vae/models.py:259) and the heads' (:97-98) filter + bias gradients, two ~190-block grids of a latency-bound kernel back to back on the caller's stream.  Pairs the one-launch form
 * does not cover (other dtypes / shapes) run as the two single calls. */
int mi_gemm_wgrad_bias_pair_ws(void* stream, int dtype, const void* a0, const void* dy0, int M0, int K0, int N0, float* dw0, float* dbias0, void* scratch0, long long scratch_bytes0,
                               const void* a1, const void* dy1, int M1, int K1, int N1, float* dw1, float* dbias1, void* scratch1, long long scratch_bytes1);
/* same; overwrite != 0: dw (and dbias) = the gradient instead of += (plain stores / the storing form of the ordered sum): the gradient buffer need not be zeroed and no
 * element is touched by an atomic.  Row splits then NEED the scratch (MI_ERR_ARG otherwise). */
int mi_gemm_wgrad_bias_set(void* stream, int dtype, const void* a, const void* dy, int M, int K, int N, float* dw, float* dbias, void* scratch, long long scratch_bytes, int overwrite);

/* ---- VAE elementwise / reduction kernels ---- */
/* Normal(mean, exp(.5 lv)).sample + kl_divergence — vae/models.py:7-9,101-105 (eps injected; TF RNG is unseeded) */
int mi_vae_reparam_kl_fwd(void* stream, int dtype, const float* heads, int nsplit, const float* bias_mean, const float* bias_lv, const float* eps, int sample, int B, int Z, float* mean, float* logvar, void* z, float* kl_row);
/* same with the engine-side noise source: eps == NULL and sample != 0 draws N(0,1) from the Philox4x32-10 stream in rng_state (device, 4 x uint64:
 * seed, next element offset, 2 words of kernel bookkeeping) and stores the draw in eps_out [B,Z] for the backward pass — tfp Normal.sample, vae/models.py:101-105 */
int mi_vae_reparam_kl_fwd_rng(void* stream, int dtype, const float* heads, int nsplit, const float* bias_mean, const float* bias_lv, const float* eps, int sample, int B, int Z, float* mean, float* logvar, void* z, float* kl_row, unsigned long long* rng_state, float* eps_out);
/* out[i] = N(0,1) element (offset + i) of Philox stream `seed` (exploration noise of ppo.py:58-60, tests) */
int mi_normal_philox(void* stream, unsigned long long seed, unsigned long long offset, float* out, long long n);
/* the two halves behind ONE entry point, as SURVEY 8b names it: heads != NULL runs the forward (as mi_vae_reparam_kl_fwd), dz_slabs != NULL runs the backward (as
 * mi_vae_reparam_kl_bwd, on the mean / logvar / kl_row the forward half of this or an earlier call left in the same buffers); both: forward, then backward */
int mi_vae_reparam_kl_fwd_bwd(void* stream, int dtype, const float* heads, int nsplit, const float* bias_mean, const float* bias_lv, const float* eps, int sample, int B, int Z, float* mean, float* logvar, void* z, float* kl_row, const float* dz_slabs, int dz_nsplit, float beta, float kl_floor, float inv_batch, void* dheads);
int mi_vae_reparam_kl_bwd(void* stream, int dtype, const float* dz_slabs, int nsplit, const float* mean, const float* logvar, const float* eps, const float* kl_row, float beta, float kl_floor, float inv_batch, int B, int Z, void* dheads);
/* bce_loss / bce_loss_v2 / mse_loss + reduce_sum(axis=1) + gradient — vae/models.py:11-22,123-128 */
int mi_recon_loss_chunks(int P);
int mi_bce_logits_fwd_bwd(void* stream, int dtype, const void* logits, const float* labels, const int* frame_idx, long long label_stride, int B, int P, int loss_kind, float inv_batch, void* dlogits, float* partial);
/* same + the BiasAddGrad of the layer that produced the logits: dbias[c] += sum of the stored dlogits of channel c (channels = 1..3) */
/* same with the labels as raw uint8 camera bytes (label_stride in values = bytes): float32(k) / float32(255) formed exactly in registers */
int mi_bce_logits_fwd_bwd_u8(void* stream, int dtype, const void* logits, const unsigned char* labels, const int* frame_idx, long long label_stride, int B, int P, int loss_kind, float inv_batch, void* dlogits, float* partial);
int mi_bce_logits_fwd_bwd_bias(void* stream, int dtype, const void* logits, const float* labels, const int* frame_idx, long long label_stride, int B, int P, int loss_kind, float inv_batch, void* dlogits, float* partial, int channels, float* dbias);
/* reduce_mean over the batch, kl_tolerance clamp, tf.metrics.mean accumulators — vae/models.py:124-137,145-146 */
int mi_vae_finalize_losses(void* stream, const float* partial, int nchunks, const float* kl_row, float kl_floor, int B, float inv_batch, float* out2, float* metrics3, float metric_weight);
/* same over a flat list of loss partial sums; optionally folds per-block channel sums [n][4] of a fused loss pass into dbias */
int mi_vae_finalize_losses_flat(void* stream, const float* partial, int n_partial, const float* kl_row, float kl_floor, int B, float inv_batch, float* out2, float* metrics3, float metric_weight, const float* bias_partial, int n_bias_partial, int channels, float* dbias);
/* tf.train.AdamOptimizer ApplyAdam x N fused over one flat buffer — vae/models.py:141-142, ppo.py:143-144 */
int mi_adam_tf_flat(void* stream, float* param, float* m, float* v, float* grad, long long n, float alpha, float beta1, float beta2, float epsilon, void* bf16_shadow, int clear_grad);
/* same; alpha_dev != NULL: the step size is read from device memory (a captured step is replayed with a new value) */
int mi_adam_tf_flat_dev(void* stream, float* param, float* m, float* v, float* grad, long long n, float alpha, const float* alpha_dev, float beta1, float beta2, float epsilon, void* bf16_shadow, int clear_grad);
/* same; the shadow weight copy the MFMA kernels read is of storage type shadow_dtype: MI_BF16 (2 bytes per weight) or MI_BF16X3 (split, 4 bytes) */
int mi_adam_tf_flat_shadow(void* stream, float* param, float* m, float* v, float* grad, long long n, float alpha, const float* alpha_dev, float beta1, float beta2, float epsilon, void* shadow, int shadow_dtype, int clear_grad);
/* TF ApplyAdam (tf.train.AdamOptimizer.minimize, vae/models.py:140-142) over the flat buffer [0, n) that ALSO refreshes both weight copies of the `count` (<= 16) listed [K, N] kernels (offsets in floats, ascending, N % 4 == 0,
 * offsets % 4 == 0) in the same launch: shadow = storage-type copy in the master layout (NULL for fp32 engines), wt = K-contiguous copy wt[off + n * K + k] (what
 * mi_transpose_weights writes; may be NULL).  dtype MI_F32 | MI_BF16 = element type of both copies.  skip (may be NULL): per kernel, bit 0 = do not write its shadow
 * copy, bit 1 = do not write its K-contiguous copy (copies that nobody reads).  Bit-identical p / m / v to mi_adam_tf_flat. */
int mi_adam_tf_layouts(void* stream, int dtype, float* param, float* m, float* v, float* grad, long long n, const long long* offsets, const int* K, const int* N, const int* skip, int count, float alpha, const float* alpha_dev, float beta1, float beta2, float epsilon, void* shadow, void* wt, int clear_grad);
/* same + FRAGMENT-ORDERED bf16 copies of some kernels for the activation-resident convolutions (round 5): frag_ptrs[2 i + q] / frag_forms[2 i + q], q = 0, 1, for kernel i -- what
 * mi_ares_pack_weights(form, master kernel) writes (form 0 | 1: a [2048, 256] kernel, 2 | 3: a [1024, 128] kernel, 4 | 6: deconv3's [800, 64], 5: conv2's [512, 64]), emitted by the optimiser launch from the tile it holds anyway;
 * NULL pointer = none.  Both arrays may be NULL (= mi_adam_tf_layouts). */
int mi_adam_tf_layouts_frag(void* stream, int dtype, float* param, float* m, float* v, float* grad, long long n, const long long* offsets, const int* K, const int* N, const int* skip, int count, float alpha, const float* alpha_dev, float beta1, float beta2, float epsilon, void* shadow, void* wt, int clear_grad, void* const* frag_ptrs, const int* frag_forms);
/* out[b, :] = storage_type(src[idx[b], :]) for b < B (idx NULL: rows 0 .. B-1): the frame rows of a minibatch (the feed_dict slice of vae/models.py:211-216) gathered and
 * converted in one launch; dtype MI_F32 | MI_BF16.  The table's row count is not an argument: idx[b] must lie inside the table (the host mirror builds every index vector from
 * arange(N) permutations, vae/models.py:207-212) */
int mi_gather_rows_cast(void* stream, int dtype, const float* src, const int* idx, int B, long long row_len, void* out);
/* the same from a uint8 table of raw camera bytes: out[b, :] = storage_type(float32(src[idx[b], :]) / float32(255)), correctly rounded (vae/train_vae.py:15-18 on the device) */
int mi_gather_rows_cast_u8(void* stream, int dtype, const unsigned char* src, const int* idx, int B, long long row_len, void* out);
int mi_cast_f32_to_bf16(void* stream, const float* src, void* dst, long long n);
/* fp32 <-> split storage (dtype MI_BF16X3): word = bf16(x) << 16 | bf16(x - bf16(x)); back: hi + lo */
int mi_cast_f32_to_split(void* stream, const float* src, void* dst, long long n);
int mi_cast_split_to_f32(void* stream, const void* src, float* dst, long long n);
/* raw uint8 frames -> float32(k) / float32(255), correctly rounded: the reference's host preprocessing (vae/train_vae.py:15-18) done on the device */
int mi_u8_to_unit_f32(void* stream, const unsigned char* src, float* dst, long long n);
/* K-contiguous copies of the [K,N] kernels for the MFMA B operand: dst[off + n*K + k] = (T) src[off + k*N + n], count <= 16 tensors */
int mi_transpose_weights(void* stream, int dtype, const float* src, void* dst, const long long* offsets, const int* K, const int* N, int count);
/* BiasAddGrad: out[n] += sum_m x[m,n].  NON-DETERMINISTIC summation order (row blocks meet in fp32 atomics); mi_colsum_ws is the deterministic form */
int mi_colsum(void* stream, int dtype, const void* x, long long M, int N, float* out);
/* same with caller scratch (>= mi_colsum_scratch_bytes; NULL = the form above): per-block column sums added up in a fixed order -- bitwise reproducible */
long long mi_colsum_scratch_bytes(int dtype, long long M, int N);
int mi_colsum_ws(void* stream, int dtype, const void* x, long long M, int N, float* out, void* scratch, long long scratch_bytes);
/* tf.nn.sigmoid(reconstructed_logits) — vae/models.py:113 */
int mi_sigmoid(void* stream, int dtype, const void* x, float* out, long long n);
/* verify_range — vae/models.py:24-30 */
int mi_range_check(void* stream, const float* x, long long n, float lo, float hi, int* flag);

/* ---- PPO kernels ---- */
/* prob ratio, clipped surrogate, value loss, entropy, and their gradients wrt the heads — ppo.py:58-66,112-132 */
int mi_ppo_loss_blocks(int M);
int mi_ppo_loss_partial_floats(int M);
int mi_ppo_loss_fwd_bwd(void* stream, const float* u, const float* u_old, const float* logstd, const float* logstd_old, const float* vraw, const float* actions, const float* returns, const float* advantage, const float* low, const float* high, int M, int A, float clip_eps, float value_scale, float entropy_scale, float inv_m, float grad_scale, float* du, float* dv, float* partial, float* losses5, float* dlogstd);
/* build_mlp trunk (utils.py:25-28 with ppo.py:42-44,51-53: two dense layers, ReLU on both) as op-level calls; exact fp32.  din, H1, H2 multiples of 4 (pad the state).
 * fwd: h1 = relu(x W1 + b1), h2 = relu(h1 W2 + b2).  bwd: from g2 = dL/dh2 [M, H2]: dW1, db1, dW2, db2 are ACCUMULATED into; scratch M * (H1 + H2) floats.
 * (The engines run the fused forms: mi_ppo_train_step / mi_ppo_predict / mi_rollout_step.) */
int mi_mlp_policy_fwd(void* stream, const float* x, int M, int din, const float* W1, const float* b1, int H1, const float* W2, const float* b2, int H2, float* h1, float* h2);
int mi_mlp_policy_bwd(void* stream, const float* x, int M, int din, const float* W2, int H1, int H2, const float* h1, const float* h2, const float* g2, float* dW1, float* db1, float* dW2, float* db2, float* scratch);
/* action_mean rescale, Normal.sample, clip_by_value — ppo.py:47,58-62 */
int mi_policy_head(void* stream, const float* u, const float* logstd, const float* noise, const float* low, const float* high, int M, int A, int greedy, float* action, float* mean_out);
/* compute_gae — utils.py:45-50 (fp64, rounding sequence of numpy + scipy.signal.lfilter) */
int mi_gae_scan(void* stream, const double* rewards, const double* values, const double* terminals, int R, int T, double gamma, double lam, double* adv);
/* returns = adv + values; advantage normalisation — train.py:176-177 (fp64, population std, per row) */
int mi_adv_normalize(void* stream, double* adv, const double* values, int R, int T, double* returns);


/* ---- ConvVAE engine: the graph of VAE.__init__ + ConvVAE (vae/models.py:85-142,249-266) on caller-owned buffers ---- */
int mi_vae_desc_size(void);
int mi_vae_tensor_count(void);
long long mi_vae_param_floats(const MiVaeDesc* d);
int mi_vae_param_layout(const MiVaeDesc* d, long long* offsets, long long* sizes, int n);
long long mi_vae_workspace_bytes(const MiVaeDesc* d);
void* mi_vae_create(const MiVaeDesc* d, float* params, float* grads, float* adam_m, float* adam_v, void* bf16_shadow, void* weights_t, void* workspace, long long workspace_bytes);
void mi_vae_destroy(void* h);
int mi_vae_sync_shadow(void* h, void* stream);
/* device pointers into the workspace: 0 losses[2] (recon, kl), 1 mean [B,Z], 2 logvar [B,Z], 3 kl_row [B] (fp32); 4 logits [B,P], 5 z [B,Z] (storage type T).
 * For tests: 6..16 the fragment-ordered weight copies (NULL unless the activation-resident kernels take the model); the tensors the last pass stored, type T, NHWC at
 * the CURRENT batch: 20 + i = output of conv i (i = 1..4), 30 + i = dense1's output (i = 0) / output of deconv i (i = 1..4), 40 + i and 50 + i = the gradients wrt those
 * (pre-activation), 60 = dheads [B,2Z].  NULL where the workspace has no such region (an inference-only engine has no gradients, and no conv1 output behind the fused
 * encoder head) and for any other `which`.  A fused route leaves a region it skips unwritten. */
void* mi_vae_buffer(void* h, int which);
/* Debug mode of the engine workspace (sanitizer row): with MI355_DEBUG_GUARDS=1 in the environment of BOTH mi_vae_workspace_bytes and mi_vae_create every
 * workspace region is followed by 256 guard bytes of a known pattern (armed by mi_vae_create).  *n_regions = guarded regions (0: mode off), *n_bad = guards that no longer
 * hold the pattern (a kernel wrote past the region in front of it; mi_last_error() names the first); guard_index >= 0 additionally returns that guard's byte offset.
 * Synchronises the device; never used on the production path. */
int mi_vae_debug_check_guards(void* h, int* n_regions, int* n_bad, int guard_index, long long* guard_offset);
/* forward + ELBO terms: the per-minibatch sess.run of VAE.evaluate (vae/models.py:226-229) / forward half of train_step (:213-216) */
/* frames_u8 != 0: src / tgt are raw uint8 frame tables (bf16 engine, rgb target == source format); eps == NULL with sample != 0: the engine draws the noise (mi_vae_set_seed) */
int mi_vae_forward(void* h, void* stream, const void* src, const void* tgt, int frames_u8, const int* idx, int B, float inv_batch, const float* eps, int sample, int want_grad, float* metrics3, float metric_weight);
/* gradients of loss = recon + beta*kl wrt all 22 variables (optimizer.minimize, vae/models.py:142); part 0 all, 1 decoder half,
 * 2 encoder half = 3 (heads + conv4) then 4 (conv3..conv1): the data-parallel host all-reduces a finished part's bucket under the next part */
int mi_vae_backward(void* h, void* stream, const void* src, const int* idx, const float* eps, float inv_batch, int part);
int mi_vae_apply_adam(void* h, void* stream, float alpha, float beta1, float beta2, float epsilon);
/* seed of the engine's own N(0,1) source (TF's graph-level seed, train.py:50-51) */
int mi_vae_set_seed(void* h, unsigned long long seed);
/* one whole SGD step = the reference's sess.run([train_step, ...]) (vae/models.py:213-216) in ONE call (eager launches on the caller's stream + the engine's filter-gradient stream; nothing synchronises the host) */
int mi_vae_train_step(void* h, void* stream, const void* src, const void* tgt, int frames_u8, const int* idx, int B, float inv_batch, const float* eps, float alpha, float beta1, float beta2, float epsilon, float* metrics3, float metric_weight);
/* the data-parallel form of the same step in ONE call (no reference counterpart: the reference is single-process): this rank's rows with inv_batch = 1 / B_global,
 * backward in the three parts of mi_vae_dp_buckets, each finished bucket's all-reduce on the communicator's own stream under the next part, mi_comm_wait, TF-Adam.
 * mi_vae_dp_buckets (pure, no GPU): out9 = 3 x {part, first float, one past the last float of the flat gradient buffer} in completion order. */
int mi_vae_dp_buckets(const MiVaeDesc* d, long long* out9);
int mi_vae_train_step_dp(void* h, void* comm, void* stream, const void* src, const void* tgt, int frames_u8, const int* idx, int B, float inv_batch, const float* eps, float alpha, float beta1, float beta2, float epsilon, float* metrics3, float metric_weight);
/* VAE.encode / generate_from_latent (= north_star "decode") / reconstruct — vae/models.py:188-202 */
int mi_vae_encode(void* h, void* stream, const void* src, int frames_u8, const int* idx, int B, float* mean_out);
int mi_vae_decode(void* h, void* stream, const float* z, int B, float* recon_out);
int mi_vae_reconstruct(void* h, void* stream, const void* src, int frames_u8, const int* idx, int B, const float* eps, int sample, float* recon_out);

/* ---- MlpVAE engine (round 4; vae/models.py:271-299 on the base graph :85-142): the same surface as the ConvVAE engine for the dense variant.  Frame tables are float32 (or, round 5, uint8 camera bytes: frames_u8)
 * [n_frames, source_size] / [n_frames, target_size] on the device; the noise eps [B, z_dim] comes from the caller (mi_normal_philox); gradients are STORED into the
 * gradient buffer by every backward pass (not accumulated).  Tensor order of mi_mlpvae_param_layout: encoder layers {kernel [K, N], bias}, heads {kernel [K, 2 z] =
 * [mean | logstd_sqare], bias}, decoder layers incl. the output layer {kernel, bias}; no padding between tensors. ---- */
int mi_mlpvae_desc_size(void);
long long mi_mlpvae_param_floats(const MiMlpVaeDesc* d);
int mi_mlpvae_tensor_count(const MiMlpVaeDesc* d);
int mi_mlpvae_param_layout(const MiMlpVaeDesc* d, long long* offsets, long long* sizes, int n);
long long mi_mlpvae_workspace_bytes(const MiMlpVaeDesc* d);
void* mi_mlpvae_create(const MiMlpVaeDesc* d, float* params, float* grads, float* adam_m, float* adam_v, void* shadow, void* weights_t, void* workspace, long long workspace_bytes);
void mi_mlpvae_destroy(void* h);
int mi_mlpvae_sync_shadow(void* h, void* stream);
/* device pointers into the workspace: 0 losses[2] (recon, kl), 1 mean [B,Z], 2 logvar [B,Z], 3 kl_row [B] (fp32); 4 logits [B,P], 5 z [B,Z] (storage type T).
 * For tests, the other tensors the last pass stored (type T unless noted, rows at the CURRENT batch): 10 the staged input x [B,S] (left unwritten where the fp32 engine
 * reads the caller's float table directly: idx == NULL), 11 the raw heads [B,2Z] fp32 (no bias), 12 the split-K slab region (fp32 [slabs][B][N] of the last
 * split product, from the region's start; 16 bytes where no layer splits); 20 + i = output of encoder layer i, 30 + i = output of decoder layer i
 * (the last one: the logits), 40 + i and 50 + i = the gradients wrt those (pre-activation), 60 = dheads [B,2Z], 61 = dz [B,Z] fp32.  NULL where the workspace has no
 * such region (an inference-only engine has no gradients) and for any other `which`. */
void* mi_mlpvae_buffer(void* h, int which);
/* Debug mode of the workspace, as mi_vae_debug_check_guards: with MI355_DEBUG_GUARDS=1 in the environment of BOTH mi_mlpvae_workspace_bytes and mi_mlpvae_create every
 * workspace region is followed by 256 guard bytes of a known pattern (armed by mi_mlpvae_create).  *n_regions = guarded regions (0: mode off), *n_bad = guards that no
 * longer hold the pattern (mi_last_error() names the first); guard_index >= 0: that guard's byte offset in *guard_offset (-1: no such guard).  Synchronises the device;
 * writes and reads the engine's own workspace only.  With the variable unset the workspace size and every offset are what they were. */
int mi_mlpvae_debug_check_guards(void* h, int* n_regions, int* n_bad, int guard_index, long long* guard_offset);
long long mi_mlpvae_decoder_offset(void* h);
/* round 5: src / tgt are `const void*` + frames_u8 (bit 0: src is a uint8 table of raw camera bytes, bit 1: tgt is; 0: float32 tables as before): the bytes are normalised to
 * float32(k) / float32(255) -- the reference's host preprocessing, vae/train_vae.py:15-18 -- where the minibatch rows are staged / inside the loss kernel */
int mi_mlpvae_forward(void* h, void* stream, const void* src, const void* tgt, int frames_u8, const int* idx, int B, float inv_batch, const float* eps, int sample, int want_grad, float* metrics3, float metric_weight);
int mi_mlpvae_backward(void* h, void* stream, const float* eps, float inv_batch, int part);
int mi_mlpvae_apply_adam(void* h, void* stream, float alpha, float beta1, float beta2, float epsilon);
int mi_mlpvae_train_step(void* h, void* stream, const void* src, const void* tgt, int frames_u8, const int* idx, int B, float inv_batch, const float* eps, float alpha, float beta1, float beta2, float epsilon, float* metrics3, float metric_weight);
/* round 6 (ABI 7): one DATA-PARALLEL SGD step of the MlpVAE (vae/models.py:271-299 behind :140-142,213-216) in ONE call -- forward + ELBO of this rank's rows (inv_batch =
 * 1 / B_global), the decoder half of the backward pass, its gradients' all-reduce on the communicator's own stream under the encoder half, that half's all-reduce, the join,
 * TF-Adam.  mi_mlpvae_dp_buckets: out6 = 2 x {part, first float, one past the last float of the flat gradient buffer} in completion order. */
int mi_mlpvae_dp_buckets(void* h, long long* out6);
int mi_mlpvae_train_step_dp(void* h, void* comm, void* stream, const void* src, const void* tgt, int frames_u8, const int* idx, int B, float inv_batch, const float* eps, float alpha, float beta1, float beta2, float epsilon, float* metrics3, float metric_weight);
int mi_mlpvae_encode(void* h, void* stream, const void* src, int frames_u8, const int* idx, int B, float* mean_out);
int mi_mlpvae_decode(void* h, void* stream, const float* z, int B, float* recon_out);
int mi_mlpvae_reconstruct(void* h, void* stream, const void* src, int frames_u8, const int* idx, int B, const float* eps, int sample, float* recon_out);

/* one environment step of the rollout loop in one call — vae_common.py:45-61 (encode_state) + ppo.py:231-251 (predict): raw uint8 frame [IH,IW,3] and
 * measurements -> out [num_actions + 1 + z_dim] = action | value | z; noise [num_actions] for sampling or NULL with greedy.  Exact fp32.
 * Every buffer may be HBM or pinned (device-mapped) host memory: with pinned buffers the step needs no copy in either direction. */
int mi_rollout_step(void* vae_h, void* ppo_h, void* stream, const unsigned char* frame_u8, const float* measurements, int n_meas, const float* noise, int greedy, float* out);
/* the same step for n environments in one call (same eight launches, rows of every layer running over the environments) — vae_common.py:45-61 + ppo.py:231-251 per
 * environment: frames_u8 [n][IH*IW*3], measurements [n][n_meas], noise [n][num_actions] or NULL with greedy -> out [n][num_actions + 1 + z_dim], row e = action | value | z of
 * environment e; rows >= n are not written.  Exact fp32 on the master weights.  1 <= n <= MI_ROLLOUT_MAX_ENVS and n <= the PPO engine's max_batch (the trunks' raw sums live in
 * that engine's workspace); anything else is an error and launches nothing.  Input and output buffers may be HBM or pinned host memory; `scratch` is HBM, 16-byte aligned, at
 * least mi_rollout_batch_workspace_bytes(vae_h, ppo_h, n) bytes (fp32 act1 | raw sums of conv2..conv4 | raw means: 0.67 MB per environment at the reference geometry; < 0 = error). */
#define MI_ROLLOUT_MAX_ENVS 1024
long long mi_rollout_batch_workspace_bytes(void* vae_h, void* ppo_h, int n_envs);
int mi_rollout_step_batch(void* vae_h, void* ppo_h, void* stream, const unsigned char* frames_u8, const float* measurements, int n_meas, const float* noise, int greedy, int n, void* scratch, long long scratch_bytes, float* out);
/* the batched step that also RECORDS what it computed (same eight launches, the last one being the recording heads) — vae_common.py:45-61 + ppo.py:231-251 per environment, and the
 * state / value the trainer keeps per step and for the bootstrap (train.py:172): the arguments of mi_rollout_step_batch, and call row e is stored as row r = table_rows[e] of
 * the horizon-batch tables mi_ppo_train_step_idx gathers from: tab_states[r] = [z | measurements[e]] (z_dim + n_meas floats), tab_actions[r] (num_actions floats),
 * tab_values[r] -- the registers that go to `out`, bit for bit.  table_rows: int32 [n], HBM or pinned host memory like the other inputs; a row outside [0, n_table_rows)
 * (-1 = "do not record this environment") is skipped: no value of it stores outside the tables.  The tables are HBM with n_table_rows rows each.  Same checks as
 * mi_rollout_step_batch, plus missing tables. */
int mi_rollout_step_batch_rec(void* vae_h, void* ppo_h, void* stream, const unsigned char* frames_u8, const float* measurements, int n_meas, const float* noise, int greedy, int n, void* scratch, long long scratch_bytes, float* out, const int* table_rows, long long n_table_rows, float* tab_states, float* tab_actions, float* tab_values);
/* the VALUE of n observations and nothing else -- the final observations of episodes that were TRUNCATED (stopped without being terminal, train.py:172's bootstrap value
 * for an episode whose lane goes on with a reset observation): the encoder chain of mi_rollout_step_batch, the value trunk alone and a value head whose arithmetic is
 * the step's (ppo.py:70-71), eight launches like the step.  out [n] = the values; call row e is also stored as tab_final_values[table_rows[e]] (fp32, n_table_rows entries, HBM; plain
 * vector stores); a row outside [0, n_table_rows) records nothing.  frames_u8 / measurements / table_rows / out: HBM or pinned host memory; `scratch` as for
 * mi_rollout_step_batch (the same bytes).  The policy net's raw sums in the PPO engine are neither cleared nor read.  Same checks as mi_rollout_step_batch, plus missing tables. */
int mi_rollout_value_batch_rec(void* vae_h, void* ppo_h, void* stream, const unsigned char* frames_u8, const float* measurements, int n_meas, int n, void* scratch, long long scratch_bytes, float* out, const int* table_rows, long long n_table_rows, float* tab_final_values);
/* finishes a RAGGED rollout buffer in one launch — compute_gae (utils.py:45-50) + returns and advantage normalisation (train.py:175-177) per row: row e of num_envs has
 * len[e] = L <= T recorded steps in slots 0 .. L-1 of its T + 1 table slots (table row e (T + 1) + t) and the bootstrap value in slot L.  tab_values: the fp32 values table;
 * rewards / terminals: fp64 [num_envs, T]; len: int32 [num_envs] (all device).  fp64 with the rounding sequence of mi_gae_scan + mi_adv_normalize on that row alone (divisor L,
 * population std, + 1e-8), bit for bit.  Writes fp32 returns / normalised advantages into tab_returns / tab_advantages (round to nearest even) and, where non-NULL, fp64
 * raw advantages / returns / normalised advantages [num_envs, T].  Slots >= L and rows with L = 0 are not written.  1 <= T <= MI_ROLLOUT_MAX_HORIZON. */
#define MI_ROLLOUT_MAX_HORIZON 4096
int mi_rollout_finish(void* stream, const float* tab_values, const double* rewards, const double* terminals, const int* len, int num_envs, int T, double gamma, double lam, float* tab_returns, float* tab_advantages, double* adv_raw, double* returns, double* adv_norm);
/* the same finish for lanes that hold SEVERAL episodes (continuous collection) — compute_gae (utils.py:45-50) + returns and advantage normalisation (train.py:175-177) per
 * SEGMENT: segment i is seg_len[i] = n recorded steps that start at table row seg_row[i] = e (T + 1) + s of lane e and lie inside its step slots (s + n <= T); seg_row /
 * seg_len: int32 [n_seg] on the device; the other buffers as in mi_rollout_finish.  If the segment's last step has terminals != 0 its bootstrap value is 0.0 and the slot
 * behind it is NOT read (it may hold the next episode's first value, or a stale one); otherwise it is the table value in the slot behind it.  normalize = 0: every segment
 * comes out bit for bit as mi_gae_scan + mi_adv_normalize give it on that segment alone (divisor n, population std, + 1e-8; fp32 tables round to nearest even).
 * normalize = 1: returns and raw advantages as before; the normalised advantages use the mean and population std (+ 1e-8) over ALL steps of all segments of the call,
 * summed in a fixed order (per-segment partials, then the partials in segment order; no floating-point atomics: two calls are bitwise equal); it NEEDS adv_raw (the raw
 * advantages are read back from it) and `scratch`, device doubles, at least mi_rollout_finish_segments_scratch_doubles(n_seg) = 2 n_seg + 2 of them; scratch may be
 * NULL with normalize = 0.  A descriptor that does not lie inside one lane's step slots (n < 1, s + n > T, lane >= num_envs, negative row) is not executed; slots that
 * belong to no executed segment are not written.  n_seg, num_envs, T >= 1, T <= MI_ROLLOUT_MAX_HORIZON. */
long long mi_rollout_finish_segments_scratch_doubles(int n_seg);
int mi_rollout_finish_segments(void* stream, const float* tab_values, const double* rewards, const double* terminals, const int* seg_row, const int* seg_len, int n_seg, int num_envs, int T, double gamma, double lam, int normalize, double* scratch, float* tab_returns, float* tab_advantages, double* adv_raw, double* returns, double* adv_norm);
/* mi_rollout_finish_segments with a per-segment bootstrap source — compute_gae (utils.py:45-50) + train.py:175-177 per segment: seg_boot: int32 [n_seg] on the device.
 * seg_boot[i] == 0: exactly mi_rollout_finish_segments' rule.  seg_boot[i] != 0 (the segment was TRUNCATED: its episode stopped without being terminal and the lane went
 * on): the value behind the last step is tab_final_values[seg_row[i] + seg_len[i] - 1] (fp32 [num_envs (T + 1)], what mi_rollout_value_batch_rec left at the row of
 * that step) and the slot behind the segment in tab_values is NOT read (it holds the next episode's first value, or a stale one); the segment comes out bit for bit as
 * mi_gae_scan + mi_adv_normalize give it on [v_0 .. v_{n-1}, v_final].  normalize, scratch and every other argument as in mi_rollout_finish_segments, and the same checks. */
int mi_rollout_finish_segments_boot(void* stream, const float* tab_values, const double* rewards, const double* terminals, const int* seg_row, const int* seg_len, int n_seg, int num_envs, int T, double gamma, double lam, int normalize, double* scratch, float* tab_returns, float* tab_advantages, double* adv_raw, double* returns, double* adv_norm, const float* tab_final_values, const int* seg_boot);
/* the finish with V-TRACE off-policy correction (Espeholt et al. 2018, IMPALA; no reference counterpart in train.py) -- for the refreshes of a multi-epoch update,
 * where the recorded actions came from pi_old and the values are those of the moved parameters.  Segment form: seg_row / seg_len (and, both or neither,
 * tab_final_values / seg_boot) as in mi_rollout_finish_segments[_boot].  tab_logp_now / tab_logp_old: fp32 [num_envs (T + 1)] in the table layout (row
 * e (T + 1) + t): log pi_theta(a_t | s_t) (mi_ppo_logp_idx) and the cache of log pi_old.  Per step w_t = exp((double)lp_now - (double)lp_old), delta_t as in the GAE
 * entries, and from the segment's last step to its first, in fp64 with each product and sum rounded once, in this order (gl = gamma * lam, D_L = 0):
 *     A_t = gl D_{t+1} + delta_t                                            the policy advantage delta_t + gamma lam (vs_{t+1} - V_{t+1})
 *     D_t = ((gl min(c_bar, w_t)) D_{t+1}) + (min(rho_bar, w_t) delta_t)    vs_t - V_t
 * tab_returns / returns = D_t + V_t (the V-trace value target), adv_raw = A_t, tab_advantages / adv_norm = A normalised per segment (normalize = 0) or over the
 * batch (normalize = 1: scratch and adv_raw as in mi_rollout_finish_segments, the same kernels behind it, fixed order, no atomics); weights_out (fp64
 * [num_envs, T], or NULL) receives w_t.  The weight of step t does NOT multiply A_t: PPO's surrogate applies the ratio itself.  A NaN weight is not masked by
 * a bar: it reaches the segment's outputs.  read_behind_done = 1: the successor value by mi_rollout_finish's rule (the slot behind a terminal last step is read
 * and masked by the flag); 0: by the segment entries' rule (0.0, the slot is not read).  A truncated segment (seg_boot[i] != 0) takes tab_final_values under either.
 * TERMINALS: as in the GAE entries the recurrence is not cut at a terminal inside a segment -- segments end at their terminal.
 * THE GAE IDENTITY: with w_t = 1 (tab_logp_now bitwise tab_logp_old), rho_bar >= 1 and c_bar >= 1 every product with a weight is exact and D = A = the GAE
 * recurrence: all outputs are bit for bit those of mi_rollout_finish (read_behind_done = 1, one segment per lane) or mi_rollout_finish_segments[_boot] (0).
 * A descriptor that does not lie inside one lane's step slots is not executed and adds nothing to the batch sums; slots of no executed segment are not written.
 * MI_ERR_ARG, before any launch and with nothing written: T outside [1, MI_ROLLOUT_MAX_HORIZON]; n_seg or num_envs < 1; rho_bar NaN or <= 0; c_bar NaN or < 0
 * (+inf is a valid bar: never truncates); read_behind_done or normalize outside {0, 1}; missing buffers; exactly one of tab_final_values / seg_boot; scratch or
 * adv_raw NULL with normalize = 1.  Dynamic LDS: 2 T doubles (64 KB at T = 4096). */
int mi_rollout_finish_vtrace(void* stream, const float* tab_values, const float* tab_logp_now, const float* tab_logp_old, const double* rewards, const double* terminals, const int* seg_row, const int* seg_len, int n_seg, int num_envs, int T, double gamma, double lam, double rho_bar, double c_bar, int read_behind_done, int normalize, double* scratch, float* tab_returns, float* tab_advantages, double* adv_raw, double* returns, double* adv_norm, double* weights_out, const float* tab_final_values, const int* seg_boot);
/* running-return reward scaling in front of the finish calls above — baselines' VecNormalize (ret = ret * gamma + rew; ret_rms.update(ret); rew / sqrt(ret_rms.var + epsilon),
 * clipped), no reference counterpart in train.py: the rewards of one collection divided by the running standard deviation of the discounted return.  No engine handle.
 * rewards / terminals: fp64 [num_envs, T]; truncs: uint8 [num_envs, T] or NULL (none); len: int32 [num_envs], the recorded steps per lane (0: an unused lane; a value
 * beyond T is clamped to T); state: double [4] = {count, mean, M2, den}; carry: double [num_envs], the discounted return each lane's running episode has reached;
 * g_out / rewards_out: fp64 [num_envs, T] (all device; rewards_out must not overlap rewards).  fp64 throughout, per lane e with L = len[e] >= 1:
 *   c = carry[e];  for t = 0 .. L-1:  G[e,t] = c * gamma + r[e,t]  (one multiply, then one add: no fused multiply-add);  c = (terminals[e,t] != 0 || truncs[e,t]) ? 0.0 : G[e,t]
 *   carry[e] = c   (a lane with L = 0 keeps its carry and writes nothing)
 *   n_b = sum of L,  m_b = sum of G / n_b,  M2_b = sum of (G - m_b)^2   (two passes; per-lane partials by lane-strided sums and a wave reduction, the lanes' partials added
 *                                                                        by one wave in lane-strided order; no floating-point atomics: two calls are bitwise equal)
 *   merge = 1 (Chan / Welford):  delta = m_b - mean;  n' = count + n_b;  mean += delta * n_b / n';  M2 += M2_b + delta^2 * count * n_b / n';  count = n'
 *   merge = 0 (frozen statistics): state[0..2] stay bitwise as they were; the carry still advances.  An empty batch (n_b = 0) merges nothing.
 *   var = count > 0 ? M2 / count : 1.0;  den = state[3] = sqrt(var + epsilon);  rewards_out[e,t] = min(max(r[e,t] / den, -clip), clip)  (a true division)
 * Entries of g_out / rewards_out at t >= L are not written and entries of the inputs at t >= L are not read.  DEVIATIONS from baselines, both on purpose: a collection is
 * scaled by ONE factor, from statistics that already include it ("update ret_rms, then divide" per update instead of per step: per-step scaling needs the reward on the
 * device at every step and puts the rewards of one collection on different scales), and the statistics start from count = 0, not from the prior count = 1e-4, var = 1.
 * scratch: device doubles, at least mi_rollout_scale_rewards_scratch_doubles(num_envs) = 2 num_envs + 2 (needs no GPU; -1 for num_envs < 1).  Four small launches
 * (scan + per-lane sums; batch mean + per-lane squared deviations; merge; scaling stores), dynamic LDS sized by T.  Errors (checked before any launch, nothing is written):
 * missing buffers; num_envs < 1 or T < 1; T > MI_ROLLOUT_MAX_HORIZON; num_envs > MI_ROLLOUT_MAX_ENVS; gamma outside [0, 1] or NaN; epsilon not finite or < 0; clip NaN
 * or <= 0 (+inf is valid: never clamp); merge outside {0, 1}. */
long long mi_rollout_scale_rewards_scratch_doubles(int num_envs);
int mi_rollout_scale_rewards(void* stream, const double* rewards, const double* terminals, const unsigned char* truncs, const int* len, int num_envs, int T, double gamma, double epsilon, double clip, int merge, double* state, double* carry, double* scratch, double* g_out, double* rewards_out);
/* running OBSERVATION normalisation, the other half of baselines' VecNormalize (obs_rms; clip(obs - mean) / sqrt(var + epsilon)), no reference counterpart in train.py:
 * the batched step of vae_common.py:45-61 + ppo.py:231-251 with the state [z | measurements] standardised per column in front of trunk layer 1.
 * mi_rollout_step_batch_norm: the arguments and checks of mi_rollout_step_batch, and obs_mean / obs_inv_std: fp32 [din] on the device (din = z_dim + n_meas), obs_clip > 0
 * (+inf is valid: never clamp), nstate: fp32 [n][din], HBM, 16-byte aligned, the caller's (mi_rollout_batch_workspace_bytes does not grow).  One more launch than
 * mi_rollout_step_batch, between the mean layer and trunk layer 1: with s = the raw state entry (mean_raw + mean_bias for a latent column, the measurement as fed for the others)
 *   nstate[e][j] = min(max((s - obs_mean[j]) * obs_inv_std[j], -obs_clip), obs_clip)      (fp32: one subtract, one multiply)
 * and trunk layer 1 reads nstate.  Nothing changes obs_mean / obs_inv_std during the call: every row is normalised alike.  `out` is what mi_rollout_step_batch returns: its
 * latents are the RAW z.  table_rows != NULL: the recording step; call row e is stored as row r = table_rows[e] (inside [0, n_table_rows), else skipped) of tab_states[r] = the
 * NORMALISED row (plain vector stores), tab_raw_states[r] = [z | measurements[e]] (the bits mi_rollout_step_batch_rec stores), tab_actions[r], tab_values[r].  table_rows ==
 * NULL records nothing (the evaluation step; the four tables are not read).
 * mi_rollout_value_batch_norm: mi_rollout_value_batch_rec (train.py:172's bootstrap value of a truncated episode) with the same normalise launch in front of the value trunk;
 * no table of states is written.  Errors of both (MI_ERR_ARG, before any launch): those of the entries they extend; obs_mean / obs_inv_std / nstate NULL; nstate not 16-byte
 * aligned; obs_clip <= 0 or NaN; table_rows without all four tables. */
int mi_rollout_step_batch_norm(void* vae_h, void* ppo_h, void* stream, const unsigned char* frames_u8, const float* measurements, int n_meas, const float* noise, int greedy, int n, void* scratch, long long scratch_bytes, float* out, const float* obs_mean, const float* obs_inv_std, float obs_clip, float* nstate, const int* table_rows, long long n_table_rows, float* tab_states, float* tab_raw_states, float* tab_actions, float* tab_values);
int mi_rollout_value_batch_norm(void* vae_h, void* ppo_h, void* stream, const unsigned char* frames_u8, const float* measurements, int n_meas, int n, void* scratch, long long scratch_bytes, float* out, const float* obs_mean, const float* obs_inv_std, float obs_clip, float* nstate, const int* table_rows, long long n_table_rows, float* tab_final_values);
/* the batched rollout step for the MlpVAE encoder (--vae_model_type mlp; vae/models.py:271-299 in front of vae_common.py:45-61 + ppo.py:231-251): mlp_h is a handle of
 * mi_mlpvae_create.  The mi_rollout_* entries above read their vae_h as a ConvVAE engine and never inspect it: an MlpVAE handle goes to these two entries only.
 * Exact fp32 on the fp32 master weights (params), whatever the engine's storage type.  Launches: clear (every raw-sum buffer of the call: nothing depends on what the
 * scratch held on entry) -> layer 1 from the camera bytes (rollout_mlp.hip: W1 streamed once, every frame byte fetched once, K split over ceil(S / KS) blocks, KS = 64 .. 256 by n, that meet by
 * fp32 atomics) -> hidden layers 2.. and the mean head as the flat split-K layers of mi_rollout_step_batch -> the trunks and heads of mi_rollout_step_batch.
 * scratch: HBM, 16-byte aligned, at least mi_mlp_rollout_workspace_bytes(d, n) = 4 n (enc[0] + .. + enc[n_enc - 1] + z_dim) bytes (raw sums [n][enc[0]] | .. | raw means
 * [n][z_dim]; needs no handle and no GPU; MI_ERR_ARG for n_envs outside 1 .. MI_ROLLOUT_MAX_ENVS, MI_ERR_SHAPE for a desc mi_mlpvae_create refuses).  frames_u8: uint8
 * [n][source_size], HBM or pinned host memory, 4-byte aligned.  measurements / noise / out / n / greedy as in mi_rollout_step_batch.
 * mi_mlp_rollout_step_batch is the plain, the recording and the normalised step in one: obs_mean == NULL: no normalisation (obs_inv_std, nstate and tab_raw_states must be NULL
 * too; tab_states takes the raw rows [z | measurements], as mi_rollout_step_batch_rec stores them); else the arguments of mi_rollout_step_batch_norm.  table_rows == NULL
 * records nothing (no table is read).  mi_mlp_rollout_value_batch: the value-only call (mi_rollout_value_batch_rec / _norm); table_rows may be NULL: the values go to out alone.
 * Errors, each message under the entry's own name, everything that needs no device before the first launch: null handle (MI_ERR_STATE); missing buffers or tables, n outside
 * 1 .. MI_ROLLOUT_MAX_ENVS, frames not 4-byte / scratch or nstate not 16-byte aligned, obs_clip <= 0 or NaN, scratch too small, more than 8 actions, n above the PPO
 * engine's max_batch (MI_ERR_ARG); z_dim + n_meas != the policy's input size (MI_ERR_SHAPE). */
long long mi_mlp_rollout_workspace_bytes(const MiMlpVaeDesc* d, int n_envs);
int mi_mlp_rollout_step_batch(void* mlp_h, void* ppo_h, void* stream, const unsigned char* frames_u8, const float* measurements, int n_meas, const float* noise, int greedy, int n, void* scratch, long long scratch_bytes, float* out, const float* obs_mean, const float* obs_inv_std, float obs_clip, float* nstate, const int* table_rows, long long n_table_rows, float* tab_states, float* tab_raw_states, float* tab_actions, float* tab_values);
int mi_mlp_rollout_value_batch(void* mlp_h, void* ppo_h, void* stream, const unsigned char* frames_u8, const float* measurements, int n_meas, int n, void* scratch, long long scratch_bytes, float* out, const float* obs_mean, const float* obs_inv_std, float obs_clip, float* nstate, const int* table_rows, long long n_table_rows, float* tab_final_values);
/* the moments pass behind it — VecNormalize's obs_rms.update at the granularity of a collection, no reference counterpart in train.py.  No engine handle.  The rows
 * row_idx[i], i < n (int32, device; a row outside [0, n_table_rows) is skipped and does not count) of tab_raw_states (fp32 [n_table_rows][din]) are merged into
 * state: double [1 + 2 din] = {count, mean[din], M2[din]}, per column j, fp64 throughout:
 *   n_b = rows inside the table,  m_b = sum of x / n_b,  M2_b = sum of (x - m_b)^2      (two passes over the rows; ordered sums: per-block partials over consecutive list
 *                                                                                       entries, added in block order; the partition is a function of n alone; no
 *                                                                                       floating-point atomics: two calls are bitwise equal)
 *   merge = 1 (Chan / Welford):  delta = m_b - mean;  n' = count + n_b;  mean += delta * n_b / n';  M2 += M2_b + delta^2 * count * n_b / n';  count = n'
 *   merge = 0 (frozen statistics) and an empty batch (n_b = 0) leave state bitwise as it was.
 *   A batch with an entry that is not finite (NaN, +-inf: then some m_b is not finite) is NOT merged, in any column: state stays bitwise as it was, the fp32 pair is
 *   derived from it, and batch_out holds the m_b that show it -- one such entry would otherwise make mean / M2 NaN for good.
 *   var = count > 0 ? M2 / count : 1.0;  obs_mean[j] = float32(mean);  obs_inv_std[j] = float32(1 / sqrt(var + epsilon));  j < first_col: obs_mean[j] = 0, obs_inv_std[j] = 1
 * (fresh statistics give mean 0 and inv_std exactly 1.0f).  batch_out: double [3][din] = m_b | M2_b | the number of the batch's entries of column j whose normalised value
 * under obs_mean / obs_inv_std AS THEY WERE ON ENTRY has magnitude clip (the normalise kernel's expression).  n = 0: nothing is read but state, the fp32 pair is derived
 * (tab_raw_states, row_idx and scratch may be NULL).  DEVIATIONS from baselines, both on purpose: the statistics move once per collection, not per step, so every row of a
 * collection is normalised alike, and they start from count = 0, not from the prior count = 1e-4.
 * scratch: device doubles, at least mi_rollout_obs_stats_scratch_doubles(n, din) = 3 nb din + nb + din + 1 with nb = ceil(n / max(32, ceil(n / 256))) (needs no GPU; -1 for
 * n < 1 or din < 1).  Three small launches.  Errors (MI_ERR_ARG, checked before any launch, nothing is written): missing buffers; n < 0; din < 1 or n_table_rows < 1;
 * first_col outside [0, din]; merge outside {0, 1}; epsilon not finite or < 0; clip NaN or <= 0 (+inf is valid). */
long long mi_rollout_obs_stats_scratch_doubles(long long n, int din);
int mi_rollout_obs_stats(void* stream, const float* tab_raw_states, long long n_table_rows, const int* row_idx, long long n, int din, int first_col, int merge, double epsilon, float clip, double* state, float* obs_mean, float* obs_inv_std, double* scratch, double* batch_out);
/* LATENT STACKING — frame stacking (the usual remedy for a feed-forward policy that sees one frame per step) on the compressed observation, no reference counterpart in
 * train.py: the batched step of vae_common.py:45-61 + ppo.py:231-251 on the state
 *   s_t = [ z_t | z_{t-1} | .. | z_{t-k+1} | measurements_t ],   din = k z_dim + n_meas <= 1024,   2 <= k = latent_stack <= MI_ROLLOUT_MAX_STACK
 * One more launch than mi_rollout_step_batch (rollout_stack_kernel, where the normaliser of mi_rollout_step_batch_norm runs: between the mean layer and trunk layer 1), one
 * block per call row e.  hist: fp32 [n_lanes][k - 1][z_dim], HBM, the per-environment memory: slot 0 of lane l is the latent of that lane's previous step.  lanes / first:
 * int32 [n], HBM or pinned host memory like the other inputs: the history lane of call row e (the lanes of one call are distinct: the caller's duty) and whether the row
 * is the first step of an episode.  With z_t = mean_raw + mean_bias, the sum `out` returns as z:
 *   old_i = first[e] != 0 ? z_t : hist[lanes[e]][i - 1],  i = 1 .. k - 1        (a select: NaN in a history that `first` overrides does not reach the row)
 *   row   = [ z_t | old_1 | .. | old_{k-1} | measurements[e] ]
 * An episode's first step repeats its own latent, as frame stacking pads with the first observation.  A lane outside [0, n_lanes) is treated as `first` and no history is
 * read or written for it.  The row goes, as plain vector stores of one register, to sstate[e] (fp32 [n][din], HBM, 16-byte aligned, the caller's: trunk layer 1 reads
 * it) and, where table_rows != NULL and r = table_rows[e] lies in [0, n_table_rows), to tab_states[r]; old_1 .. old_{k-1} go to older_out[e] (fp32 [n][(k - 1) z_dim], HBM
 * or pinned host memory; NULL: nowhere), so the caller can return the whole state without a copy of the history.  obs_mean != NULL (fp32 [din], with obs_inv_std and
 * obs_clip as in mi_rollout_step_batch_norm): sstate[e] and tab_states[r] take min(max((s - obs_mean[j]) * obs_inv_std[j], -obs_clip), obs_clip) instead and
 * tab_raw_states[r] the raw row; obs_mean == NULL: obs_inv_std and tab_raw_states must be NULL too.  The recording heads store tab_actions[r] and tab_values[r] and no
 * state row.  Behind a barrier -- every read of a lane's history comes before every write of it -- and only with advance != 0:
 *   hist[lanes[e]] = [ z_t | old_1 | .. | old_{k-2} ]
 * advance == 0 writes nothing into hist (the bootstrap observation is stepped again when its episode continues).  `out`, noise, greedy, scratch: as in mi_rollout_step_batch.
 * mi_rollout_value_batch_stack: mi_rollout_value_batch_rec on the stacked state; it never advances the history and writes neither a table of states nor older latents.
 * The mi_mlp_ forms: the same two behind the encoder chain of mi_mlp_rollout_step_batch (an MlpVAE handle goes to these only; their value form takes table_rows == NULL).
 * Errors, each under the entry's own name, before any launch, nothing written: those of the entries they extend; latent_stack < 2 or > MI_ROLLOUT_MAX_STACK; hist, lanes,
 * first or sstate NULL, n_lanes < 1, sstate not 16-byte aligned; obs_clip <= 0 or NaN with obs_mean; table_rows without its tables (MI_ERR_ARG);
 * latent_stack * z_dim + n_meas != the policy's input size; more than 1024 inputs (MI_ERR_SHAPE). */
#define MI_ROLLOUT_MAX_STACK 16
int mi_rollout_step_batch_stack(void* vae_h, void* ppo_h, void* stream, const unsigned char* frames_u8, const float* measurements, int n_meas, const float* noise, int greedy, int n, void* scratch, long long scratch_bytes, float* out, const float* obs_mean, const float* obs_inv_std, float obs_clip, const int* table_rows, long long n_table_rows, float* tab_states, float* tab_raw_states, float* tab_actions, float* tab_values, int latent_stack, float* hist, int n_lanes, const int* lanes, const int* first, int advance, float* sstate, float* older_out);
int mi_rollout_value_batch_stack(void* vae_h, void* ppo_h, void* stream, const unsigned char* frames_u8, const float* measurements, int n_meas, int n, void* scratch, long long scratch_bytes, float* out, const float* obs_mean, const float* obs_inv_std, float obs_clip, const int* table_rows, long long n_table_rows, float* tab_final_values, int latent_stack, float* hist, int n_lanes, const int* lanes, const int* first, float* sstate);
int mi_mlp_rollout_step_batch_stack(void* mlp_h, void* ppo_h, void* stream, const unsigned char* frames_u8, const float* measurements, int n_meas, const float* noise, int greedy, int n, void* scratch, long long scratch_bytes, float* out, const float* obs_mean, const float* obs_inv_std, float obs_clip, const int* table_rows, long long n_table_rows, float* tab_states, float* tab_raw_states, float* tab_actions, float* tab_values, int latent_stack, float* hist, int n_lanes, const int* lanes, const int* first, int advance, float* sstate, float* older_out);
int mi_mlp_rollout_value_batch_stack(void* mlp_h, void* ppo_h, void* stream, const unsigned char* frames_u8, const float* measurements, int n_meas, int n, void* scratch, long long scratch_bytes, float* out, const float* obs_mean, const float* obs_inv_std, float obs_clip, const int* table_rows, long long n_table_rows, float* tab_final_values, int latent_stack, float* hist, int n_lanes, const int* lanes, const int* first, float* sstate);

/* ---- collectives of the data-parallel path (no reference counterpart: the reference is single-process) ----
 * RCCL over xGMI, one communicator per process = per GPU; librccl.so.1 is bound at mi_comm_init (a single-GPU process never loads it).
 * Rendezvous: rank 0 calls mi_comm_unique_id, the mi_comm_id_bytes() = 128 bytes travel to the other ranks by any out-of-band channel, every
 * rank calls mi_comm_init (collective).  All calls below enqueue on HIP streams and never synchronise the host.
 *   mi_allreduce_sum_f32        buf <- sum over ranks, in stream order on `stream` (gradient buffer / metric accumulators)
 *   mi_allreduce_sum_f32_async  the same on the communicator's own stream, after what `stream` holds so far: a gradient bucket's all-reduce
 *                               runs under the next part of the backward pass; mi_comm_wait(comm, stream) joins before the optimiser step
 *   mi_broadcast                rank `root`'s bytes to every rank (the initial parameter replica, vae/models.py / ppo.py init_session)
 *   mi_comm_probe               binds librccl (dlopen + entry points) and nothing else: called on EVERY rank before the collective mi_comm_init so that
 *                               a rank that cannot load RCCL is agreed on while everybody can still fall back together
 *   mi_comm_set_algo            gradient-bucket schedule of this communicator: 0 = ncclAllReduce (default), 1 = reduce-scatter + all-gather (one hop per phase on the
 *                               fully connected xGMI mesh).  The SAME value on every rank: the host agrees on it first (mi355/dist.py reads
 *                               MI355_COMM_ALGO=rsag per process and takes the minimum over the ranks)
 *   mi_comm_allreduce_plan      what one all-reduce of n floats issues on a given rank under a schedule (pure function, no GPU: checked on the CPU for every rank):
 *                               out5 = {rsag?, floats per rank slice, this rank's slice offset, tail offset, tail floats} */
int mi_comm_probe(void);
/* 1: the bound RCCL offers the reduce-scatter + all-gather schedule (both entry points); the host takes the minimum over the ranks before anybody calls mi_comm_set_algo(1) */
int mi_comm_has_rsag(void);
/* A communicator that RECORDS what it would issue instead of communicating (no RCCL, no GPU; test infrastructure of the data-parallel step): log = HOST memory, 4 long long per
 * entry {op: 1 all-reduce 2 reduce-scatter 3 all-gather 4 broadcast 5 wait, floats (bytes for 4; buckets joined for 5), issued by the _async form?, buffer address}; the data is
 * left alone (the sum over one rank).  mi_comm_recorded: entries issued so far, -1 for a real communicator.  mi_comm_set_algo / mi_comm_destroy work on it as usual. */
int mi_comm_init_recording(void** comm_out, int rank, int world, long long* log, int log_capacity);
int mi_comm_recorded(void* comm);
/* round 6: the number of ranks the communicator spans as RCCL reports it (ncclCommCount); recording communicator: the world it was created for */
int mi_comm_ranks(void* comm);
int mi_comm_set_algo(void* comm, int algo);
int mi_comm_allreduce_plan(int algo, int world, int rank, long long n, long long* out5);
int mi_comm_id_bytes(void);
int mi_comm_unique_id(unsigned char* id_out);
int mi_comm_init(void** comm_out, int rank, int world, const unsigned char* id);
int mi_comm_destroy(void* comm);
int mi_allreduce_sum_f32(void* comm, void* stream, float* buf, long long n);
int mi_allreduce_sum_f32_async(void* comm, void* stream, float* buf, long long n);
int mi_comm_wait(void* comm, void* stream);
int mi_broadcast(void* comm, void* stream, void* buf, long long bytes, int root);

/* per-op timing with HIP events recorded on the launch stream (bench.py's live roofline numbers) */
int mi_vae_op_count(void);
const char* mi_vae_op_name(int op);
int mi_vae_timing_begin(void* h, int mode, int op_filter, int max_records);
int mi_vae_timing_collect(void* h, float* ms_sum, int* count, int n_ops);

/* ---- PPO engine: PolicyGraph x2 + losses + Adam (ppo.py:16-66,112-147) ---- */
int mi_ppo_desc_size(void);
int mi_ppo_tensor_count(void);
long long mi_ppo_param_floats(const MiPpoDesc* d);
int mi_ppo_param_layout(const MiPpoDesc* d, long long* offsets, long long* sizes, int n);
long long mi_ppo_workspace_bytes(const MiPpoDesc* d);
void* mi_ppo_create(const MiPpoDesc* d, float* params, float* params_old, float* grads, float* adam_m, float* adam_v, void* workspace, long long workspace_bytes, const float* action_low, const float* action_high);
void mi_ppo_destroy(void* h);
void* mi_ppo_buffer(void* h, int which);
/* PPO.update_old_policy — ppo.py:275-276 */
int mi_ppo_update_old(void* h, void* stream);
/* PPO.predict — ppo.py:231-251.  mi_ppo_buffer(h, 0): losses of the last step: [policy, value, entropy, total, mean ratio, mean action_mean[A], std[A]] (the
 * scalars of ppo.py:150-163); mi_ppo_buffer(h, 1): action_mean [M,A] of the last predict / train step; mi_ppo_buffer(h, 3): the step's workspace dv [M], the
 * gradient of the loss with respect to each sample's value-head output as the last step formed it (exactly 0 where value clipping stops it); mi_ppo_buffer(h, 5): likewise du [M, A], the gradient with respect to each sample's
 * action-mean head outputs (exactly 0 on a dual-clipped sample with the KL penalty off: mi_ppo_set_dual_clip) */
int mi_ppo_predict(void* h, void* stream, const float* states, int M, const float* noise, int greedy, float* action, float* value);
/* gradient half + optimiser half of PPO.train (= north_star "learn") — ppo.py:218-229.  Both paths of mi_ppo_forward_backward are bitwise reproducible: the
 * per-layer one (shapes outside the fused range, MI355_PPO_FUSED=0) adds the row splits of its filter and bias gradients in a fixed order (mi_gemm_wgrad_bias_ws on
 * slabs in the workspace), as the fused kernels do */
int mi_ppo_forward_backward(void* h, void* stream, const float* states, const float* actions, const float* returns, const float* advantage, int M, float inv_m, float grad_scale);
int mi_ppo_apply_adam(void* h, void* stream, float alpha, float beta1, float beta2, float epsilon);
/* PPO.train's device work in ONE call (single rank): fused forward / losses / backward / Adam, five launches — ppo.py:218-229; logp_old (optional):
 * log pi_old(a|s) of the samples from mi_ppo_logp_old, computed once per horizon batch (theta_old is constant between update_old_policy() calls) */
int mi_ppo_train_step(void* h, void* stream, const float* states, const float* actions, const float* returns, const float* advantage, const float* logp_old, int M, float inv_m, float grad_scale, float alpha, float beta1, float beta2, float epsilon);
/* the same step with the minibatch gather fused in — train.py:199-204 (`states[mb_idx]`, ...): the five operands are the horizon-batch tables (n_rows rows,
 * device resident for the whole update) and row_idx [M] (int32, device) names this minibatch's rows */
int mi_ppo_train_step_idx(void* h, void* stream, const float* states, const float* actions, const float* returns, const float* advantage, const float* logp_old, const int* row_idx, int n_rows, int M, float inv_m, float grad_scale, float alpha, float beta1, float beta2, float epsilon);
/* round 6 (ABI 7): one DATA-PARALLEL SGD step of PPO.train (ppo.py:218-229 under the minibatch loop of train.py:193-207) in ONE call: the fused chain of
 * mi_ppo_train_step[_idx] with the gradients of this rank's M rows (inv_m = 1 / M_global, grad_scale = M / M_global) left in the flat buffer, ONE all-reduce of that
 * buffer through `comm` in stream order, tf.train.AdamOptimizer.  row_idx != NULL: the operands are this rank's horizon-batch tables (n_rows rows) and the gather of
 * train.py:199-204 stays inside the kernels; row_idx == NULL: contiguous minibatch tensors. */
int mi_ppo_train_step_dp(void* h, void* comm, void* stream, const float* states, const float* actions, const float* returns, const float* advantage, const float* logp_old, const int* row_idx, int n_rows, int M, float inv_m, float grad_scale, float alpha, float beta1, float beta2, float epsilon);
/* 1: this engine's shape (1 <= num_actions <= 8, h2 <= 320 and a multiple of 4, padded input width <= 96 -- <= 1024 with mi_ppo_set_wide_inputs(h, 1 or 2)) is inside
 * the range of the fused kernels and they are switched on, i.e. mi_ppo_train_step_idx / mi_ppo_logp_old will run; 0: only the per-layer path exists for it (mi_ppo_train_step and mi_ppo_forward_backward fall
 * back by themselves; gather the minibatch on the host side instead of calling the _idx form).  Row indices are clamped into [0, n_rows) by the kernels. */
int mi_ppo_fused_shape_ok(void* h);
int mi_ppo_logp_old(void* h, void* stream, const float* states, const float* actions, int M, float* out);
/* precision of the PPO step (the GEMMs of the forward, the losses' gradients and PPO.train) — ppo.py:42-66,112-147,218-229.  dtype MI_F32 (exact fp32, the
 * default of a new engine) or MI_BF16X3: the GEMM stages of the fused kernels (layers 1-2 of the policy / value / old-policy nets, the layer-1 input gradient, the
 * weight gradients) take their fp32 operands from HBM as they are, split them in registers (hi = bf16(x), lo = bf16(x - hi)) and form hi.hi + hi.lo + lo.hi with
 * v_mfma_f32_32x32x16_bf16, fp32 accumulate; heads, losses, bias gradients, Adam and the order of every sum stay as in fp32 (bitwise reproducible run to run).
 * The mode governs mi_ppo_train_step, mi_ppo_train_step_idx, mi_ppo_train_step_dp, the fused path of mi_ppo_forward_backward and mi_ppo_logp_old (so the cached
 * log pi_old and the in-step old-policy forward come from the same kernels).  mi_ppo_predict and mi_rollout_step stay EXACT FP32 in both modes.
 * Returns MI_ERR_ARG for MI_BF16 (no bf16-storage PPO) or any other value, MI_ERR_SHAPE when mi_ppo_fused_shape_ok(h) is 0 (the split form exists only as fused
 * kernels: never a silent fp32 run).  Weights, gradients and optimiser state are fp32 in both modes; a new engine (mi_ppo_create) starts in MI_F32. */
int mi_ppo_set_precision(void* h, int dtype);
/* the engine's current precision (MI_F32 or MI_BF16X3) — ppo.py:42-66,112-147,218-229 */
int mi_ppo_precision(void* h);
/* wide inputs: which padded input widths kin = ceil(input_dim / 8) * 8 the fused kernels take -- ppo.py:16-66 with a VAE of more than 93 latents (train_vae.py
 * --z_dim 128: 131 inputs; ConvVAE's own default z_dim = 512: 515).
 *   mode 0 (the default of a new engine): kin <= 96, every launch as it always was; a wider policy runs the per-layer path, on which mi_ppo_train_step_idx,
 *          _vclip, _kl, mi_ppo_old_policy_cache, mi_ppo_logp_old, mi_ppo_update_stats_idx, mi_ppo_kl_stats_idx, mi_ppo_values_idx and MI_BF16X3 return MI_ERR_SHAPE;
 *   mode 1: kin <= 1024; layer 1 of an engine with kin > 96 runs as ppo_l1_wide_kernel (the four waves of a block split K and meet in LDS in a fixed order: no
 *          atomics, two runs bitwise equal; a state entry at or past input_dim counts as 0.0 whatever the table holds there), every launch behind it is the one
 *          the narrow range takes; an engine with kin <= 96 takes the launches of mode 0 bit for bit;
 *   mode 2: kin <= 1024 with ppo_l1_kernel at every width (one wave walks the whole K; like mode 0 it reads up to 7 entries of the table row BEHIND a gathered
 *          row against zero weights, so those must be finite) -- kept for measuring mode 1 against (tools/ppo_wide_bench.py).
 * The other limits stay: 1 <= num_actions <= 8, h2 <= 320 and a multiple of 4.  The setting changes routing only -- the parameter layout (kin rows of W1, the
 * last kin - input_dim of them zero, and zero in both Adam slots) is the same on every path -- so it may be switched between two steps, and it is no part of a
 * checkpoint.  mi_ppo_fused_shape_ok reports the result.
 * 2 GiB limit (every mode): the fused kernels address a state table through 32-bit byte offsets, so every fused entry returns MI_ERR_SHAPE and launches nothing
 * when n_rows * input_dim * 4 >= 2^31 (a table handed over with row_idx: 1.04 M rows at 515 inputs; without row_idx the M rows of the call) or
 * max_batch * kin * 4 >= 2^31.
 * MI_ERR_ARG: mode outside 0..2; MI_ERR_SHAPE: mode 0 on an engine in MI_BF16X3 whose kin exceeds 96 (the split form has no per-layer path). */
int mi_ppo_set_wide_inputs(void* h, int mode);
/* the engine's mode (0, 1 or 2) */
int mi_ppo_wide_inputs(void* h);
/* per-epoch update diagnostics: how far the CURRENT policy theta has moved from the old one on M rows of the horizon-batch tables, and how well the value net
 * fits the returns -- one forward-only pass (policy and value trunks of theta in the engine's precision mode, one head kernel, one ordered reduction; four
 * launches, no backward, no optimiser).  Sample m is row row_idx[m] (int32, device; clamped into [0, n_rows)) of states / actions / returns / logp_old, gathered
 * inside the kernels as in mi_ppo_train_step_idx; 1 <= M <= max_batch.  logp_old is the cache mi_ppo_logp_old filled: log pi_old(a|s) per table row.  Per sample
 *   lp = log pi(a|s) under theta (fp32, the arithmetic and summation order of mi_ppo_logp_old: with theta == theta_old it equals logp_old bit for bit),
 *   v = h2_v Wv + bv (fp32), and in double precision  d = lp - logp_old,  r = exp(d),  ret = returns[row];
 * stats [MI_PPO_N_STATS] (double, device) receives the sums over the M samples of
 *   [0] 1 (the count)   [1] d   [2] r - 1 - d   [3] 1 where |r - 1| > clip_eps (the engine's), else 0   [4] r   [5] ret   [6] ret^2   [7] ret - v   [8] (ret - v)^2
 * so that [2] / [0] is the k3 estimator of KL(pi_old || pi), the mean of r - 1 - log r; -[1] / [0] the k1 estimator; [3] / [0] the clipped fraction; [4] / [0] the
 * mean ratio; [8] / [0] the value error; 1 - Var(ret - v) / Var(ret) from [5]..[8] the explained variance.  The reduction is ordered (no atomics): every block of
 * 32 samples stores its partial sums to scratch (mi_ppo_update_stats_scratch_doubles(M) doubles, device), one wave adds them in block order; two runs on the same
 * inputs give bitwise equal stats.  accumulate 0: stats is overwritten; accumulate 1: the sums are added to what stats holds -- a caller covers more than
 * max_batch rows as a chain of calls, the first with 0.  logp_new_out / value_out (each may be NULL): tables of n_rows floats, lp / v of sample m goes to entry
 * row_idx[m], every other entry is left alone.  NOT modified: parameters, theta_old, the optimiser state, the gradient buffer, the losses and action_mean buffers
 * (mi_ppo_buffer) -- only the engine's activation workspace, scratch, stats and the two optional tables are written.  A row that row_idx does not name is not
 * read, except that layer 1 (as in mi_ppo_train_step_idx) reads the first few state entries of the table row behind a named one against zero weights: those must
 * be finite.  MI_ERR_STATE: null handle; MI_ERR_ARG: M outside [1, max_batch], n_rows < 1, a missing buffer (named in the message), accumulate not 0 / 1;
 * MI_ERR_SHAPE: mi_ppo_fused_shape_ok(h) is 0 (there is no per-layer form of this pass). */
#define MI_PPO_N_STATS 9
long long mi_ppo_update_stats_scratch_doubles(int M);
int mi_ppo_update_stats_idx(void* h, void* stream, const float* states, const float* actions, const float* returns, const float* logp_old, const int* row_idx, int n_rows, int M, int accumulate, double* scratch, double* stats, float* logp_new_out, float* value_out);
/* global-norm gradient clipping in front of the optimiser (tf.clip_by_global_norm; the `max_grad_norm` of other PPO implementations) -- ppo.py:143-144.  With a
 * limit c the order of operations of an optimiser step is:
 *   sumsq = sum of (double)g * (double)g over every element of the 13 policy/ variables of the gradient buffer -- the variables, not the flat buffer: the alignment
 *           gaps behind the tensors whose size is no multiple of 8 (action bias, action_logstd, value bias) may hold anything and do not count --
 *   norm  = sqrt(sumsq) in double;   scale = (float)(c / norm) where norm is finite and norm > (double)c, else 1.0f (so c = +inf measures and never clips, and a
 *           non-finite norm leaves the gradient as it is and is reported as it is);
 *   g'    = g * scale, rounded to fp32, and g' goes through the TF ApplyAdam arithmetic of mi_ppo_apply_adam unchanged:
 * a clipped step equals multiplying the gradient buffer by scale in fp32 and then calling mi_ppo_apply_adam with clipping off, bit for bit.  The sum is ordered
 * (one kernel stores one double per block, the optimiser kernel adds them in block order, the same order in every block): no atomics, and two runs on the same
 * gradients give bitwise equal results.  Two launches (sum of squares, Adam) in place of the one Adam launch.
 * mi_ppo_set_max_grad_norm: max_norm 0 switches clipping off (the default of a new engine), > 0 or +inf switches it on; MI_ERR_ARG for a negative value or NaN,
 * MI_ERR_STATE for a null handle.  With clipping on, mi_ppo_apply_adam clips, and mi_ppo_train_step / mi_ppo_train_step_idx take, for every M, the route they take
 * above 256 rows (the fused chain with the gradients left in the flat buffer, then mi_ppo_apply_adam) instead of applying Adam inside the gradient kernels;
 * mi_ppo_train_step_dp clips behind its all-reduce, so every rank forms the same factor.  The gradient buffer is zero after the step, gaps included.  With
 * clipping off every entry makes exactly the launches it made before.  Both precision modes.  mi_ppo_buffer(h, 2): four floats {norm, scale, c, 0} of the last
 * norm that was formed (zeros in a new engine); NOT written while clipping is off.
 * mi_ppo_max_grad_norm: the current setting (0 = off); -1 for a null handle.
 * mi_ppo_grad_norm: the building block alone -- the norm of the gradient buffer as it stands (e.g. behind mi_ppo_forward_backward) and the factor that max_norm
 * (> 0 or +inf; MI_ERR_ARG otherwise) gives, left in mi_ppo_buffer(h, 2); two launches.  NOT modified: parameters, theta_old, the optimiser state, the gradient
 * buffer, the losses and action_mean buffers, the engine's setting. */
int mi_ppo_set_max_grad_norm(void* h, float max_norm);
float mi_ppo_max_grad_norm(void* h);
int mi_ppo_grad_norm(void* h, void* stream, float max_norm);
/* Dual-clip PPO (Ye et al. 2020, "Mastering Complex Control in MOBA Games with Deep Reinforcement Learning", eq. 5): a bound on the one side the clipped
 * surrogate leaves open.  With r = pi_theta / pi_old, A the advantage, eps = clip_eps, s = min(r A, clamp(r, 1 - eps, 1 + eps) A) the surrogate of ppo.py:112-132
 * and a constant c > 1, the per-sample surrogate of the fused head / loss kernel becomes
 *   s' = (A < 0 && c A > s) ? c A : s                      tf.maximum(s, c A) on the samples with A < 0: on a tie s keeps the gradient
 * A sample in the first branch is "dual-clipped": c A does not depend on theta, so its surrogate contributes exactly 0.0 to du and to dlogstd (dr = 0, as on the
 * clipped branch), and the policy-loss partial takes c A.  A sample with A >= 0, -0.0 included, never takes the branch.  The KL penalty's own gradient terms, the
 * value side, the entropy term and demonstration rows are not touched.  c = +inf never takes the branch: every stored bit equals the plain step's.
 * mi_ppo_set_dual_clip: c = 0 switches the setting off (the default of a new engine), c > 1 -- finite or +inf -- switches it on; anything else (NaN, a negative
 * value, a value in (0, 1]) is MI_ERR_ARG and leaves the setting as it was; MI_ERR_STATE for a null handle.  Handle state, like mi_ppo_set_max_grad_norm.  On,
 * every fused step entry uses it -- mi_ppo_train_step / _idx / _dp / _vclip / _kl / _demo and mi_ppo_forward_backward where it runs the fused chain -- with the
 * launches, routes and reproducibility of the plain step, in both precision modes; mi_ppo_clone_step has no ratio and ignores it.  The per-layer path has no dual
 * clip: with the setting on, an engine for which mi_ppo_fused_shape_ok(h) is 0 refuses mi_ppo_forward_backward (and mi_ppo_train_step / _dp, which run it) with
 * MI_ERR_SHAPE in front of the first launch, nothing written -- the way it refuses MI_BF16X3.  (mi_ppo_loss_fwd_bwd, the per-layer loss kernel, takes no handle and
 * has no dual-clip argument.)
 * mi_ppo_dual_clip: the current setting (0 = off); -1 for a null handle.
 * mi_ppo_set_loss_coefs: replaces the descriptor's clip_eps, value_scale and entropy_scale on a live engine -- a clip-range or entropy-coefficient schedule without
 * giving up the optimiser state.  Every later call reads the new values: the steps, mi_ppo_update_stats_idx's clipped fraction, the per-layer path.  clip_eps finite
 * and > 0, value_scale and entropy_scale finite and >= 0; anything else is MI_ERR_ARG and changes nothing.  mi_ppo_loss_coefs fills the three current values.
 * mi_ppo_dual_clip_stats: the diagnostics, without an engine, in the mould of mi_ppo_value_clip_stats: over the M rows row_idx[m] (int32, device; clamped into
 * [0, n_rows)) of three fp32 tables -- logp_new (log pi_theta(a | s): the logp_new_out table mi_ppo_update_stats_idx writes), logp_old (the cached log pi_old),
 * advantage (the table the steps gathered from) -- the sums
 *   [0] 1 (the count)   [1] 1 where A < 0   [2] 1 where the sample is dual-clipped   [3] s'   [4] s
 * into stats [MI_PPO_N_DUAL_CLIP_STATS] (double, device).  A sample's class is formed in fp32 exactly as the step forms it (r = __expf(lp - lp_old), then the
 * step's operations), so the counts say what a step on these tables does; the sums [3] and [4] are formed in double from the fp32 inputs.  dual_clip > 1 or +inf,
 * clip_eps finite and > 0.  Ordered: every block of 256 samples stores its sums to scratch (mi_ppo_dual_clip_stats_scratch_doubles(M) doubles, device), one wave
 * adds them in block order; no atomics, two runs are bitwise equal.  accumulate 0: stats is overwritten, 1: added to.  Rows not named are not read; nothing but
 * scratch and stats is written.  MI_ERR_ARG: M < 1, n_rows < 1, a missing buffer, clip_eps or dual_clip outside their ranges, accumulate not 0 / 1. */
#define MI_PPO_N_DUAL_CLIP_STATS 5
int mi_ppo_set_dual_clip(void* h, float c);
float mi_ppo_dual_clip(void* h);
int mi_ppo_set_loss_coefs(void* h, float clip_eps, float value_scale, float entropy_scale);
int mi_ppo_loss_coefs(void* h, float* clip_eps, float* value_scale, float* entropy_scale);
long long mi_ppo_dual_clip_stats_scratch_doubles(int M);
int mi_ppo_dual_clip_stats(void* stream, const float* logp_new, const float* logp_old, const float* advantage, const int* row_idx, int n_rows, int M, float clip_eps, float dual_clip, int accumulate, double* scratch, double* stats);
/* PPO2-style value-function clipping (the clipped value loss of baselines ppo2; clip_vloss / clip_range_vf of other PPO implementations) -- the value term of
 * ppo.py:112-132.  Per sample, with V the value head's output under theta, V_old = old_values[row] the value recorded when the data was collected, R the return and
 * eps_v = clip_range_vf > 0:
 *   V_c  = min(max(V, V_old - eps_v), V_old + eps_v)     a clamp of V itself, so V_c == V bit for bit inside the range
 *   l_u  = (V - R)^2 ,  l_c = (V_c - R)^2
 *   value_loss = value_scale * mean(max(l_u, l_c))        the max form of baselines ppo2, not the V_c-only form
 *   dLoss/dV   = (l_c > l_u) ? 0 : 2 * value_scale * (V - R) / M_global
 * i.e. tf.maximum(l_u, l_c) over tf.clip_by_value: on a tie the gradient goes to the first argument; inside the range and at its edge both terms are the same
 * number, so the plain gradient flows, and the clipped branch is chosen only outside the range, where its slope is 0.  eps_v = +inf gives the unclipped step bit
 * for bit.  losses[1] (value_loss, mi_ppo_buffer(h, 0)) of a clipped step is the clipped objective.  Nothing on the policy side changes.
 * mi_ppo_train_step_vclip is ONE entry for the three unclipped forms: row_idx == NULL: contiguous minibatch tensors (n_rows ignored) as mi_ppo_train_step;
 * row_idx != NULL: states / actions / returns / advantage / logp_old and old_values are horizon-batch tables of n_rows rows gathered inside the kernels (rows
 * clamped) as mi_ppo_train_step_idx -- V_old is one more 4-byte gather per sample in the head / loss kernel, rows that row_idx does not name are not read; comm !=
 * NULL: one all-reduce of the flat gradient buffer in front of Adam as mi_ppo_train_step_dp.  logp_old may be NULL (the old policy's forward runs in the step).
 * adam == 0: the step stops with the gradients in the flat buffer (the role of mi_ppo_forward_backward; no all-reduce, no optimiser); adam == 1: the routes the
 * existing entries take -- Adam inside the gradient kernels for M <= 256 with mi_ppo_set_max_grad_norm off and no communicator, else the flat buffer and
 * mi_ppo_apply_adam (which clips by the global norm when that is on).  The same launches as the unclipped step, no atomics, bitwise reproducible, both precision
 * modes.  MI_ERR_STATE: null handle; MI_ERR_ARG: M outside [1, max_batch], row_idx set with n_rows < 1, old_values == NULL (an unclipped step: the existing
 * entries), clip_range_vf not > 0 (NaN included), adam not 0 / 1; MI_ERR_SHAPE: mi_ppo_fused_shape_ok(h) is 0 (there is no per-layer form).
 * mi_ppo_value_clip_stats: the diagnostics of it, without an engine: over the M rows row_idx[m] (int32, device; clamped into [0, n_rows)) of three fp32 tables --
 * values_new (V under the current parameters: the value_out table mi_ppo_update_stats_idx writes), old_values, returns -- the sums, formed in double from the fp32
 * inputs, of
 *   [0] 1 (the count)   [1] 1 where |V - V_old| > eps_v   [2] max(l_u, l_c)   [3] 1 where l_c > l_u (no value gradient from this sample)
 * into stats [MI_PPO_N_VCLIP_STATS] (double, device).  Ordered: every block of 256 samples stores its sums to scratch
 * (mi_ppo_value_clip_stats_scratch_doubles(M) doubles, device), one wave adds them in block order; no atomics, two runs are bitwise equal.  accumulate 0: stats is
 * overwritten, 1: added to.  Rows not named are not read; nothing but scratch and stats is written.  MI_ERR_ARG: M < 1, n_rows < 1, a missing buffer,
 * clip_range_vf not > 0, accumulate not 0 / 1. */
#define MI_PPO_N_VCLIP_STATS 4
int mi_ppo_train_step_vclip(void* h, void* comm, void* stream, const float* states, const float* actions, const float* returns, const float* advantage, const float* logp_old, const float* old_values, float clip_range_vf, const int* row_idx, int n_rows, int M, float inv_m, float grad_scale, int adam, float alpha, float beta1, float beta2, float epsilon);
long long mi_ppo_value_clip_stats_scratch_doubles(int M);
int mi_ppo_value_clip_stats(void* stream, const float* values_new, const float* old_values, const float* returns, const int* row_idx, int n_rows, int M, float clip_range_vf, int accumulate, double* scratch, double* stats);
/* adaptive KL penalty: the other objective of the PPO paper (Schulman et al. 2017, section 4), the KL-penalised surrogate, ADDED to the clipped surrogate (the clip
 * stays as configured; RLlib runs both by default).  Direction: KL(pi_old || pi_theta), as in the paper.  For the diagonal Gaussian policy it is a closed form of the
 * means and log-stds, so it enters the loss exactly.  Per sample m and action a, with ls / lso the current / old action_logstd, mu / mu_o the current / old action
 * means (after the low + (tanh(u) + 1) / 2 (high - low) map), d = ls - lso, D = mu - mu_o, sigma = exp(ls):
 *   KL[m,a]  = d + expm1(-2 d) / 2 + D^2 / (2 sigma^2)        (= ls - lso + (sigma_o^2 + D^2) / (2 sigma^2) - 1/2, spelled without the cancellation)
 *   KL[m]    = sum_a KL[m,a]
 *   loss     = -policy_loss + value_loss - entropy_loss + beta * mean_m KL[m]
 *   dKL/dmu  = D / sigma^2                   -> du[m,a]    += beta * inv_m * (D / sigma^2) * (high - low) / 2 * (1 - t^2)
 *   dKL/dls  = -expm1(-2 d) - D^2 / sigma^2  -> dlogstd[a] += beta * inv_m * sum_m (...)
 * The value side and the entropy term are untouched.  The ls part is state independent but is summed per sample with inv_m = 1 / M_global, so under data parallelism
 * it needs no grad_scale (unlike the entropy term).  beta = kl_coef, a finite float >= 0; 0 runs the penalised kernel as measure-only (the KL slot is filled, nothing
 * is added: parameters, optimiser state and the five loss scalars are those of the unpenalised step).  The losses buffer (mi_ppo_buffer(h, 0)) gains two floats
 * behind the 5 + 2 A defined above: [5 + 2 A] mean_m KL[m] and [5 + 2 A + 1] beta times that, which losses[3] (total) also takes.  Only this entry writes them.
 * mi_ppo_old_policy_cache: mi_ppo_logp_old that keeps the old policy's means -- logp_out [M] (bit for bit what mi_ppo_logp_old gives) and mean_out [M, A].
 * mi_ppo_train_step_kl: ONE entry for every form, as mi_ppo_train_step_vclip: row_idx NULL (contiguous minibatch tensors, n_rows ignored) or the in-kernel gather
 * from tables of n_rows rows (mean_old [n_rows, A] and logp_old among them; rows clamped; mu_o is one more 4-byte gather per (sample, action) in the head / loss
 * kernel, rows that row_idx does not name are not read); comm NULL or a communicator (one all-reduce in front of Adam); adam 0 (the gradients stay in the flat
 * buffer) or 1 (Adam inside the gradient kernels for M <= 256 with no communicator and mi_ppo_set_max_grad_norm off, else the flat buffer and mi_ppo_apply_adam).
 * logp_old and mean_old are both NULL (the step evaluates the old policy itself, and forms mu_o as the cache does: the same step either way) or both given.
 * old_values NULL: the plain value loss; else the value term is clipped with clip_range_vf exactly as mi_ppo_train_step_vclip does.  The same launches as the
 * unpenalised step, a fixed summation order, no atomics, both precision modes.  MI_ERR_STATE: null handle; MI_ERR_ARG: M outside [1, max_batch], row_idx set with
 * n_rows < 1, one of logp_old / mean_old without the other, kl_coef negative, NaN or infinite, old_values with clip_range_vf not > 0, adam not 0 / 1; MI_ERR_SHAPE:
 * mi_ppo_fused_shape_ok(h) is 0 (there is no per-layer form; nothing is written).
 * mi_ppo_kl_stats_idx: the exact KL of M rows row_idx[m] (int32, device; clamped into [0, n_rows)) of the tables states / mean_old under the CURRENT theta --
 * forward only (the policy trunk in the engine's precision mode, one head kernel, one ordered reduction).  The means are fp32 (this pass: the arithmetic of
 * mi_ppo_old_policy_cache, so theta == theta_old gives KL = 0 exactly), the KL per sample is formed in double from them and the two log-stds.  stats
 * [MI_PPO_N_KL_STATS] (double, device) receives the sums of
 *   [0] 1 (the count)   [1] KL[m]   [2] KL[m]^2   [3] sum_a D^2 / (2 sigma^2) (the mean part of the KL)
 * Ordered like mi_ppo_update_stats_idx: a scratch row per block of 32 samples (mi_ppo_kl_stats_scratch_doubles(M) doubles), one wave adds them in block order; two
 * runs are bitwise equal; accumulate 0 / 1 as there.  NOT modified: parameters, theta_old, optimiser state, gradient buffer, the losses and action_mean buffers.
 * MI_ERR_ARG: M outside [1, max_batch], n_rows < 1, a missing buffer, accumulate not 0 / 1; MI_ERR_SHAPE: mi_ppo_fused_shape_ok(h) is 0. */
#define MI_PPO_N_KL_STATS 4
int mi_ppo_old_policy_cache(void* h, void* stream, const float* states, const float* actions, int M, float* logp_out, float* mean_out);
int mi_ppo_train_step_kl(void* h, void* comm, void* stream, const float* states, const float* actions, const float* returns, const float* advantage, const float* logp_old, const float* mean_old, float kl_coef, const float* old_values, float clip_range_vf, const int* row_idx, int n_rows, int M, float inv_m, float grad_scale, int adam, float alpha, float beta1, float beta2, float epsilon);
long long mi_ppo_kl_stats_scratch_doubles(int M);
int mi_ppo_kl_stats_idx(void* h, void* stream, const float* states, const float* mean_old, const int* row_idx, int n_rows, int M, int accumulate, double* scratch, double* stats);
/* values of table rows: V(s) under the CURRENT theta for M rows of a state table of n_rows rows -- the forward-only value pass the rollout buffers recompute their
 * advantages from before every later epoch of an update (Andrychowicz et al. 2021, "What Matters in On-Policy RL").  Only the value net runs: layers 1 - 2 of it
 * (the narrow or the wide layer-1 form, as mi_ppo_set_wide_inputs selects; the engine's precision mode, as mi_ppo_update_stats_idx) and one value head kernel --
 * three launches per chunk, no policy trunk, no reduction, no scratch, no atomics; two runs give bitwise equal tables.
 * Sample m is row row_idx[m] (int32, device) of `states`, or row m with row_idx == NULL (then M <= n_rows).  Its value goes to values_out[row_idx[m]] (values_out[m]
 * without a list): values_out is a table of n_rows floats laid out like the rollout buffers' other tables, and an entry no sample names is left alone.  A row that
 * is negative or >= n_rows stores NOTHING (its loads are clamped into the table as in mi_ppo_train_step_idx; unlike mi_ppo_update_stats_idx, which clamps the store
 * as well).  The stored value is bit for bit what value_out of mi_ppo_update_stats_idx holds for the same row and parameters.
 * M may exceed the engine's max_batch: the entry walks chunks of max_batch rows itself (the last one partial), so a caller makes one call per table.
 * NOT modified: parameters, theta_old, the optimiser state, the gradient buffer, the losses and action_mean buffers -- only the engine's activation workspace and
 * values_out are written.  Like the other gathering entries layer 1 reads the first few state entries behind a named row against zero weights (narrow form): those
 * must be finite.  Every refusal comes before the first launch and writes nothing; those that need no engine come first: MI_ERR_ARG: M < 1, n_rows < 1, states or
 * values_out NULL, row_idx == NULL with M > n_rows; then MI_ERR_STATE: null handle; MI_ERR_SHAPE: mi_ppo_fused_shape_ok(h) is 0 (there is no per-layer form), or the
 * 2 GiB limit stated at mi_ppo_set_wide_inputs. */
int mi_ppo_values_idx(void* h, void* stream, const float* states, const int* row_idx, long long n_rows, long long M, float* values_out);
/* log-probabilities of table rows: log pi_theta(a | s) under the CURRENT theta for M rows of the tables `states` / `actions` of n_rows rows -- the twin of
 * mi_ppo_values_idx for the policy side, the forward-only pass the rollout buffers form their V-trace importance weights from (mi_rollout_finish_vtrace).  Only
 * the policy net runs: layers 1 - 2 of it (the narrow or the wide layer-1 form, as mi_ppo_set_wide_inputs selects; the engine's precision mode, as
 * mi_ppo_update_stats_idx) and one head kernel -- three launches per chunk, no value trunk, no statistics, no reduction, no scratch, no LDS, no atomics; two runs
 * give bitwise equal tables.
 * Sample m is row row_idx[m] (int32, device) of `states` and of `actions` [n_rows, num_actions], or row m with row_idx == NULL (then M <= n_rows).  Its result goes
 * to logp_out[that row]: logp_out is a table of n_rows floats, and an entry no sample names is left alone.  A row that is negative or >= n_rows stores NOTHING (its
 * loads are clamped into the tables).  The stored float is bit for bit logp_new_out of mi_ppo_update_stats_idx for the same row and parameters, and with
 * theta == theta_old the cache mi_ppo_logp_old fills (csrc/ppo_head.hpp, the fifth contract).
 * M may exceed the engine's max_batch: the entry walks chunks of max_batch rows itself.
 * NOT modified: parameters, theta_old, the optimiser state, the gradient buffer, the losses and action_mean buffers -- only the engine's activation workspace and
 * logp_out are written.  The finiteness rule of mi_ppo_values_idx for the state entries behind a named row holds here too.  Every refusal comes before the first
 * launch and writes nothing; those that need no engine come first: MI_ERR_ARG: M < 1, n_rows < 1, states, actions or logp_out NULL, row_idx == NULL with
 * M > n_rows; then MI_ERR_STATE: null handle; MI_ERR_SHAPE: mi_ppo_fused_shape_ok(h) is 0 (there is no per-layer form), or the 2 GiB limit stated at
 * mi_ppo_set_wide_inputs. */
int mi_ppo_logp_idx(void* h, void* stream, const float* states, const float* actions, const int* row_idx, long long n_rows, long long M, float* logp_out);
/* behaviour cloning: one supervised step of the policy (and optionally the value net) on (state, expert action[, return]) rows -- the warm start from demonstrations
 * in front of PPO.  The fused chain of the minibatch step with a head / loss kernel of its own (csrc/ppo_fused.hip, ppo_head_clone_kernel); no old policy, no
 * advantage, no ratio, no clip, no entropy term.  Per sample m and action a, with t = tanh(u), mean = lo + (t + 1) / 2 (hi - lo), sigma = exp(logstd[a]),
 * a_E the expert's action, z = (a_E - mean) / sigma:
 *   kind 0 ("nll"): l[m] = sum_a (z^2 / 2 + logstd[a] + log(2 pi) / 2)      dl/du = -(z / sigma) (hi - lo) / 2 (1 - t^2)      dl/dlogstd[a] = 1 - z^2
 *   kind 1 ("mse"): l[m] = sum_a (mean - a_E)^2                            dl/du = 2 (mean - a_E) (hi - lo) / 2 (1 - t^2)    dl/dlogstd = 0 exactly
 *   with returns:   value_loss = value_scale mean_m (V - R)^2 ,  dV = 2 value_scale (V - R) inv_m       (the value side of the PPO step, operation for operation)
 *   clone_loss = inv_m sum_m l[m] ,  loss = clone_loss + value_loss
 * returns NULL is the policy-only form: the value net is not run, and its parameters and both of its Adam slots are bitwise unchanged on every route (the in-tile
 * Adam, the flat buffer + Adam over the policy's prefix of it, clipping, a communicator, M > 256); with adam = 0 the value net's range of the gradient buffer is
 * exactly 0.0.  One entry for every form, as mi_ppo_train_step_kl: row_idx NULL (contiguous tensors, n_rows ignored) or states / expert_actions / returns are tables
 * of n_rows rows gathered in-kernel (rows clamped; rows that row_idx does not name are not read); comm NULL or a communicator; adam 0 / 1 on the routes of
 * mi_ppo_train_step_kl.  Both precision modes; wide inputs as mi_ppo_set_wide_inputs routes them.  The losses buffer (mi_ppo_buffer(h, 0)) holds
 *   [0] clone_loss   [1] value_loss (0 without returns)   [2] 0   [3] loss   [4] mean_sq_error = mean_m sum_a (mean - a_E)^2 (in both kinds)
 * and behind them the mean action_mean [A] and std [A] as after every step.  MI_ERR_STATE: null handle, missing gradient / optimiser buffers; MI_ERR_ARG: M outside
 * [1, max_batch], row_idx set with n_rows < 1, states or expert_actions NULL, kind not 0 / 1, adam not 0 / 1; MI_ERR_SHAPE: mi_ppo_fused_shape_ok(h) is 0 (there is
 * no per-layer form).  A refused call writes nothing. */
int mi_ppo_clone_step(void* h, void* comm, void* stream, const float* states, const float* expert_actions, const float* returns, int kind, const int* row_idx, int n_rows, int M, float inv_m, float grad_scale, int adam, float alpha, float beta1, float beta2, float epsilon);
/* the PPO step with a demonstration term: M PPO rows and M_demo demonstration rows in ONE step -- one fused chain over M + M_demo rows (a staging launch that gathers
 * the state rows of the two tables, the trunks, a head / loss kernel that takes the PPO or the clone arithmetic per sample, the layer-1 input gradient, the weight
 * gradients), one gradient, one Adam update -- where mi_ppo_train_step_kl followed by mi_ppo_clone_step is two chains and two optimiser steps.
 *   loss = L_ppo(PPO rows) + demo_coef L_demo(demonstration rows)
 * L_ppo: the objective of mi_ppo_train_step[_idx] on the PPO rows with inv_m = 1 / M(global); old_values given: the clipped value loss of mi_ppo_train_step_vclip;
 * kl_on = 1: the KL penalty of mi_ppo_train_step_kl (kl_coef a finite float >= 0) and logp_old / mean_old both given or both NULL; kl_on = 0: mean_old is not read.
 * L_demo: clone_loss of mi_ppo_clone_step, demo_kind 0 ("nll") or 1 ("mse"), policy only, the same per-sample formulas with inv_m_demo = 1 / M_demo(global).
 * Demonstration rows carry no return, advantage, old policy or value target: their dv (mi_ppo_buffer(h, 3), rows M .. M + M_demo - 1) is exactly 0.0, and they add
 * nothing to the entropy and KL terms nor to the scalars of the losses buffer, mean action_mean among them (those stay means over the PPO rows; grad_scale is the PPO
 * rows').  Global-norm clipping sees the whole gradient.  row_idx NULL: contiguous PPO tensors, else the PPO tables of n_rows rows gathered in-kernel; demo_row_idx
 * NULL: demo_states [M_demo, input_dim] / demo_actions [M_demo, A] contiguous, else tables of n_demo_rows rows; the two sides gather from different tables, rows are
 * clamped and a row no list names is never read.  comm NULL or a communicator; adam 0 / 1 on the routes of mi_ppo_train_step_kl with M + M_demo in the place of M (the
 * in-tile Adam only when M + M_demo <= 256 with clipping off and no communicator).  Both precision modes; wide inputs as mi_ppo_set_wide_inputs routes them.
 * mi_ppo_buffer(h, 4): three floats [demo_loss, demo_coef x demo_loss, mean_sq_error] of the demonstration rows; losses[3] includes the weighted term.  All sums in a
 * fixed order, no atomics: two runs are bitwise equal.  MI_ERR_STATE: null handle, missing gradient / optimiser buffers; MI_ERR_ARG: M or M_demo < 1, M + M_demo >
 * max_batch, a row list with an empty table, a missing buffer, demo_kind not 0 / 1, demo_coef negative / NaN / infinite, inv_m_demo not > 0, kl_on not 0 / 1 and the
 * argument checks of mi_ppo_train_step_kl; MI_ERR_SHAPE: mi_ppo_fused_shape_ok(h) is 0 (there is no per-layer form).  A refused call writes nothing. */
int mi_ppo_train_step_demo(void* h, void* comm, void* stream, const float* states, const float* actions, const float* returns, const float* advantage, const float* logp_old, const float* mean_old, int kl_on, float kl_coef, const float* old_values, float clip_range_vf, const int* row_idx, int n_rows, int M, const float* demo_states, const float* demo_actions, const int* demo_row_idx, int n_demo_rows, int M_demo, int demo_kind, float demo_coef, float inv_m_demo, float inv_m, float grad_scale, int adam, float alpha, float beta1, float beta2, float epsilon);
/* advantages normalised PER MINIBATCH, inside the SGD loop — SB3's normalize_advantage, CleanRL's norm_adv; no reference counterpart in train.py, which normalises per
 * trajectory (train.py:176-177): one pass per epoch between the finish calls (mi_rollout_finish*, which leave the raw advantages in fp64) and the epoch's SGD steps, which
 * gather their advantage from an fp32 table by row index.  No engine handle.  adv_raw: fp64 [num_envs, T], the raw advantages (entries beyond a lane's length may hold
 * NaN); perm: int32 [n], table rows e (T + 1) + t = slot t of lane e, the epoch's shuffled rows in the order the steps take them; tab_adv_out: fp32 [num_envs (T + 1)],
 * the layout of the advantages table; stats: fp64 [n_mb, 3] with n_mb = ceil(n / batch_size) (all device).  Minibatch b is perm[b batch_size .. min((b + 1) batch_size, n)).
 * An entry that names no step slot -- row < 0, row >= num_envs (T + 1), slot == T (a lane's bootstrap slot) -- is skipped: it does not count and nothing is written for
 * it (the rule of the finish calls' segment descriptors for a one-step segment).  Over the c counted entries a of minibatch b, in fp64:
 *   mean = sum(a) / c;   ss = sum((a - mean)^2)  (two passes);   std = (c - ddof >= 1) ? sqrt(ss / (c - ddof)) : 0.0
 *   tab_adv_out[row] = (float)((a - mean) / (std + 1e-8))   (a true division, round to nearest even; the + 1e-8 of mi_adv_normalize)
 *   stats[b] = {c, mean, std};  c == 0: stats[b] = {0, 0, 0} and nothing else is written
 * ddof = 0: the population std the finish calls use; ddof = 1: the sample std (torch's .std(), what SB3 / CleanRL compute).  A one-sample minibatch has std 0 with
 * either and its entry becomes 0.0; equal advantages give exactly 0.0 wherever their sum is exact (mean == a).  One launch, one block per minibatch; the gathered
 * doubles are read from global memory again in each of the three passes (no LDS is sized by the minibatch, which can be the whole collection).  Every sum in ONE
 * order: thread i of the block's 256 adds positions i, i + 256, .. of the minibatch from the first, a wave reduction (xor tree of shuffles) inside each of the four
 * waves, the waves' partials added in wave order by one thread; no floating-point atomics: two calls are bitwise equal.  Rows that perm does not name are neither read
 * from adv_raw nor written in tab_adv_out; perm and adv_raw are not written.  A row named twice inside one call is stored twice (by its minibatches, in no order).
 * mi_ppo_minibatch_advantages_stats_doubles(n, batch_size) = 3 ceil(n / batch_size), the doubles of `stats` (needs no GPU; -1 for n < 1 or batch_size < 1).
 * Errors (MI_ERR_ARG, checked before the launch, nothing is written; the message names the argument): adv_raw, perm, tab_adv_out or stats missing; n < 1;
 * batch_size < 1; num_envs < 1 or > MI_ROLLOUT_MAX_ENVS; T < 1 or > MI_ROLLOUT_MAX_HORIZON; ddof outside {0, 1}. */
long long mi_ppo_minibatch_advantages_stats_doubles(int n, int batch_size);
int mi_ppo_minibatch_advantages(void* stream, const double* adv_raw, const int* perm, int n, int batch_size, int num_envs, int T, int ddof, float* tab_adv_out, double* stats);

#ifdef __cplusplus
}
#endif
#endif /* MI355_CARLA_H */

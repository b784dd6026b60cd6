/*
 * nst_hip.h — C ABI of libnst_hip.so, the MI355X (gfx950) stylization engine.
 *
 * Drop-in boundary for the reference's per-frame stylization hot path
 * (TrentMahaffey/NeuralStyleTransferV1).  The reference is pure Python/PyTorch;
 * the interfaces these entry points replace are Python call sites, cited per
 * function below.  Plain pointers and sizes only: no torch types cross this ABI.
 * Device pointers are HIP device pointers (e.g. a PyTorch-ROCm tensor's
 * data_ptr()); `stream` is a hipStream_t passed as void* (NULL = default stream).
 *
 * Ownership: the caller owns every input/output/workspace buffer; a handle owns
 * its packed weights (device) and nothing else.  No entry point allocates device
 * memory except nst_create / nst_lab_create (one-time packing/uploads).
 * Threading: calls on one handle must be serialised on one stream; handles on
 * different devices may be used concurrently from different threads/processes.
 * Errors: every int-returning function returns NST_OK (0) or a negative NST_E*
 * code; nst_last_error() returns the calling thread's last message.
 */
#ifndef NST_HIP_H
#define NST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
#define NST_OK 0
#define NST_E_INVALID (-1)   /* bad argument / unknown enum */
#define NST_E_PARAM (-2)     /* missing or mis-shaped checkpoint tensor */
#define NST_E_SHAPE (-3)     /* unsupported input/output geometry */
#define NST_E_HIP (-4)       /* HIP runtime error */
#define NST_E_WORKSPACE (-5) /* workspace too small */
#define NST_E_RANGE (-6)     /* nst_set_range_check: a value left the compute dtype's range (non-finite result) */

/* ---- architectures (pipeline.py:72-79 _detect_transformer_type, :598-603 reconet) ---- */
#define NST_ARCH_JOHNSON 0 /* transformer_net.py:4-41 */
#define NST_ARCH_NST 1     /* transformer_net_nst.py:62-127 */
#define NST_ARCH_RECONET 2 /* model.py:107-116 (frn=False, as pipeline.py:602 builds it) */
#define NST_ARCH_RECONET_FRN 3 /* model.py:107-116 with frn=True: FRN + TLU (frn.py:7-78) */
/* Torch7 fast-style nets (the *.t7 files pipeline.py:445-478, 583-596 runs through OpenCV DNN): ReflectionPad(40),
 * zero-padded 9x9 / stride-2 convs, five residual blocks of two VALID 3x3 convs joined with the block input shaved
 * by 2 px, two SpatialFullConvolution(3, s2, p1, adj1), 9x9 conv, Tanh, MulConstant.  Parameters by the NST_ARCH_NST
 * names (down1.conv / down1.norm ... res5.conv2 / res5.norm2, up1, up2, final: the host matcher
 * neuralstyletransferv1_amd/torch7.py emits them), plus "mul_constant" [1] and per norm layer "<norm>.eps" [1].
 *   _IN: nn.InstanceNormalization (biased variance over the layer's own, shrinking map)
 *   _BN: nn.SpatialBatchNormalization in eval mode: also "<norm>.running_mean" and "<norm>.running_var" [c]
 * Output side for input H: 4*(h3 - 20), h1 = H + 80, h2 = (h1-1)/2 + 1, h3 = (h2-1)/2 + 1 (= H when H % 4 == 0);
 * min(H, W) <= 40 is NST_E_SHAPE (the reflection needs pad < side).  Runs NST_DT_F32 / BF16 / F16 / F32S
 * (NST_DT_F16M: NST_E_INVALID).  Frames go through NST_PRESET_TORCH7 only. */
#define NST_ARCH_TORCH7_IN 4
#define NST_ARCH_TORCH7_BN 5

/* ---- compute dtypes ---- */
#define NST_DT_F32 0  /* fp32 "parity" mode: exact-f32 MFMA (v_mfma_f32_16x16x4_f32) */
#define NST_DT_BF16 1 /* bf16 "throughput" mode: bf16 MFMA, fp32 accumulate/statistics */
#define NST_DT_F16 2  /* fp16 mode: fp16 weights/activations, fp16 MFMA at the bf16 rate, fp32 accumulate/statistics;
                         3 more mantissa bits than bf16 (1080p: ~99.95 % of pixels within +-1 LSB of the reference).
                         Stored conv outputs must stay inside the fp16 range (|v| <= 65504) */
#define NST_DT_F32S 3 /* split-fp16 mode: fp32 activations in HBM; each conv operand is split into an fp16 pair
                         v = hi + lo in LDS (weights at pack time), and two v_mfma_f32_16x16x32_f16 per K step give
                         Wh*(xh + xl) + Wl*xh: ~22 significant bits per product (the fp32 parity bar) at a quarter of
                         the exact-f32 MFMA cycles.  Conv inputs must stay inside the fp16 range (|v| <= 65504) */
#define NST_DT_F16M 4 /* split-precision head + fp16 trunk (Johnson / NST nets): the first layer takes the raw bytes
                         (exact) against fp16 hi/lo weight pairs, the two down-convs run split-fp16 operands and
                         weights (Wh*xh + Wh*xl + Wl*xh), the first two residual blocks split-fp16 operands against
                         fp16 weights (Wh*xh + Wh*xl), all with fp32 activations, and the rest of the net runs the
                         fp16 mode's kernels.  The layers whose rounding reaches the frame
                         most (tests/precision_study.py) keep ~22-bit products: 1080p frames within +-1 LSB of the
                         fp32 reference at about 3/4 of the fp16 mode's rate.  ReCoNet: NST_E_INVALID */

/* ---- I/O formats for nst_forward ---- */
#define NST_IO_F32_NCHW 0 /* raw model tensor [n,3,h,w] fp32 (TransformerNet.forward(X) surface) */
#define NST_IO_U8_NHWC 1  /* frames [n,h,w,3] uint8 RGB; io_preset encode/decode + clamp + ToPILImage truncation fused */

/* ---- io presets (pipeline.py:1445-1486; auto table :2518-2523) ---- */
#define NST_PRESET_NONE 0 /* only valid with NST_IO_F32_NCHW on both sides */
#define NST_PRESET_TANH 1
#define NST_PRESET_IMAGENET_01 2
#define NST_PRESET_IMAGENET_255 3
#define NST_PRESET_CAFFE_BGR 4
#define NST_PRESET_RAW_255 5
#define NST_PRESET_RAW_01 6
/* The Torch7 nets' own pre / post arithmetic (pipeline.py:445-478; the NST_ARCH_TORCH7_* handles only, and the only
 * preset they take besides NST_PRESET_NONE).  Input: the caffe_bgr encode, BGR255 - (103.939, 116.779, 123.68).
 * Output: frame = trunc(clip(tanh(y) * mul_constant + mean, 0, 255)), BGR -> RGB; NST_IO_U8_NHWC gives the frame,
 * NST_IO_F32_NCHW gives frame / 255 in RGB planes: what to_tensor(pil_out).clamp(0, 1) hands on at :1443, so it feeds
 * nst_decode_resize_u8 / nst_blend_models_u8 / the region compositor as an NST_PRESET_RAW_01 source.  With
 * NST_PRESET_NONE (NST_IO_F32_NCHW both sides) x is the mean-subtracted BGR blob and y = tanh(.) * mul_constant,
 * what net.forward() returns at :466. */
#define NST_PRESET_TORCH7 7

typedef struct nst_handle nst_handle;
typedef struct nst_lab nst_lab;

/* One checkpoint tensor, by its reference state_dict name (e.g. "res1.conv1.conv2d.weight"). */
typedef struct nst_param {
  const char* name;
  const float* data; /* host fp32, contiguous in the reference's PyTorch layout */
  int64_t numel;
} nst_param;

/* Last error message of the calling thread ("" if none). */
const char* nst_last_error(void);

/* Library version string. */
const char* nst_version(void);

/*
 * Pack a checkpoint for one device.  Replaces model construction + load:
 * `TransformerNet().to(device)` + `_load_checkpoint_compat` (pipeline.py:554-569, 597-619).
 * Every parameter of the architecture must be present (missing -> NST_E_PARAM);
 * unknown names are ignored (load_state_dict(strict=False) semantics).
 */
int nst_create(int arch, const nst_param* params, int n_params, int compute_dtype, int device,
               nst_handle** out);

/*
 * nst_create with kernel-selection flags (0 = the default, fastest mapping for every layer).  Each
 * NST_KSEL_NO_* bit removes one specialised bf16 kernel family so the layer falls back to the
 * generic implicit-GEMM mapping; the tests use this to check the specialised kernels against the
 * generic ones on the same model.  NST_KSEL_UNFUSED_RESIDUAL runs the residual add as its own
 * kernel instead of fusing it into the next conv's fill.  Unknown bits -> NST_E_INVALID.
 */
#define NST_KSEL_NO_WSTAT 0x1             /* residual-trunk weight-stationary conv (conv_wst16.hip) */
#define NST_KSEL_NO_WPHASE 0x2            /* x2 up-conv phase kernel (conv_wphase.hip) */
#define NST_KSEL_NO_WS2 0x4               /* stride-2 down-conv kernel (conv_ws2.hip) */
#define NST_KSEL_NO_WS9 0x8               /* 9x9 first-layer kernel (conv_ws9.hip) */
#define NST_KSEL_NO_KYROT 0x10            /* 9x9 output-conv row-streaming kernel (conv_out9.hip) */
#define NST_KSEL_NO_PREPAD 0x20           /* first layer over the pre-padded encoded frame (conv_prep.hip) */
#define NST_KSEL_NO_PERSISTENT 0x40       /* generic persistent LDS-weight-ring kernels */
#define NST_KSEL_UNFUSED_RESIDUAL 0x80    /* residual add as a separate kernel */
#define NST_KSEL_NO_FOLD 0x100            /* uint8 frames: stage the encoded value instead of the raw byte with the
                                             io_preset encode folded into the first layer's weights */
#define NST_KSEL_F16M_TWO_BLOCKS 0x200    /* NST_DT_F16M: residual blocks 1 AND 2 on the split-operand kernel (wider
                                            precision margin: live max 0.920 instead of 0.958 LSB; ~10 % slower) */
#define NST_KSEL_PAD_DECODER 0x400       /* ReCoNet, 16-bit modes: the decoder's 96-channel stream padded to 128
                                            channels, as the encoder's (default: unpadded) */
#define NST_KSEL_PAD_ENCODER 0x800       /* ReCoNet, 16-bit modes: the encoder's 96-channel map padded to 128 (default:
                                            unpadded) */
#define NST_KSEL_PAD_48 0x1000         /* ReCoNet, 16-bit modes: the decoder's 48-channel output padded to 64 (default:
                                            unpadded) */
#define NST_KSEL_ALL 0x1fff
int nst_create_ex(int arch, const nst_param* params, int n_params, int compute_dtype, int device,
                  unsigned flags, nst_handle** out);
void nst_destroy(nst_handle* h);

/* Output spatial size the architecture produces for an h x w input
 * (Johnson/ReCoNet: 4*ceil(ceil(h/2)/2); NST: centre-cropped back to h x w). */
int nst_output_hw(const nst_handle* h, int in_h, int in_w, int* out_h, int* out_w);

/* Whether nst_forward feeds the first layer the reference's encoded input without any extra rounding for this
 * input format and io_preset (*exact = 1): always in the fp32-activation modes; in the 16-bit modes only for uint8
 * frames whose preset encode folds into the first layer's weights (reflection-padded first layers: every preset;
 * zero-padded ones, the NST net: presets without an offset).  NST_DT_F16M's +-1 LSB bar needs it (the Python
 * engine runs the other combinations on an NST_DT_F32S twin).  Replaces no reference call: a property query. */
int nst_input_exact(const nst_handle* h, int x_fmt, int preset, int* exact);

/* Device workspace nst_forward needs for a batch of n frames of h x w (with the handle's stream split: one slice
 * per sub-batch). */
int nst_workspace_bytes(const nst_handle* h, int n, int in_h, int in_w, size_t* out);

/* Run each nst_forward batch as k sub-batches (1 <= k <= 4) on internal streams forked from and joined back to the
 * caller's stream (events only: the caller's stream order is kept, frames are independent, outputs identical).
 * Default: 2 for the ReCoNet nets in the 16-bit modes and for NST_DT_F32S (their generic kernels' launch gaps and
 * tails are filled by the other sub-batches), 1 otherwise.  Profiling and the range check run a batch whole.  Replaces no reference
 * call: scheduling only. */
int nst_set_stream_split(nst_handle* h, int k);

/* A test seam: launch the persistent conv kernels of nst_forward / nst_forward_capture on this handle with at most
 * max_workgroups workgroups instead of the device-sized grid (CUs x resident workgroups), so that frames far smaller
 * than the device walk the kernels' tile loops: each workgroup takes work items b, b + G, b + 2G, ... of its launch.
 * The kernels are the same and an output element's arithmetic does not depend on the workgroup that computed it, so
 * outputs are identical; only the schedule changes.  The 9x9 output conv (one work item per wave) sizes its row
 * segments for max_workgroups x waves slots instead.  The internal streams of nst_set_stream_split see the same cap.
 * 0 = off (the default); < 0 -> NST_E_INVALID.  Replaces no reference call. */
int nst_set_grid_cap(nst_handle* h, int max_workgroups);
/* The seam's arithmetic, a pure function: the grid of a launcher that would use nb workgroups, under cap (0 = off). */
int nst_capped_blocks(int nb, int cap);
/* What op's conv launcher did in the handle's last forward: the workgroups and work items of its last launch and how
 * many launches it made (a batch of more frames than the kernel holds InstanceNorm tables for runs in chunks);
 * nst_op_launch_grid gives launch 0 .. launches-1 one by one.  All 0 for an op that ran no persistent kernel (a
 * residual add, a one-tile-per-workgroup kernel) or before any forward.  With a stream split: the last sub-batch's. */
int nst_op_last_grid(const nst_handle* h, int op, int* blocks, int* n_work, int* launches);
int nst_op_launch_grid(const nst_handle* h, int op, int launch, int* blocks, int* n_work);

/*
 * Stylize a batch.  Replaces `model(x_in)` with its io_preset pre/post arithmetic
 * (pipeline.py:1445-1486: preset encode -> .to(device) -> model -> .cpu() -> decode -> clamp(0,1))
 * and, for NST_IO_U8_NHWC output, the ToPILImage truncation `pic.mul(255).byte()`
 * (pipeline.py:1943/2094).  x: [n,3,h,w] f32 or [n,h,w,3] u8; y: [n,3,oh,ow] f32 (raw
 * model output, no preset) or [n,oh,ow,3] u8 (decoded).  U8 output requires
 * nst_output_hw(h,w) == (h,w) (otherwise use F32 output + nst_resize_bilinear_u8).
 */
int nst_forward(nst_handle* h, const void* x, int x_fmt, int n, int in_h, int in_w, int preset,
                void* y, int y_fmt, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Per-layer inspection (parity tests): the handle runs its architecture as a program of ops, each a
 * conv (with the producer's InstanceNorm + ReLU, or the residual join, applied in its fill) or a
 * separate residual add.  nst_op_describe gives op i's wiring and geometry for an n x h x w batch;
 * nst_forward_capture is nst_forward that also copies, after each op i, the activation it wrote
 * (act[i]: [n][out_h][out_w][cout_stride] in the compute dtype, the raw conv output before its
 * InstanceNorm), the joined residual stream it wrote (res[i]: [n][in_h][in_w][cin_stride]) and its
 * layer's InstanceNorm {scale, shift} pairs (stats[i]: [n][cout_stride] float2) into caller-owned
 * device buffers; NULL arrays or NULL entries skip a copy.  The final op writes y and captures nothing.
 * Replaces inspecting intermediate tensors of the reference's module graph (transformer_net.py:29-41).
 */
#define NST_BUF_INPUT (-1)  /* nst_op_desc src: the input frames / tensor */
#define NST_BUF_OUTPUT (-2) /* nst_op_desc dst: y */
typedef struct nst_op_desc {
  int kind;         /* 0 conv, 1 residual add (out = IN_in_norm(src) + r) */
  int layer;        /* conv layer index (nst_layer_name); for a residual add the layer whose IN applies */
  int src, dst;     /* activation buffer ids (0..6) or NST_BUF_INPUT / NST_BUF_OUTPUT */
  int in_norm;      /* layer whose InstanceNorm the fill applies to src, -1 = none */
  int in_relu;      /* ReLU after that InstanceNorm */
  int res_buf;      /* residual stream r joined in (-1 none): operand = IN(src) + r' */
  int res_norm;     /* r' = ReLU(IN_res_norm(r)) if >= 0, else r */
  int res_out;      /* buffer that receives the joined stream (-1 none) */
  int relu_out;     /* ReLU after the join (ReCoNet ResLayer) */
  int in_h, in_w;   /* source extent */
  int conv_h, conv_w; /* conv output extent (before the NST centre crop) */
  int out_h, out_w; /* stored output extent */
  int cin_stride, cout_stride;
  int kernel_mode;  /* internal kernel family (0 generic, 1 phase, 2 x-shift, 3 out9, 4 wstat = the weight-stationary trunk kernel, 5 wphase, 6 ws2, 7 ws9) */
  int elem_bytes;   /* bytes per element of what the op writes (act[i]): 2 (bf16 / fp16) or 4 (fp32) */
  int in_elem_bytes;  /* bytes per element of src (NST_BUF_INPUT: the staged first-layer operand, 2 or 4) */
  int res_elem_bytes; /* bytes per element of the joined residual stream (res_buf / res_out), 0 if none */
  int kernel_dtype;   /* the op's arithmetic: an NST_DT_* value, or 16 / 17 (fp16 operand x fp16 hi/lo weight
                         pairs, fp32 / fp16 output), 18 / 19 (split fp16 operand and weights, fp32 / fp16 output),
                         20 (split fp16 operand x fp16 weights, fp32 output) */
} nst_op_desc;
int nst_num_ops(const nst_handle* h);
/* Optional range check (the 16-bit and split modes hold operands inside the fp16 range, |v| <= 65504):
 * enabled, every nst_forward zeroes a device flag, checks each layer's InstanceNorm table (an overflowing operand
 * turns into inf, then a non-finite statistic) and an fp32 output for non-finite values, waits for the stream and
 * returns NST_E_RANGE if any was found.  Off by default (no extra launches, no synchronisation). */
int nst_set_range_check(nst_handle* h, int enable);
int nst_op_describe(const nst_handle* h, int n, int in_h, int in_w, int op, nst_op_desc* out);
int nst_forward_capture(nst_handle* h, const void* x, int x_fmt, int n, int in_h, int in_w, int preset,
                        void* y, int y_fmt, void* workspace, size_t workspace_bytes, void* const* act,
                        void* const* res, void* const* stats, void* stream);

/*
 * Decode a raw model output (f32 NCHW [n,3,h,w]) with `preset` + clamp(0,1), resize
 * bilinearly (align_corners=False) to out_h x out_w, truncate to u8 NHWC.
 * Replaces pipeline.py:1512-1516 (F.interpolate to content size) + :1943 ToPILImage.
 */
int nst_decode_resize_u8(const float* y, int n, int h, int w, int preset, uint8_t* out, int out_h,
                         int out_w, void* stream);

/*
 * Multi-model RGB blend (slots A..H, pipeline.py:1872-1879 with parse_blend_weights :502-511):
 * out01 = sum_i w_i * clamp(decode_i(y_i)), each y_i a raw model output f32 NCHW [n,3,h,w] with its
 * own io preset, fitted to out_h x out_w (bilinear, align_corners=False); clamp(0,1); truncate to
 * u8 NHWC.  ys: host array of m (<= 8) device pointers.  Weights are the fp32 values of the slots'
 * Python floats (the caller validates they sum to 1 +- 1e-6, as the reference does).
 */
int nst_blend_models_u8(const float* const* ys, const int* presets, const float* weights, int m, int n,
                        int h, int w, uint8_t* out, int out_h, int out_w, void* stream);

/* ---- LAB temporal smoothing (pipeline.py:1942-1978) ---- */

/* Upload the two 2^24-entry LittleCMS (Pillow) LUTs: rgb2lab[(r<<16)|(g<<8)|b] = {L,a,b}
 * bytes and lab2rgb[(L<<16)|(a<<8)|b] = {r,g,b} bytes (3*2^24 bytes each, host). */
int nst_lab_create(const uint8_t* rgb2lab, const uint8_t* lab2rgb, int device, nst_lab** out);
void nst_lab_destroy(nst_lab* lab);

/*
 * One frame (or a batch processed in frame order) of the LAB EMA:
 * L' = alpha*L + (1-alpha)*prev_L (fp32), prev_L = L', L byte = trunc(clip(L',0,255));
 * optional same EMA on a/b bytes with chroma_alpha.  `state` is a caller-owned device
 * buffer of 3*h*w floats (prev_L, prev_a, prev_b); `first` != 0 seeds it from the frame
 * (pipeline.py:1951-1952 `prev_L = L.copy()`).  rgb in/out: [n,h,w,3] u8 (may alias).
 * alpha/chroma_alpha are the fp32 values of the Python float coefficients.
 */
int nst_lab_ema_u8(const nst_lab* lab, const uint8_t* rgb_in, uint8_t* rgb_out, int n, int h, int w,
                   int smooth_lightness, float alpha, float one_minus_alpha, int smooth_chroma,
                   float chroma_alpha, float one_minus_chroma_alpha, float* state, int first,
                   void* stream);

/*
 * nst_lab_ema_u8 split in three stages for the sharded video pipeline (pipeline.py:1942-1978 with the
 * frames of one sequence stylized on several GPUs): the EMA's only cross-frame dependency is the fp32
 * state of the planes it smooths, so each frame's owner extracts those planes, one rank runs the ordered
 * EMA over the planes alone, and the owner rebuilds RGB from its own frame with the smoothed planes put
 * back.  The three calls give bytes identical to nst_lab_ema_u8 on the same frames in the same order.
 * planes: uint8 [n][np][h*w], np = smooth_lightness + 2*smooth_chroma, planes in the order L, a, b.
 *   nst_lab_planes_u8: rgb [n,h,w,3] -> planes (rgb2lab bytes of the smoothed channels);
 *   nst_lab_ema_planes: planes_in -> planes_out in frame order (may alias), state / first as nst_lab_ema_u8;
 *   nst_lab_merge_u8: rgb + smoothed planes -> rgb_out = lab2rgb(rgb2lab(rgb) with those planes replaced).
 */
int nst_lab_planes_u8(const nst_lab* lab, const uint8_t* rgb_in, int n, int h, int w, int smooth_lightness,
                      int smooth_chroma, uint8_t* planes, void* stream);
int nst_lab_ema_planes(const uint8_t* planes_in, uint8_t* planes_out, int n, int h, int w, int smooth_lightness,
                       float alpha, float one_minus_alpha, int smooth_chroma, float chroma_alpha,
                       float one_minus_chroma_alpha, float* state, int first, void* stream);
int nst_lab_merge_u8(const nst_lab* lab, const uint8_t* rgb_in, const uint8_t* planes, int n, int h, int w,
                     int smooth_lightness, int smooth_chroma, uint8_t* rgb_out, void* stream);

/*
 * Multi-model LAB blend (pipeline.py:1841-1870, --blend_models_lab): L from model A; per pixel
 *   a = trunc(clip(wL * a_A + wab * (sum_i w_i * a_i), 0, 255))  (float32, models B.. in order; same for b)
 * on Pillow's raw LAB bytes (signed a/b stored as uint8), then LAB -> RGB through the LittleCMS
 * tables.  frames: host array of m device pointers to [n,h,w,3] uint8 outputs (A first, each the
 * decoded + clamped + truncated model output, pipeline.py's to_pil(out.clamp(0,1))); the first
 * min(m-1, n_rest) of weights_rest pair with frames[1..] (zip semantics).
 */
int nst_blend_models_lab_u8(const nst_lab* lab, const uint8_t* const* frames, int m, const float* weights_rest,
                            int n_rest, float w_l, float w_ab, int n, int h, int w, uint8_t* out, void* stream);

/*
 * Mask feathering (pipeline.py:349-351 cv2.GaussianBlur(m, (0,0), sigmaX=sigmaY=sigma) then /255,
 * :353): masks [n,h,w] uint8 (after the NEAREST fit and optional invert) -> alpha [n,h,w] f32 in
 * [0,1].  ksize = round(6*sigma+1)|1, separable Gaussian, BORDER_REFLECT_101, uint8 rounding.
 * scratch: n*h*w floats.  sigma = feather_px * 0.5 (> 0; radius <= 1023).
 */
int nst_mask_feather(const uint8_t* mask, int n, int h, int w, float sigma, float* scratch, float* alpha,
                     void* stream);

/*
 * Uniform / masked blend with the original frame (pipeline.py:1984-2092):
 *   mask (optional, [n,h,w] f32 alpha in [0,1]): keep: C = a*S + (1-a)*O; replace: (1-a)*S + a*O; clip
 *   then if 0 <= blend < 1: out = clamp(blend*C + (1-blend)*O, 0, 1); truncate to u8.
 * S and O are u8 NHWC frames read as x/255 (to_tensor).  composite_mode: 0 keep, 1 replace.
 */
int nst_blend_u8(const uint8_t* styled, const uint8_t* orig, const float* mask, int composite_mode,
                 float blend, float one_minus_blend, uint8_t* out, int n, int h, int w,
                 void* stream);
/* nst_blend_u8 with an 8-bit mask [n,h,w] (alpha = m / 255 in fp32, pipeline.py:353): the DeepLab masks of
 * nst_seg_mask / nst_resize_u8 composited straight from HBM (configs[4]) */
int nst_blend_mask8_u8(const uint8_t* styled, const uint8_t* orig, const uint8_t* mask, int composite_mode, float blend,
                       float one_minus_blend, uint8_t* out, int n, int h, int w, void* stream);

/*
 * Live per-layer kernel timing (bench.py roofline): between nst_profile_begin and
 * nst_profile_end every conv launch of nst_forward on this handle is bracketed by a pair of
 * HIP events recorded on the forward's stream.  Call nst_profile_end after synchronising
 * that stream; it returns, per layer index (0..n_layers-1, program order), the summed
 * kernel milliseconds and the launch count, and releases the events.
 */
int nst_profile_begin(nst_handle* h);
int nst_profile_end(nst_handle* h, int n_layers, float* total_ms, int* launches);
/* Number of conv layers of the handle's architecture and a layer's state_dict prefix. */
int nst_num_layers(const nst_handle* h);
const char* nst_layer_name(const nst_handle* h, int layer);

/*
 * Gram matrix G[b] = F[b] F[b]^T / (c*hw) (utils.py:80-83 gram_matrix), F f32 or bf16, G fp32 [n,c,c].
 * layout NST_GRAM_CHW: F [n][c][hw] (the reference's NCHW feature map); NST_GRAM_HWC: F [n][hw][c]
 * (NHWC activations).  MFMA tiles over K slices of hw, slices summed in fixed order: bit-identical
 * across runs.  workspace: nst_gram_workspace_bytes (0 for a single slice).
 */
#define NST_GRAM_CHW 0
#define NST_GRAM_HWC 1
int nst_gram_workspace_bytes(int n, int c, int hw, size_t* out);
int nst_gram(const void* F, int dtype, int layout, int n, int c, int hw, float* G, void* workspace,
             size_t workspace_bytes, void* stream);

/* ---- Gatys optimisation loop (BASELINE.json configs[2]) ----
 * The reference provides only gram_matrix (utils.py:80-83) and preprocess_for_vgg (utils.py:93-96);
 * it has no VGG network, loss or optimiser.  These entry points build the loop the
 * configuration names around them: VGG-19 features (torchvision layout, state_dict keys
 * "features.N.weight"/"features.N.bias", N in {0,2,5,7,10,12,14,16,19,21,23,25,28}), style =
 * MSE of Grams of relu1_1..relu5_1, content = MSE of relu4_2, gradient with respect to the image,
 * Adam on the image.  Images: [1,3,h,w] fp32 in [0,1], h and w multiples of 16; bf16 activations
 * with fp32 accumulation. */
typedef struct nst_vgg nst_vgg;
int nst_vgg_create(const nst_param* params, int n_params, int device, nst_vgg** out);
/* flags: NST_VGG_GENERIC_ONLY runs every conv on the generic implicit-GEMM kernel (conv_vgg.hip) instead of
 * conv2_1 onward on the K-streaming GEMM conv (conv_gemm.hip) — the same arithmetic in another order */
#define NST_VGG_GENERIC_ONLY 0x1
int nst_vgg_create_ex(const nst_param* params, int n_params, int device, unsigned flags, nst_vgg** out);
void nst_vgg_destroy(nst_vgg* v);
/* caller-owned device buffers: workspace (activations, gradients, Grams) and state (targets) */
int nst_gatys_buffer_bytes(const nst_vgg* v, int h, int w, size_t* workspace, size_t* state);
/* forward only: the rectified feature maps relu1_1, relu2_1, relu3_1, relu4_1, relu5_1, relu4_2 (bf16
 * NHWC [h_l][w_l][c_l]) into feats[0..5] (NULL entries skipped) */
int nst_vgg_features(nst_vgg* v, const float* image, int h, int w, void* const* feats, void* workspace,
                     size_t workspace_bytes, void* stream);
/* targets into state: style Grams of `style` (same size as content) and relu4_2 of `content` */
int nst_gatys_targets(nst_vgg* v, const float* content, const float* style, int h, int w, void* state,
                      void* workspace, size_t workspace_bytes, void* stream);
/* losses (device float[3]: total, content, style) of `image` and grad = dL/d(normalised image),
 * fp32 [1,3,h,w]; L = content_weight * mean((F - P)^2) + style_weight * sum_l w_l mean((G_l - A_l)^2),
 * style_layer_weights: host float[5] (NULL = all 1) */
int nst_gatys_grad(nst_vgg* v, const float* image, int h, int w, const float* style_layer_weights,
                   float content_weight, float style_weight, const void* state, float* grad, float* losses,
                   void* workspace, size_t workspace_bytes, void* stream);
/* nst_gatys_grad that also copies dL/dz of each of the 13 convs (z = its pre-activation; bf16 NHWC
 * [h_i][w_i][c_i]) into dz[i] (NULL entries skipped): per-layer checks of the backward pass */
int nst_gatys_grad_capture(nst_vgg* v, const float* image, int h, int w, const float* style_layer_weights,
                           float content_weight, float style_weight, const void* state, float* grad,
                           float* losses, void* workspace, size_t workspace_bytes, void* const* dz,
                           void* stream);
/* torch.optim.Adam step on an image [c=3][hw] (step >= 1 counts updates; bias corrections from it);
 * grad_is_normalised: the gradient is with respect to (x - mean) / std (nst_gatys_grad's), so it is
 * divided by std per channel; clamp01 clamps the image to [0, 1] after the update */
int nst_adam_step(float* x, const float* grad, float* m, float* v, int c, int hw, float lr, float beta1,
                  float beta2, float eps, int step, int clamp01, int grad_is_normalised, void* stream);

/* ---- DeepLab v3+ mask program (BASELINE.json configs[4]) ----
 * The network of modeling/deeplab.py:9-33 as sky_swap.py:143-177 load_deeplab builds it: backbone
 * 'resnet' (ResNet-101, modeling/backbone/resnet.py:45-124), output stride 16, BatchNorm2d in eval mode,
 * ASPP (modeling/aspp.py:34-78), decoder (modeling/decoder.py:7-43).  Parameters by their state_dict
 * names without the "module." prefix (sky_swap.py:150 strips it), e.g. "backbone.layer3.22.conv2.weight",
 * "aspp.global_avg_pool.1.weight", "decoder.last_conv.8.bias"; running_mean / running_var are used,
 * num_batches_tracked is ignored.  NHWC activations in the compute dtype, fp32 accumulation; compute_dtype
 * NST_DT_F32S keeps fp32 activations and splits every conv's operands into fp16 pairs (the split-fp16 GEMM).
 *
 * nst_seg_create_ex picks the backbone.  NST_SEG_RESNET101: the network above (what nst_seg_create builds).
 * NST_SEG_DRN_D54: backbone 'drn' = DRN-D-54 (modeling/backbone/drn.py:102-234, :386-387), for which deeplab.py:13-14
 * forces output stride 8: a 7x7 3->16, 3x3 16->16 and 3x3/2 16->32 head at full input resolution (direct
 * convolutions, fp32 accumulation, preprocess fused), bottleneck layers 3..6 (3, 4, 6, 3 blocks; strides 2, 2, 1, 1;
 * dilations 1, 1, 2, 4), two conv layers 2048->512->512, ASPP on 512 channels with dilations 1, 12, 24, 36, the same
 * decoder on layer3's 256 channels at 1/4.  Names e.g. "backbone.layer0.0.weight", "backbone.layer6.2.conv2.weight",
 * "backbone.layer7.1.running_var".  Every other nst_seg_* entry serves either handle. */
#define NST_SEG_RESNET101 0
#define NST_SEG_DRN_D54 1
typedef struct nst_seg nst_seg;
int nst_seg_create(const nst_param* params, int n_params, int num_classes, int compute_dtype, int device,
                   nst_seg** out);
int nst_seg_create_ex(const nst_param* params, int n_params, int num_classes, int compute_dtype, int device,
                      int backbone, nst_seg** out);
void nst_seg_destroy(nst_seg* s);
int nst_seg_num_classes(const nst_seg* s);
int nst_seg_workspace_bytes(const nst_seg* s, int n, int h, int w, size_t* out);
/*
 * DeepLab.forward (deeplab.py:27-33) on a batch.  x: NST_IO_F32_NCHW = the module input [n,3,h,w]
 * (already normalised), or NST_IO_U8_NHWC = frames [n,h,w,3] with sky_swap.py:179-183 preprocess_pil
 * fused.  logits (optional): f32 NCHW [n,nc,h,w] = the module output (bilinear, align_corners=True);
 * pred (optional): u8 [n,h,w] = logits.argmax(1) (sky_swap.py:189-193: the second interpolate to the
 * same size is the identity).
 */
int nst_seg_forward(nst_seg* s, const void* x, int x_fmt, int n, int h, int w, float* logits, uint8_t* pred,
                    void* workspace, size_t workspace_bytes, void* stream);
/*
 * infer_mask's post-processing (sky_swap.py:196-215) on class maps pred [n,h,w] -> mask u8 [n,h,w]:
 * 255 where pred is one of target_ids, MORPH_CLOSE with ones(close_ks, close_ks) (5 in the reference;
 * 0 skips), dilate ones(2e+1), erode ones(2c+1), GaussianBlur(sigma = feather_px / 2) (cv2 restated:
 * parity unpinned).  scratch: nst_seg_mask_scratch_bytes.
 */
int nst_seg_mask_scratch_bytes(int n, int h, int w, size_t* out);
int nst_seg_mask(const uint8_t* pred, int n, int h, int w, const int* target_ids, int n_ids, int close_ks,
                 int expand_px, int contract_px, int feather_px, uint8_t* mask, void* scratch, size_t scratch_bytes,
                 void* stream);

/* ---- image resamplers of the mask / inference_res paths ----
 * NST_RESIZE_PIL_LANCZOS: Pillow Image.resize((ow, oh), Image.LANCZOS) of RGB frames (sky_swap.py:294-301,
 *   pipeline.py:1089-1097 --inference_res): Resample.c's two integer passes, bit-exact.
 * NST_RESIZE_CV_LINEAR: cv2.resize(m, (ow, oh), interpolation=INTER_LINEAR) of u8 images with c channels
 *   (sky_swap.py:321-324 mask upscale): OpenCV's fixed-point taps restated (cv2 absent: parity unpinned).
 * A resampler is made once per (h, w) -> (oh, ow) geometry: its tap tables live on the device. */
#define NST_RESIZE_PIL_LANCZOS 0
#define NST_RESIZE_CV_LINEAR 1
typedef struct nst_resize nst_resize;
int nst_resize_create(int kind, int h, int w, int oh, int ow, int device, nst_resize** out);
void nst_resize_destroy(nst_resize* r);
int nst_resize_scratch_bytes(const nst_resize* r, int n, size_t* out);
int nst_resize_u8(const nst_resize* r, const uint8_t* in, int n, int c, uint8_t* out, void* scratch,
                  size_t scratch_bytes, void* stream);

/* ---- Region-blend compositor (region_blend.py; pipeline.py:1120-1407 --region_optimize and :1720-1839
 * --region_mode) ----
 * The reference's control logic (random.Random draws, blend specs, animations) stays on the host
 * (neuralstyletransferv1_amd/regions.py); these entry points render, feather, rotate and composite. */
#define NST_REGION_MAX 32     /* regions per composite */
#define NST_REGION_TERMS 9    /* models A..H + the original per region */
#define NST_REGION_MAX_SRC 16 /* sources per composite */
/* mask geometry kinds (generate_region_masks, region_blend.py:925-980) */
#define NST_RG_RECTS 0      /* grid_masks / fractal_quad_masks :109-135, 307-364: region k = rects[k] {y1,y2,x1,x2} */
#define NST_RG_DIAGONAL 1   /* diagonal_masks :138-171: ivals[0] = 1 for x+y, 0 for (W-1-x)+y; dvals[3] = its max */
#define NST_RG_VORONOI 2    /* voronoi_masks :174-236: points[k] = (x, y); divisor[k] = sqrt(w_k)+1e-6 or 0 */
#define NST_RG_RADIAL 3     /* radial_masks :367-401: ivals = cx, cy; dvals[0] = rotation; lo/hi = wedge bounds */
#define NST_RG_WAVES 4      /* wave_masks :404-447: ivals[0] = 0 horizontal, 1 vertical, 2 diagonal;
                               dvals = frequency, amplitude, phase */
#define NST_RG_SPIRAL 5     /* spiral_masks :450-485: ivals = cx, cy; dvals = tightness, rotation, max(H, W) */
#define NST_RG_CONCENTRIC 6 /* concentric_masks :488-516: ivals = cx, cy; dvals[3] = r.max() */
/*
 * Hard (unfeathered) region masks [count][h][w] f32 0/1.  n_gen regions were generated (masks k >= n_gen
 * repeat region n_gen-1; n_gen = 0 gives all ones, :977-978).  Band kinds use lo[k] <= t < hi[k].  All
 * double constants are rounded to fp32 as torch rounds a Python float against a float32 tensor.
 * scratch (NST_RG_WAVES only): h*w + 2052 floats.
 */
int nst_region_masks(int kind, int count, int n_gen, const int* ivals, const double* dvals, const double* lo,
                     const double* hi, const int* rects, const double* points, const double* divisor, int h, int w,
                     float* masks, float* scratch, void* stream);
/* feather_mask (:69-102) in place on k planes: F.pad(reflect, ks/2) + the separable Gaussian whose ks (odd,
 * <= 511) host fp32 taps are the reference's normalised torch taps.  scratch: k*h*w floats. */
int nst_region_feather(float* masks, int k, int h, int w, const float* taps, int ks, float* scratch, void* stream);
/* rotate_all_masks (:25-66): cv2.warpAffine(INTER_LINEAR, BORDER_REPLICATE) of each plane about (W/2, H/2)
 * (OpenCV's fixed-point warp restated: cv2 absent, parity unpinned), then each pixel divided by the sum of
 * the rotated planes clamped to 1e-6.  in != out. */
int nst_region_rotate(const float* in, int k, int h, int w, double angle_deg, float* out, void* stream);
/*
 * warp_all_masks_organic (:737-810, --region_morph) of k planes: each plane j warped by cv2.remap(INTER_LINEAR,
 * BORDER_REFLECT; OpenCV's fixed-point remap restated, cv2 absent: parity unpinned) through
 * x + flow_x * max_disp, y + flow_y * max_disp, flows per mode (0 blob, 1 tentacle, 2 wave, 3 pulse; :688-715;
 * frequency is the noise frequency the mode uses, i.e. 2x for tentacle); blob/tentacle fields are
 * _simplex_noise_2d (:604-652) with the numpy PCG64 draws * 1000 in offsets[((j*2 + field)*2 + octave)*2 + xy]
 * (field 0 seeded morph.seed + 100 j, field 1 that + 1000); then the coverage-gap dilations (5/11/21/41 where
 * the sum < 0.1) and the normalisation by the clamped sum.  in != out.
 */
int nst_region_morph_scratch_floats(int k, int h, int w, size_t* out);
int nst_region_morph(const float* in, int k, int h, int w, int mode, double frequency, double time_offset,
                     double max_disp, const double* offsets, float* out, float* scratch, size_t scratch_floats,
                     void* stream);
/* compute_mask_bbox (:1969-1994): bbox[4k..4k+3] = {x1, y1, x2, y2} (exclusive ends) of the values >
 * threshold in plane k, device int buffer; an empty plane leaves {INT_MAX, INT_MAX, -1, -1}. */
int nst_region_bbox(const float* masks, int k, int h, int w, float threshold, int* bbox, void* stream);
/* scratch floats nst_region_composite_u8 needs (crops mode only) */
int nst_region_scratch_floats(int n, int h, int w, int crops, int with_orig, size_t* out);
/*
 * Region composite of a batch of n frames, out u8 NHWC [n,h,w,3] (ToPILImage truncation) and/or out_f32
 * NCHW [n,3,h,w] in [0,1].  Sources s < n_src: f32 NCHW [n,3,src_hw[2s],src_hw[2s+1]] decoded with
 * src_preset[s] (NST_PRESET_NONE for already-decoded images) and bilinearly fitted; source -1 is the
 * original frame orig u8 NHWC [n,h,w,3] (to_tensor).  Region k blends n_terms[k] (<= 9) terms
 * term_src[9k+j] with weights term_w[9k+j] (region_blend = zeros; += w * src in order).
 *   boxes == NULL: composite_regions(_advanced) (:1049-1108, 1589-1679) over full-frame masks [n_regions][h][w],
 *                  sources fitted to (h, w).
 *   boxes != NULL: composite_from_crops (:2186-2294): region k covers the padded bbox boxes[4k..4k+3] =
 *                  {x1,y1,x2,y2}, its sources are fitted to that crop; then the < 0.1 coverage-gap fill
 *                  (original frame, or max-pool dilation 5/11/21 without one); scratch per
 *                  nst_region_scratch_floats.
 */
int nst_region_composite_u8(const float* const* src_y, const int* src_hw, const int* src_preset, int n_src,
                            const int* n_terms, const int* term_src, const float* term_w, int n_regions,
                            const int* boxes, const uint8_t* orig, const float* masks, int n, int h, int w,
                            float* scratch, size_t scratch_floats, uint8_t* out, float* out_f32, void* stream);
/* --region_optimize crop input (pipeline.py:1309-1332): to_tensor(frame)[:, y1:y2, x1:x2] resized bilinearly
 * (align_corners=False) to out_h x out_w when they differ -> f32 NCHW [n,3,out_h,out_w] in [0,1], the
 * nst_forward NST_IO_F32_NCHW input.  box = {x1, y1, x2, y2}. */
int nst_region_crop_input(const uint8_t* frames, int n, int h, int w, const int* box, int out_h, int out_w, float* out,
                          void* stream);
/* the advanced path's low-resolution outputs (pipeline.py:1786-1796): raw output y [n,3,h,w] decoded with
 * preset, fitted to fit_h x fit_w, then resized bilinearly to out_h x out_w -> decoded f32 NCHW */
int nst_region_resize(const float* y, int n, int h, int w, int preset, int fit_h, int fit_w, int out_h, int out_w,
                      float* out, void* stream);

/* ---- Temporal stage (pipeline.py:1884-1940 --flow_ema, :2072-2086 --motion_blend) ---- */
/* pil_rgb.convert("L") (pipeline.py:1100): Pillow's integer luma (r*19595 + g*38470 + b*7471 + 0x8000) >> 16 of
 * frames [n,h,w,3] -> gray [n,h,w] */
int nst_gray_u8(const uint8_t* rgb, int n, int h, int w, uint8_t* gray, void* stream);
/* cv2.calcOpticalFlowFarneback(prev, next, None, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, 0)
 * (pipeline.py:1896-1899 passes 0.5, 3, 15, 3, 5, 1.1): OpenCV's optflowgf.cpp restated (cv2 absent: parity
 * unpinned).  prev/next u8 [h,w] device, flow f32 [h,w,2] = (dx, dy); scratch per nst_flow_scratch_floats.  This is
 * nst_flow_farneback_ex (below) with n = 1 and flags = 0, the same code: a pyramid whose coarsest level needs 64 to
 * 511 pre-blur taps, which used to fail at launch, now runs; a deeper one -> NST_E_SHAPE. */
int nst_flow_scratch_floats(int h, int w, size_t* out);
int nst_flow_farneback(const uint8_t* prev, const uint8_t* next, int h, int w, double pyr_scale, int levels,
                       int winsize, int iterations, int poly_n, double poly_sigma, float* flow, float* scratch,
                       size_t scratch_floats, void* stream);
/* DIS optical flow, the reference's default --flow_method (pipeline.py:1904-1914:
 * cv2.DISOpticalFlow_create(cv2.DISOPTICAL_FLOW_PRESET_FAST).calc(prev, next, None)) for n frame pairs: OpenCV's
 * dis_flow.cpp + variational_refinement.cpp restated with PRESET_FAST's parameters (patch 8, stride 4, finest scale 2,
 * 16 gradient-descent iterations, 5 variational refinement iterations; cv2 absent: parity unpinned).  prev/next u8
 * [n,h,w] device, flow f32 [n,h,w,2] = (dx, dy); scratch per nst_flow_dis_scratch_bytes (NST_E_SHAPE for frames too
 * small for the pyramid: min(round(log2(max(h,w)/32)), floor(log2(min(h,w)/8))) < 2). */
int nst_flow_dis_scratch_bytes(int n, int h, int w, size_t* out);
int nst_flow_dis(const uint8_t* prev, const uint8_t* next, int n, int h, int w, float* flow, void* scratch,
                 size_t scratch_bytes, void* stream);
/* --flow_downscale ds (pipeline.py:1886-1892, 1920-1923): gray [h,w] -> [h//ds, w//ds] (floored, as the reference's
 * (W0 // ds, H0 // ds)) by cv2.resize INTER_AREA (restated: integer scales take resizeAreaFast, others the fractional
 * cells of ResizeArea_Invoker), and the small flow [hs,ws,2] back to [h,w,2] by INTER_LINEAR times mul = ds */
int nst_flow_downscale_gray(const uint8_t* gray, int h, int w, int ds, uint8_t* out, void* stream);
/* cv2.resize(img, (out_w, out_h), interpolation=INTER_AREA) of n u8 images [n,h,w,c] (c <= 4), downscaling only
 * (out <= in): the DIS pyramid (cv2.DISOpticalFlow prepareBuffers) and --flow_downscale */
int nst_resize_area_u8(const uint8_t* in, int n, int h, int w, int c, uint8_t* out, int out_h, int out_w, void* stream);
int nst_flow_upscale(const float* flow_small, int hs, int ws, int h, int w, float mul, float* flow, void* stream);
/* flow EMA (pipeline.py:1926-1931 with _warp_with_flow :425-439): out = clip(alpha*curr + (1-alpha)*warp(prev)),
 * warp = cv2.remap(prev, x + dx, y + dy, INTER_LINEAR, BORDER_REPLICATE) restated; curr/prev/out f32 planar
 * [3,h,w] in [0,1], out != prev */
int nst_flow_fuse(const float* curr, const float* prev, const float* flow, int h, int w, float alpha,
                  float one_minus_alpha, float* out, void* stream);
/* motion-adaptive blend alpha (pipeline.py:2073-2080): m = GaussianBlur(clip(|flow| / motion_norm, 0, 1), sigma),
 * alpha = max_alpha - span * m (span = max_alpha - min_alpha as the fp32 the reference multiplies by);
 * alpha/scratch f32 [h,w] */
int nst_motion_alpha(const float* flow, int h, int w, float motion_norm, double sigma, float max_alpha, float span,
                     float* alpha, float* scratch, void* stream);

/* ---- Optical-flow morph between stills (the reference's optical_flow_morph: scripts/optical_flow_slideshow.py:17-70,
 * scripts/morph_v2.py:365-468; morph.py).  cv2 absent: every restatement below is parity unpinned. ---- */
/* cv2.calcOpticalFlowFarneback(prev, next, None, ..., flags) for n independent pairs in the same launches: prev/next
 * u8 [n,h,w] device, flow f32 [n,h,w,2]; scratch per nst_flow_scratch_floats_ex(n, h, w).  flags = 0 (the box window
 * of nst_flow_farneback, which is this entry point at n = 1) or NST_FLOW_GAUSSIAN (cv2.OPTFLOW_FARNEBACK_GAUSSIAN,
 * FarnebackUpdateFlow_GaussianBlur restated): m = winsize/2 (<= 63), sigma = m*0.3, taps k[0] = 1,
 * k[i] = (float)exp(-i*i/(2*sigma*sigma)), normalised by s = 1 + 2*sum k[i] in double; the 5 fields of M summed in
 * fp32 down the columns then along the rows, v = M[y]*k[0], v += (M[y-i] + M[y+i])*k[i] for i = 1..m (replicated
 * border), and the 2x2 solve in fp32.  Any other flags value -> NST_E_INVALID.  The pyramid's pre-blur takes up to
 * 511 taps (round(5 sigma) | 1 at the coarsest surviving level; 1080p at 5 or 6 levels needs 77): a deeper one ->
 * NST_E_SHAPE. */
#define NST_FLOW_GAUSSIAN 256
int nst_flow_scratch_floats_ex(int n, int h, int w, size_t* out);
int nst_flow_farneback_ex(const uint8_t* prev, const uint8_t* next, int n, int h, int w, double pyr_scale, int levels,
                          int winsize, int iterations, int poly_n, double poly_sigma, int flags, float* flow,
                          float* scratch, size_t scratch_floats, void* stream);
/* cv2.cvtColor(img, COLOR_BGR2GRAY) on 8-bit images, here on RGB-ordered frames [n,h,w,3] -> gray [n,h,w]:
 * (R*9798 + G*19235 + B*3735 + 16384) >> 15.  (nst_gray_u8 is Pillow's luma, what the frame loop uses.) */
int nst_gray_cv_u8(const uint8_t* rgb, int n, int h, int w, uint8_t* gray, void* stream);
/* cv2.GaussianBlur(gray, (5, 5), 1.0) of n u8 images [n,h,w] (morph_v2.py:387-388): fp32 taps of
 * getGaussianKernel(5, 1.0), BORDER_REFLECT_101, rows then columns in fp32, rounded half-to-even to u8.  OpenCV >= 4
 * blurs u8 images in 8.8 fixed point, so cv2's result may differ from this by 1 grey level (unmeasured).  out != in. */
int nst_gauss_u8(const uint8_t* in, int n, int h, int w, uint8_t* out, void* stream);
/* morph_v2.py:405-432 on n flows [n,h,w,2] in place: each component GaussianBlur((15, 15), 3.0) (REFLECT_101,
 * fp32), then where sqrtf(dx*dx + dy*dy) < 2: dx = (float)(dx + sign*((x - w/2.0)/w)*4.0), dy likewise with y and
 * h (the sum in double, rounded once).  sign: n host values, +1 (forward flow) or -1 (backward); n <= 16.
 * scratch: f32 [n,h,w,2]. */
int nst_morph_flow_post(float* flow, int n, int h, int w, const float* sign, float* scratch, void* stream);
/* All k frames of one transition in one launch: out u8 [k,h,w,3]; img1/img2 u8 RGB [h,w,3]; flow_fwd/flow_bwd f32
 * [h,w,2]; t, one_minus_t, wa, wb: k host values each (1 <= k <= NST_MORPH_MAX_FRAMES).  Frame f:
 *   warped1 = cv2.remap(img1, x + t[f]*fwd.x, y + t[f]*fwd.y, INTER_LINEAR, BORDER_REFLECT)
 *   warped2 = cv2.remap(img2, x + one_minus_t[f]*bwd.x, y + one_minus_t[f]*bwd.y, INTER_LINEAR, BORDER_REFLECT)
 *   out[f]  = cv2.addWeighted(warped1, wa[f], warped2, wb[f], 0)
 * restated: the maps in fp32 (multiply, then add), clamped to [-2w, 3w] x [-2h, 3h] (NaN to the low end) so that no
 * flow value indexes outside the images; remap in cv2's fixed point (X = rint(mx*32), 5 fraction bits, integer
 * weights summing to 32768, (sum + 16384) >> 15; each of the four taps reflected on its own, r = p mod 2n,
 * r < n ? r : 2n-1-r); the blend rint_half_even(p1*wa + p2*wb) in fp32, saturated.  h, w <= 32768. */
#define NST_MORPH_MAX_FRAMES 128
int nst_morph_frames(const uint8_t* img1, const uint8_t* img2, const float* flow_fwd, const float* flow_bwd, int h,
                     int w, int k, const float* t, const float* one_minus_t, const float* wa, const float* wb,
                     uint8_t* out, void* stream);

/* ---- Camera stage of the morph slideshow (scripts/morph_v2.py:624-999, create_morph_video with --pan_zoom; camera.py):
 * what the reference does to every morph frame before the video writer.  cv2 absent: every restatement below is
 * parity unpinned; tests/camera_ref.py is the numpy yardstick and the kernels equal it byte for byte (integer fixed
 * point, fp32 without contraction, or double).  Every entry point is batched over n <= NST_CAMERA_MAX_FRAMES frames
 * [n,h,w,3] u8 RGB (device) with per-frame parameters in host arrays, checks its arguments before any launch
 * (NST_E_INVALID; frame sizes outside 1..32768 NST_E_SHAPE) and launches on `stream`; out != in. ---- */
#define NST_CAMERA_MAX_FRAMES 32
#define NST_CAMERA_MAX_SMOOTH 15
/* (a) zoom pulse: cv2.resize(frame, (nw[i], nh[i]), INTER_LINEAR) cropped back to w x h at ((nw-w)/2, (nh-h)/2);
 * nw >= w, nh >= h.  8-bit linear path: scale = w/nw in double, fx = (float)((dx+0.5)*scale - 0.5), sx = floor(fx),
 * fx -= sx, sx < 0 -> (0, 0), sx >= w-1 -> (w-1, 0); taps (short)rint((1-fx)*2048), (short)rint(fx*2048); rows
 * likewise without the reset, rows sy and sy+1 clipped to the frame; S = S[sx]*a0 + S[sx+1]*a1,
 * out = (((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2. */
int nst_camera_pulse_u8(const uint8_t* in, int n, int h, int w, const int* nw, const int* nh, uint8_t* out,
                        void* stream);
/* (b) cv2.getRectSubPix(frame, (pw, ph), (cx[i], cy[i])), u8 -> u8 [n,ph,pw,3]: c -= (p-1)*0.5f, ip = floor(c),
 * a = cx-ip.x, b = cy-ip.y in fp32; weights rint(v*65536) of (1-a)(1-b), a(1-b), (1-a)b, ab, 1-b, b; pixel =
 * (a11*s0[j] + a12*s0[j+1] + a21*s1[j] + a22*s1[j+1] + 32768) >> 16; a row whose lower tap is past h-1 uses
 * s1 = s0, a column whose right tap is past w-1 reads column w-1 alone, (b1*s0 + b2*s1 + 32768) >> 16.  Only
 * ip >= 0 and ip + patch <= size is built (all the camera produces); anything else NST_E_INVALID. */
int nst_camera_rect_subpix_u8(const uint8_t* in, int n, int h, int w, int pw, int ph, const float* cx, const float* cy,
                              uint8_t* out, void* stream);
/* (c) cv2.resize(crop, (tw, th), INTER_LANCZOS4) -> [n,th,tw,3]; frame i's crop is the top-left ch[i] x cw[i] region
 * of its h x w buffer.  Table driven: device arrays xofs int32 [n,tw] (floor(fx), never reset), xcoef int16 [n,tw,8]
 * (saturate_cast<short>(rint(c*2048)) of interpolateLanczos4(fx)), yofs [n,th], ycoef [n,th,8]; frame i reads slot i.
 * Taps at ofs-3 .. ofs+4, each index clamped to the crop in the kernel (no table content reads outside it); rows
 * summed in int32, columns in int64, out = sat_u8((v + (1<<21)) >> 22). */
int nst_camera_lanczos_u8(const uint8_t* in, int n, int h, int w, const int* cw, const int* ch, int tw, int th,
                          const int32_t* xofs, const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef,
                          uint8_t* out, void* stream);
/* (d) apply_hue_shift (morph_v2.py:324-345) where hue_on[i], a copy otherwise (the caller applies |shift| < 0.1):
 * cv2's 8-bit BGR2HSV (sdiv / hdiv tables in 12 bits), h = np.remainder(float32(h) + hue_half[i], 180) in fp32
 * truncated to u8 (hue_half = float32(shift / 2)), HSV2BGR's float path, sat_u8(rint(x*255.f)).  in == out allowed. */
int nst_camera_hue_u8(const uint8_t* in, int n, int h, int w, const int* hue_on, const float* hue_half, uint8_t* out,
                      void* stream);
/* (e) temporal_smooth_frames (morph_v2.py:282-321) with NumPy >= 2 promotion: window = frames first .. first+win_n-1
 * of a sequence of seq_len frames, out = smoothed frames out_first .. out_first+out_count-1.  Per byte: acc (fp32)
 * = (float)((double)acc + (double)pixel * weights[j]) over the taps idx = g + j - kernel_size/2 inside the sequence,
 * total = the double sum of their weights in tap order, out = (u8)((double)acc / total) truncated.  weights:
 * kernel_size host doubles (1 <= kernel_size <= NST_CAMERA_MAX_SMOOTH).  A valid tap outside the window ->
 * NST_E_INVALID.  seq_len <= kernel_size: the frames are copied unchanged (the call site's condition). */
int nst_camera_smooth_u8(const uint8_t* window, int win_n, int h, int w, int first, int seq_len, int out_first,
                         int out_count, int kernel_size, const double* weights, uint8_t* out, void* stream);
/* (f) the fused stage: frame i goes through pulse (pulse_w x pulse_h; (w, h) = none), then getRectSubPix of
 * (patch_w, patch_h) at (cx, cy), then, zoom != 0, Lanczos to tw x th with table slot `table` (< table_slots), or,
 * zoom == 0, nothing (patch = target); then the hue rotation where hue_on.  The u8 rounding between the stages is
 * kept: taps of an earlier stage are recomputed, not skipped.  Pan-phase frames are one gather pass over the input
 * frame and one store; zoom-phase patches go through `scratch` (nst_camera_scratch_bytes; smaller NST_E_WORKSPACE).
 * out u8 [n,th,tw,3]; tw <= w, th <= h (NST_E_SHAPE).  At most two launches. */
typedef struct nst_camera_frame {
  int pulse_w, pulse_h;
  int zoom;
  int patch_w, patch_h;
  float cx, cy;
  int hue_on;
  float hue_half;
  int table;
} nst_camera_frame;
int nst_camera_scratch_bytes(const nst_camera_frame* frames, int n, size_t* out);
int nst_camera_frames_u8(const uint8_t* in, int n, int h, int w, const nst_camera_frame* frames, int tw, int th,
                         const int32_t* xofs, const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef,
                         int table_slots, uint8_t* out, void* scratch, size_t scratch_bytes, void* stream);

/* ---- Style morph: the weight-ladder blend of scripts/style_morph.py (create_video :216-298, interpolate_ladder
 * :105-118, the filters :42-59; style_morph.py here) ----
 * n output frames [n,h,w,3] u8 RGB from a bank of u8 RGB images [n_bank,h,w,3] (device; image i at byte i*h*w*3, any
 * alignment) and a host table of n descriptors; any n >= 1, the call splits it into launches itself.  Per channel, in
 * fp32 without contraction, in this order:
 *   S  = (float)bank[orig] * orig_w
 *   per term:  sf = hi < 0 ? (float)bank[lo] : (float)bank[lo] * w_lo + (float)bank[hi] * w_hi;  S = S + sf * weight
 *   v  = n_sides == 2 ? S0 * fade[0] + S1 * fade[1] : S0
 *   u8 = (uint8)min(max(v, 0), 255)                       truncated, as np.clip(...).astype(np.uint8)
 * then the filter on the u8 pixel: NST_SM_FILTER_SAT 8-bit RGB2HSV (as nst_camera_hue_u8), s' = (uint8)clip((float)s *
 * fparam[0], 0, 255), HSV2RGB; NST_SM_FILTER_VIBRANCE boost = fparam[0] + fparam[1] * ((float)s / 255.f) (an IEEE
 * division), s' = (uint8)clip((float)s * boost, 0, 255); NST_SM_FILTER_WARM R * fparam[0], G * fparam[1], B * fparam[2],
 * each clipped to 0..255 and truncated.  The arithmetic is the reference's own numpy float32 code; only the two
 * cvtColor calls are restated (parity unpinned, as the camera stage).
 * NST_E_INVALID: n < 1, a null pointer, an index outside 0..n_bank-1 (hi < 0 is the one-rung form), n_terms outside
 * 0..NST_STYLE_MORPH_MAX_STYLES, n_sides outside 1..2, an unknown filter, out overlapping the bank; NST_E_SHAPE: h or
 * w outside 1..32768.  Everything is checked before the first launch. */
#define NST_STYLE_MORPH_MAX_STYLES 8
#define NST_SM_FILTER_NONE 0
#define NST_SM_FILTER_SAT 1
#define NST_SM_FILTER_VIBRANCE 2
#define NST_SM_FILTER_WARM 3
typedef struct nst_style_morph_term {
  int lo, hi;
  float w_lo, w_hi, weight;
} nst_style_morph_term;
typedef struct nst_style_morph_side {
  int orig;
  float orig_w;
  int n_terms;
  nst_style_morph_term term[NST_STYLE_MORPH_MAX_STYLES];
} nst_style_morph_side;
typedef struct nst_style_morph_frame {
  int n_sides;
  float fade[2];
  nst_style_morph_side side[2];
  int filter;
  float fparam[3];
} nst_style_morph_frame;
int nst_style_morph_frames(const uint8_t* bank, int n_bank, int h, int w, const nst_style_morph_frame* frames, int n,
                           uint8_t* out, void* stream);

/* ---- Multi-model video: the pulsed multi-style compositor of scripts/multi_model_video.py
 * (create_multi_model_video :239-353, get_styled_frame :60-107, adjust_saturation :113-122; multi_model_video.py
 * here) ----
 * n output frames [n,h,w,3] u8 RGB from a bank of u8 RGB images [n_bank,h,w,3] (device; image i at byte i*h*w*3, any
 * alignment) and a host table of n descriptors; any n >= 1, the call splits it into launches itself.  One pass per
 * frame, the running value in registers.  Per channel, in fp32 without contraction, each product and sum rounded
 * alone; trunc(x) = (uint8)min(max(x, 0), 255), numpy's np.clip(x, 0, 255).astype(np.uint8).  In the script's order:
 *   ST(s), a styled still (get_styled_frame), s = {orig, lo, hi, orig_w, style_w, w_lo, w_hi}:
 *     lo < 0:  bank[orig] unchanged (the script's `return orig.astype(np.uint8)`)
 *     else     sf = hi < 0 ? (float)bank[lo] : (float)bank[lo] * w_lo + (float)bank[hi] * w_hi
 *              ST = trunc((float)bank[orig] * orig_w + sf * style_w)
 *   base       B = base_kind == NST_MM_PLAIN ? bank[base.orig] : ST(base)
 *   overlays   F = (float)B;  for k < n_over (0..2: mosaic, then tenharmsel):  F = F * keep[k] + (float)ST(over[k]) *
 *              over_w[k]  (ST truncated to u8 before it enters the sum);  U = trunc(F)
 *   saturation (adjust_saturation) when sat_on: 8-bit RGB2HSV (as nst_camera_hue_u8), s' = trunc((float)s * sat),
 *              HSV2RGB: the arithmetic of NST_SM_FILTER_SAT
 *   fades      G = (float)U
 *              fin >= 0:  G = (float)bank[fin] * fin_w[0] + G * fin_w[1]                    (fade-in from the original)
 *              cross_kind != NST_MM_NONE:  N = cross_kind == NST_MM_PLAIN ? bank[next.orig] : ST(next);
 *                         G = G * cross_w[0] + (float)N * cross_w[1]     (no truncation between fade-in and cross-fade)
 *   out = trunc(G)
 * Every weight is a double the host rounds to fp32 once when it fills the struct.  The arithmetic is the reference's
 * own numpy float32 code; only the two cvtColor calls are restated (parity unpinned, as the camera stage).
 * NST_E_INVALID: n < 1, n_bank < 1, a null pointer, an index outside 0..n_bank-1 where it is read (lo < 0, hi < 0,
 * fin < 0 are the absent forms; a plain image reads orig alone), n_over outside 0..2, an unknown base or cross kind,
 * out overlapping the bank; NST_E_SHAPE: h or w outside 1..32768.  Everything is checked before the first launch. */
#define NST_MM_NONE 0
#define NST_MM_PLAIN 1
#define NST_MM_STYLED 2
typedef struct nst_multi_model_still {
  int orig, lo, hi;
  float orig_w, style_w, w_lo, w_hi;
} nst_multi_model_still;
typedef struct nst_multi_model_frame {
  int base_kind; /* NST_MM_PLAIN or NST_MM_STYLED */
  nst_multi_model_still base;
  int n_over;
  nst_multi_model_still over[2];
  float keep[2], over_w[2];
  int sat_on;
  float sat;
  int fin;
  float fin_w[2];
  int cross_kind; /* NST_MM_NONE, NST_MM_PLAIN or NST_MM_STYLED */
  nst_multi_model_still next;
  float cross_w[2];
} nst_multi_model_frame;
int nst_multi_model_frames(const uint8_t* bank, int n_bank, int h, int w, const nst_multi_model_frame* frames, int n,
                           uint8_t* out, void* stream);

/* ---- Soft-blob compositor: create_soft_multi_blob_masks and the frame loop of scripts/selfstyle_blob.py
 * (generate_blob_video :295-474; the same masks in scripts/morph_faces.py and scripts/gen_pytorch_only_videos.py;
 * selfstyle_blob.py here) ----
 * The masks are the reference's numpy code under the NumPy it pins (< 2.0): every array operation float32, every Python
 * scalar rounded to fp32 once before it meets the array (the host does that when it fills the structs).  For blob b of
 * n_blobs, octave o = 0..3, pixel (y, x), each operation rounded to fp32 alone, no contraction, sinf / expf the accurate
 * library functions, both divisions IEEE:
 *   r  = amp[o]      * sinf((((yn[y] * freq[o]) * pi32 + phase_y[b][o]) + t_y[o]) + blob_phase[b])
 *   c  = amp[o]      * sinf((((xn[x] * freq[o]) * pi32 + phase_x[b][o]) + t_x[o]) + blob_phase[b])
 *   d  = amp_half[o] * sinf(((((xn[x] + yn[y]) * freq[o]) * pi32 + phase_t[b][o]) + t_t) + blob_phase[b])
 *   noise_b = ((noise_b + r) + c) + d   over o = 0..3 in that order, from 0
 *   m = max_b noise_b;  e_b = expf((noise_b - m) / T);  s = e_0 + e_1 + ... in blob order;  w_b = e_b / (s + 1e-6f)
 * yn[h], xn[w]: fp32 device tables, np.linspace(0, 1, h or w, dtype=float32).  r and c are evaluated once per row and
 * column of the block a workgroup owns, d once per pixel, octave and blob.
 * nst_blob_frames: n output frames [n,h,w,3] u8 RGB from a bank of u8 RGB images [n_bank,h,w,3] (device; any alignment)
 * and a host table of n per-frame descriptors; any n >= 1, the call splits it into launches itself.  Per channel:
 *   I_b = cv2.addWeighted(bank[lo_b], w_lo_b, bank[hi_b], w_hi_b, 0)      u8, rounded half to even, as nst_morph_frames
 *   F = 0;  for b = 0..n_blobs-1:  F = F + (float)I_b * w_b;   out = (uint8)F   truncated
 * nst_blob_masks: the weights alone, fp32 [n,n_blobs,h,w] (device), from the same field and descriptors (the four
 * still fields of a blob are not read).
 * NST_E_INVALID: n < 1, n_bank < 1, a null pointer, n_blobs outside 1..NST_BLOB_MAX, T not finite or <= 0, lo or hi of
 * a blob b < n_blobs outside 0..n_bank-1, out overlapping the bank; NST_E_SHAPE: h or w outside 1..32768.  Everything is
 * checked before the first launch. */
#define NST_BLOB_MAX 8
typedef struct nst_blob_field { /* what a video keeps for all of its frames */
  int n_blobs;
  float T; /* max(0.1, feather * 5) */
  float freq[4], amp[4], amp_half[4];
  float phase_y[NST_BLOB_MAX][4], phase_x[NST_BLOB_MAX][4], phase_t[NST_BLOB_MAX][4];
  float blob_phase[NST_BLOB_MAX];
} nst_blob_field;
typedef struct nst_blob_still { /* a blob's image: the cross-fade of two neighbouring stills of its stream */
  int lo, hi;
  float w_lo, w_hi;
} nst_blob_still;
typedef struct nst_blob_frame {
  float t_y[4], t_x[4], t_t; /* time_offset * (1 + 0.3 o), * (1.2 + 0.2 o), * 1.5 */
  nst_blob_still blob[NST_BLOB_MAX];
} nst_blob_frame;
int nst_blob_frames(const uint8_t* bank, int n_bank, int h, int w, const float* yn, const float* xn,
                    const nst_blob_field* field, const nst_blob_frame* frames, int n, uint8_t* out, void* stream);
int nst_blob_masks(int h, int w, const float* yn, const float* xn, const nst_blob_field* field,
                   const nst_blob_frame* frames, int n, float* out, void* stream);

/* cv2.addWeighted(a, wa, b, wb, 0) on two u8 device buffers of n_bytes bytes (any alignment): per byte in fp32
 * saturate(rint_half_even((float)a * (float)wa + (float)b * (float)wb)), each weight rounded to fp32 once.
 * NST_E_INVALID: a null pointer, n_bytes < 1, out overlapping a or b. */
int nst_add_weighted_u8(const uint8_t* a, double wa, const uint8_t* b, double wb, size_t n_bytes, uint8_t* out,
                        void* stream);

/* ---- PNG encode on the owner rank (pipeline.py:2099-2119 `Image.fromarray(out).save(path)`, the reference's
 * default --image_ext png at :2170) ----
 * n u8 frames [n,h,w,c] (c = 1 grey, 3 RGB, 4 RGBA; device) -> n complete PNG files, file j at out + j*out_stride,
 * its byte count in sizes[j] (int64, device).  Every scanline carries the Up filter; each scanline is one deflate
 * block (dynamic Huffman codes built per frame from that frame's run-length tokens, or a stored block where that is
 * smaller), the zlib stream's Adler-32 and the chunks' CRC-32 computed on the device.  Lossless: decoders return
 * the frames' bytes exactly, as from Pillow's file.  out_stride >= nst_png_bound; workspace per
 * nst_png_workspace_bytes; out and out_stride 16-byte aligned; w*c + 1 <= 65535. */
int nst_png_bound(int h, int w, int c, size_t* out_stride);
int nst_png_workspace_bytes(int n, int h, int w, int c, size_t* out);
int nst_png_encode_u8(const uint8_t* frames, int n, int h, int w, int c, uint8_t* out, size_t out_stride,
                      int64_t* sizes, void* workspace, size_t workspace_bytes, void* stream);

/* ---- JPEG decode of the extracted frames (pipeline.py:401-408 writes them with ffmpeg -c:v mjpeg, :1086 opens each
 * with Pillow; --jpeg_reader gpu) ----
 * Split in two.  The host half (no HIP call, no global state, thread-safe) entropy-decodes one baseline stream into
 * a coefficient record; the device half turns n records of one geometry into u8 frames [n,h,w,3] that equal
 * Pillow's Image.open(f).convert("RGB") byte for byte (libjpeg-turbo defaults: islow IDCT, fancy upsampling).
 *
 * Fast path: SOF0 (baseline, 8-bit, Huffman), 8-bit quantisation tables, one scan holding every component; 1
 * component, or 3 with ids 1,2,3 (JFIF YCbCr), chroma 1x1 and luma 1x1 / 2x1 / 2x2; DRI / RSTn; APPn and COM
 * skipped, except that an Adobe APP14 marker is refused.  Every other stream -> NST_E_SHAPE; a stream that does not
 * decode completely and cleanly (bad code, coefficient index past 63, premature marker, truncation, no EOI after
 * the last MCU) -> NST_E_DATA.  Either way the caller hands the file to its usual decoder.
 *
 * Record of one frame (record_bytes from nst_jpeg_probe; a multiple of 16): uint16 qt[3][64], the dequantisation
 * table of each component in natural order, then int16 coef[blocks][64] in natural order, planar by component, each
 * plane's blocks (the MCU grid's padding included) in raster order.  sampling: NST_JPEG_444 also for 1 component. */
#define NST_E_DATA (-7) /* damaged input stream */
#define NST_JPEG_444 0
#define NST_JPEG_422 1 /* luma 2x1 (h2v1) */
#define NST_JPEG_420 2 /* luma 2x2 (h2v2) */
int nst_jpeg_probe(const uint8_t* data, size_t len, int* h, int* w, int* comps, int* sampling, size_t* record_bytes);
/* record: caller memory (2-byte aligned, e.g. page-locked) of exactly the probed record_bytes */
int nst_jpeg_entropy_decode(const uint8_t* data, size_t len, void* record, size_t record_bytes);
int nst_jpeg_workspace_bytes(int n, int h, int w, int comps, int sampling, size_t* out);
/* records: n records back to back on the device (16-byte aligned), all of (h, w, comps, sampling); out u8 [n,h,w,3]
 * (4-byte aligned; a single component gives R = G = B); n*h*w < 2^31.  Two launches on `stream`, nothing else. */
int nst_jpeg_reconstruct_u8(const void* records, size_t record_bytes, int n, int h, int w, int comps, int sampling,
                            uint8_t* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- JPEG encode of the styled frames (pipeline.py:2099-2113 `out_img.save(out_path, format="JPEG",
 * quality=int(jpeg_quality))`; --jpeg_writer gpu) ----
 * n u8 RGB frames [n,h,w,3] (device) -> n complete JPEG files, file j at out + j*out_stride, its byte count in
 * sizes[j] (int64, device).  Each file equals what Pillow (libjpeg-turbo defaults) writes for that frame and quality
 * byte for byte: JFIF 1.1 APP0 (units 0, density 1:1), two DQT, baseline SOF0 at 4:2:0, the four standard DHT, one
 * interleaved scan without restart markers, EOI.  The whole file is built on the device (colour, h2v2 downsample,
 * islow FDCT, quantise, Huffman coding, 0xFF stuffing); the host only writes bytes.
 *
 * quality 1..100; h, w 1..65535 and at most 2^21 8x8 blocks per frame (a frame's bit count stays below 2^32); out,
 * out_stride and workspace 16-byte aligned.  out_stride may be below nst_jpeg_enc_bound (the worst case of any
 * content): a frame whose file does not fit its slot gets sizes[j] = -1, nothing is written outside its slot, and the
 * other frames' files are complete.  Bytes of a slot past sizes[j] are undefined.  Workspace per
 * nst_jpeg_enc_workspace_bytes (a smaller one is NST_E_INVALID, like every other bad argument, before any GPU call).
 * Every launch goes on `stream`; no allocation, no copy, no host synchronisation. */
int nst_jpeg_enc_bound(int h, int w, size_t* out_stride);
int nst_jpeg_enc_workspace_bytes(int n, int h, int w, size_t* out);
int nst_jpeg_encode_u8(const uint8_t* frames, int n, int h, int w, int quality, uint8_t* out, size_t out_stride,
                       int64_t* sizes, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NST_HIP_H */

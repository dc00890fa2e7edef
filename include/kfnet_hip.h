/* libkfnet_hip.so -- C ABI of the MI355X-native (gfx950) KFNet prediction path.
 *
 * The reference (zlthinker/KFNet) has no native/FFI boundary: its hot path is a TF-1.x
 * graph built by the Python `cnn_wrapper.Network` DSL and executed by `sess.run`
 * (KFNet/eval.py:78-83).  Each entry point below replaces the TensorFlow op(s) that one
 * reference call site dispatches to; the Python host in kfnet_amd/ keeps the reference's
 * class/method surface and calls these through ctypes.
 *
 * Conventions
 *   - extern "C"; every function returns KFN_OK (0) or a negative KFN_ERR_*; the text
 *     of the last error on the calling thread is kfn_last_error().  No exceptions cross.
 *   - All tensors are device pointers to fp32, NHWC, unless the name says otherwise.
 *     The caller owns every buffer; the library never allocates or frees tensor memory
 *     behind the caller's back and keeps no per-call state (re-entrant; any number of
 *     host threads may call with distinct streams, on any device: launches go to the
 *     calling thread's current device, kernel attributes are set per device).
 *   - `stream` is a hipStream_t (NULL = the default stream).  All work is asynchronous
 *     on that stream and hipGraph-capturable: no entry point allocates, frees or synchronises
 *     (kfn_malloc / kfn_free / kfn_stream_sync / kfn_event_elapsed_ms / kfn_comm_init are the
 *     plumbing exceptions and say so).  Scratch memory, where a launch needs it, is the caller's
 *     (kfn_winograd_workspace_bytes, kfn_kalman_scan_scratch_bytes).
 *   - A "pixel stride" (ldx / ldy) is the distance in floats between consecutive
 *     pixels; it lets a layer read or write a channel slice of a wider buffer, which is
 *     how `Network.concat` (cnn_wrapper/network.py:316-318) is realised without copies.
 */
#ifndef KFNET_HIP_H_
#define KFNET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KFN_OK 0
#define KFN_ERR_ARG (-1)
#define KFN_ERR_HIP (-2)
#define KFN_ERR_UNSUPPORTED (-3)

/* 5 (round 4): kfn_conv_desc starts with `struct_size` (the struct had grown at its end -- weights_path -- without a
 * version bump); kfn_comm_rank asks RCCL; kfn_kalman_scan_ex no longer allocates.  A host checks
 * kfn_abi_version() == KFN_ABI_VERSION once after loading the library.
 * 6 (round 5): split-K Winograd entry points, kfn_winograd_lds_bytes.  7 (round 5): kfn_decode_png_rgb8.
 * 8 (round 6): KFN_WINO_FORM_S2_F42, kfn_apply_transform / kfn_pixel_map / kfn_bilinear_sampler.
 * 9 (round 6): kfn_conv_desc.x_layout / y_layout (KFN_LAYOUT_C16).  10 (round 6): kfn_kalman_arith_probe.
 * 11: camera poses -- kfn_pnp_desc, kfn_pnp_scratch_bytes, kfn_pnp_ransac, kfn_pnp_hypotheses.
 * 12: kfn_coord_records, kfn_flow_records; later kfn_crc32c (reading TensorFlow checkpoints), an added export that leaves
 * every ABI-12 host working, so the number stays.
 * 13: the constants the reference squares in Python cross the boundary as doubles -- kfn_kalman_desc.min_uncertainty,
 * kfn_coord_loss_desc.dist_threshold / min_uncertainty and the two thresholds of kfn_eval_metrics (layout and signature
 * change: an ABI-12 host must be rebuilt); later kfn_frame_channel_sums and kfn_augment_batch (augmenting a training
 * batch), added exports that leave every ABI-13 host working, so the number stays; likewise kfn_decode_png_gray16,
 * kfn_depth_labels and kfn_label_moments (training labels from depth maps and poses), and kfn_measurement_map,
 * kfn_filter_loss_grad, kfn_filter_backward_scratch_bytes and kfn_filter_backward (fine-tuning SCoordNet through the filter),
 * and kfn_cost_volume_backward, kfn_flow_head_backward, kfn_l2norm_backward and kfn_flow_loss_grad (training OFlowNet),
 * and kfn_filter_backward_joint (joint stage 3: both networks trained through the filter), and kfn_pnp_ransac_unc and
 * kfn_pose_filter (uncertainty-aware poses: weighted refinement, pose covariance, pose filter), and kfn_reproj_loss_grad
 * and kfn_augment_pixel_map (the reprojection loss of KFNet/KFNet.py:405-428 for stages 1 and 3), and kfn_pose_track,
 * kfn_pose_track_state_bytes and kfn_pose_track_scratch_bytes (the pose tracker: motion models, backward pass, carried state),
 * and kfn_pnp_guided_scratch_bytes, kfn_pnp_ransac_guided and kfn_pnp_hypotheses_guided (hypotheses drawn by confidence),
 * and kfn_render_scratch_bytes and kfn_render (labels, depth maps and frames rendered from a triangle mesh), and
 * kfn_fuse_scratch_bytes, kfn_fuse_integrate, kfn_fuse_extract_count and kfn_fuse_extract (depth maps fused into a truncated
 * signed distance volume, and the scene mesh extracted from it), and kfn_track_scratch_bytes, kfn_track_live_maps,
 * kfn_track_raycast, kfn_track_icp_sums, kfn_track_update and kfn_track_commit (the camera tracked against that volume), and kfn_reloc_encode,
 * kfn_reloc_search, kfn_reloc_seed and kfn_reloc_settle (a lost tracker relocalised from fern-coded keyframes), and
 * kfn_kalman_scan_plan (which of the scan's instantiations a grid launches; host only), and kfn_conv2d_grad_weights_plan
 * (tiles and runs of pixels of a weight-gradient launch; host only), and kfn_winograd_launch_plan (kfn_wino_plan: what a
 * Winograd entry point launches for a descriptor, the struct its launcher launches from; host only), and
 * kfn_kabsch_scratch_bytes, kfn_kabsch_ransac, kfn_kabsch_hypotheses and kfn_kabsch_select (poses from the records and a
 * depth frame: RANSAC-Kabsch). */
#define KFN_ABI_VERSION 13

const char* kfn_last_error(void);
int kfn_abi_version(void);
/* Device facts used by the host-side tile heuristics.  arch receives e.g. "gfx950". */
int kfn_device_info(int device, int* cu_count, int* lds_bytes_per_cu, char* arch, int arch_len);

/* ---- host side of the image stream ---------------------------------------------------------------------------------
 * tf.image.decode_png(channels=3) of the reference's queue runners (KFNet/train.py:195-239, the decode at :213-217):
 * n PNG files -> dst [n][H][W][3] uint8 RGB, decoded by `threads` native threads (<= 0: one per file, at most the
 * hardware's) straight into the caller's staging buffer (page-locked or not).  Host code only -- no device access, no GIL.
 * Non-interlaced files of bit depth <= 8, colour types gray / RGB / palette / gray+alpha / RGBA (alpha dropped, gray
 * replicated: what decode_png(channels=3) and PIL's convert('RGB') return).  status [n] (may be NULL) receives one of the
 * KFN_PNG_* codes per file: an interlaced or 16-bit file (or one without the PNG signature) is KFN_PNG_UNSUPPORTED -- its frame in dst is left untouched and
 * the call still succeeds (kfnet_amd.pipeline decodes those with PIL); a missing, corrupt or wrong-sized file is
 * KFN_PNG_ERROR and the call returns KFN_ERR_ARG with kfn_last_error() naming the first such file. */
#define KFN_PNG_OK 0
#define KFN_PNG_UNSUPPORTED 1
#define KFN_PNG_ERROR 2
int kfn_decode_png_rgb8(const char* const* paths, int n, int H, int W, unsigned char* dst, int* status, int threads);
/* The same call for depth maps (7-Scenes' frame-*.depth.png): n PNG files -> dst [n][H][W] uint16 in host order.  Decodes
 * non-interlaced colour type 0 at bit depth 16 (big-endian samples in the file), all five filter types, any IDAT split.
 * Any other colour type or bit depth, an interlaced file or one without the PNG signature is KFN_PNG_UNSUPPORTED: its
 * frame is untouched and the call succeeds (kfnet_amd.labels.load_depth decodes those with PIL).  A missing, truncated,
 * corrupt or wrong-sized file is KFN_PNG_ERROR, its frame is untouched, and the call returns KFN_ERR_ARG with
 * kfn_last_error() naming the first such file.  Host code only. */
int kfn_decode_png_gray16(const char* const* paths, int n, int H, int W, uint16_t* dst, int* status, int threads);

/* ---- host side of restoring a tf.train.Saver V2 checkpoint (ABI 12) -------------------------------------------------
 * CRC-32C (Castagnoli, reflected polynomial 0x82F63B78, ~0 pre- and post-inversion) of n bytes, extending *crc: *crc == 0
 * starts a checksum, and calls over consecutive pieces of a buffer give the value of one call over all of it.  The
 * checkpoint's table blocks and tensors carry it (masked; kfnet_amd/checkpoint.py).  Uses the SSE4.2 crc32 instruction
 * when the CPU has it, a slicing-by-8 table otherwise (same result).  Host code only -- no device access.  KFN_ERR_ARG on
 * a null crc, or null data with n > 0. */
int kfn_crc32c(const void* data, size_t n, uint32_t* crc);

/* ---- plumbing for hosts that do not bring their own allocator/streams (PyTorch does) -- */
int kfn_malloc(void** dptr, size_t bytes);
int kfn_free(void* dptr);
int kfn_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int kfn_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int kfn_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
int kfn_memset(void* dst, int value, size_t bytes, void* stream);
int kfn_stream_create(void** stream);
int kfn_stream_destroy(void* stream);
int kfn_stream_sync(void* stream);
int kfn_event_create(void** event);
int kfn_event_destroy(void* event);
int kfn_event_record(void* event, void* stream);
int kfn_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on stop */

/* ---- convolution: replaces tf.layers.conv2d / tf.layers.conv2d_transpose -------------
 * Network.conv   cnn_wrapper/network.py:116-135  (SCoordNet.py:21-32, OFlowNet.py:19-41,
 *                KFNet/KFNet.py:318-338 call tf.layers.conv2d directly)
 * Network.deconv cnn_wrapper/network.py:418-437  (OFlowNet.py:26,31,36)
 * tf.layers.dense (OFlowNet.py:50-55) is the 1x1 case on a [P,1,1,C] tensor.
 *
 * Implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32, fp32 accumulate):
 *   M = N*Ho*Wo output pixels, N = Cout, K = kh*kw*Cin (requires Cin % 16 == 0).
 * Weights are PRE-PACKED by the host into w_packed[cout_pad][kh*kw*Cin] (K contiguous;
 * row co holds w[kh][kw][ci][co] in (kh,kw,ci) order; for transposed convs the TF
 * [kh,kw,Cout,Cin] kernel is packed in the same (kh,kw,ci) order); cout_pad is Cout
 * rounded up to a multiple of 32 with zero rows.  Padding is TF 'SAME'.
 */
typedef struct kfn_conv_desc {
  int32_t struct_size;  /* = sizeof(kfn_conv_desc) AS THE CALLER COMPILED IT (use KFN_CONV_DESC_INIT).  The struct only
                         * ever grows at its end: the library copies struct_size bytes and reads every field beyond them
                         * as 0 (= AUTO / fp32), so a host built against an older header keeps working and the library
                         * never reads past the caller's object.  Smaller than the first-round struct (through `config`),
                         * not a multiple of 4, or larger than the library's own struct: KFN_ERR_ARG. */
  int32_t N, H, W, Cin; /* logical input shape */
  int32_t ldx;          /* input pixel stride (floats), >= Cin, multiple of 4 */
  int32_t Cout;         /* logical output channels */
  int32_t cout_pad;     /* rows of w_packed (multiple of 32) */
  int32_t ldy;          /* output pixel stride (floats), >= Cout */
  int32_t kh, kw;       /* kernel size (kh*kw <= 32) */
  int32_t stride;       /* 1 or 2 */
  int32_t transposed;   /* 0 = conv2d SAME, 1 = conv2d_transpose SAME (stride 2; 3x3 kernels only: any other kh x kw with
                         * transposed = 1 is KFN_ERR_ARG -- kh*kw <= 32 above is the promise of the forward convolution) */
  int32_t relu;         /* fuse tf.nn.relu */
  int32_t epilogue;     /* KFN_EPI_* applied after bias(+relu).  Forward convolutions only: a transposed call with an
                         * epilogue, and any value outside KFN_EPI_NONE .. KFN_EPI_EXP_1E2, is KFN_ERR_ARG (both used to
                         * return KFN_OK with the epilogue not applied; no caller in this repository passed either). */
  int32_t config;       /* 0 = auto tile choice, else KFN_CFG_* */
  int32_t operand_dtype; /* KFN_OPERAND_F32 (exact fp32 MFMA) or KFN_OPERAND_F16: operands rounded
                          * to fp16 while staged, fp32 accumulate on v_mfma_f32_32x32x16_f16
                          * (BASELINE config 5); then w_packed holds IEEE halfs and Cin % 32 == 0.
                          * Activations and outputs stay fp32 in memory unless x_dtype / y_dtype say
                          * otherwise. */
  int32_t wino_order;    /* Winograd kernels only: workgroup order, KFN_WINO_ORDER_* (0 = the kernel's default) */
  int32_t wino_form;     /* kfn_conv2d_winograd_fused / _f43 / _s2: KFN_WINO_FORM_* (0 = auto) */
  int32_t x_dtype;       /* KFN_ACT_F32 / KFN_ACT_F16: element type of the input activations in memory */
  int32_t y_dtype;       /* ... of the output activations.  KFN_ACT_F16 needs operand_dtype == KFN_OPERAND_F16
                          * (BASELINE config 5: fp16 activations end to end); ldx / ldy count ELEMENTS. */
  int32_t k_step;        /* 0 = auto; 16 / 32 = LDS k-step in 4-byte words (fp16 operands: 32 / 64 channels per
                          * stage).  32 exists for the fp16-activation kernels only. */
  int32_t weights_path;  /* fp16 activations in AND out only: KFN_WEIGHTS_AUTO / _VIA_REGISTERS (global -> registers ->
                          * ds_write) / _LDS_DMA (global -> LDS directly, `buffer_load ... lds`, three weight buffers) /
                          * KFN_OPERANDS_LDS_DMA (the activation tile too) */
  int32_t x_layout;      /* KFN_LAYOUT_NHWC (0) / KFN_LAYOUT_C16: memory layout of the input activations (ABI 9) */
  int32_t y_layout;      /* ... of the output.  Only kfn_conv2d_winograd_f43 (eight-wave form) and kfn_conv2d_winograd_s2
                          * (F(4,2) form) take KFN_LAYOUT_C16; every other entry point refuses a non-zero layout
                          * (KFN_ERR_UNSUPPORTED) instead of reading the buffer as NHWC. */
} kfn_conv_desc;
/* kfn_conv_desc d = KFN_CONV_DESC_INIT;  -- zero everything, set struct_size */
#define KFN_CONV_DESC_INIT {(int32_t)sizeof(kfn_conv_desc)}

#define KFN_WEIGHTS_AUTO 0
#define KFN_WEIGHTS_VIA_REGISTERS 1
#define KFN_WEIGHTS_LDS_DMA 2
#define KFN_OPERANDS_LDS_DMA 3    /* activations AND weights global -> LDS directly, three buffers each */

#define KFN_ACT_F32 0
#define KFN_ACT_F16 1

/* Activation layouts.  NHWC: element (n, h, w, c) at ((n*H + h)*W + w)*ld + c -- the layout of the reference's tensors and the
 * default everywhere.  C16 ("channel-blocked"): per image [C/16][H][W][16], element at n*H*W*C + (((c/16)*H + h)*W + w)*16
 * + c%16 -- needs C % 16 == 0 and a dense tensor (ld == C).  The image stride is the same, so batch windows of a tensor are
 * layout-agnostic.  The Winograd kernels read 16 input channels of a patch per step: in C16 a 6-pixel patch row is 384
 * contiguous bytes instead of six 64-byte pieces of six different lines (measured: the F(4x4,3x3) kernel -2 ... -3 %). */
#define KFN_LAYOUT_NHWC 0
#define KFN_LAYOUT_C16 1

/* Order in which the Winograd kernels' workgroups walk (tile block, channel group): with the tile blocks
 * fastest every resident workgroup of an XCD streams the same weight slice and the input crosses the
 * fabric once per channel group; with the channel groups fastest the input crosses once and every group's
 * weights are live at once.  Run time is the same either way (profiles/r03_wino_order_ab.log); the field
 * exists so that this A/B stays reproducible without hidden state. */
#define KFN_WINO_ORDER_AUTO 0
#define KFN_WINO_ORDER_M_FAST 1
#define KFN_WINO_ORDER_N_FAST 2
#define KFN_WINO_ORDER_GROUPS(n) (16 + (n)) /* kfn_conv2d_winograd_f43 / _s2: n channel groups (of 64 / 128) of a tile block adjacent */
#define KFN_WINO_FORM_AUTO 0
#define KFN_WINO_FORM_ONE_WAVE 1 /* force wino2_kernel (one wave per 32 output channels) where wino3_kernel / wino3_pair_kernel would run */
#define KFN_WINO_FORM_F43_FOUR_WAVE 2  /* kfn_conv2d_winograd_f43: wino4_kernel (four waves, 32x32x2 MFMA tiles) */
#define KFN_WINO_FORM_F43_EIGHT_WAVE 3 /* kfn_conv2d_winograd_f43: wino4b_kernel (eight waves, 16x16x4 MFMA tiles) */
#define KFN_WINO_FORM_S2_EIGHT_WAVE 4  /* kfn_conv2d_winograd_s2: wino_s2b_kernel (eight waves, 16x16x4 MFMA tiles; fp32 operands) */
#define KFN_WINO_FORM_S2_F42 5         /* kfn_conv2d_winograd_s2: wino_s2c_kernel, polyphase + F(4,2) on 4x4 output tiles (81 instead of 100
                                        * products per 16 outputs; fp32, H and W multiples of 8; weights: pack_winograd_s2_kernel_c) */

#define KFN_OPERAND_F32 0
#define KFN_OPERAND_F16 1
/* fp32-class accuracy on the fp16 MFMA: operands split into hi + lo halfs while staged,
 * hi*hi + hi*lo + lo*hi accumulated in fp32 (forward convs, Cin % 32 == 0).  w_packed =
 * [hi | lo] half matrices of 1024*w (each [cout_pad][K]); the kernel scales the sum by 2^-10. */
#define KFN_OPERAND_F16X3 2

#define KFN_EPI_NONE 0
#define KFN_EPI_L2NORM 1   /* tf.nn.l2_normalize(axis=-1), KFNet/KFNet.py:340; needs Cout == 32 */
#define KFN_EPI_EXP_CH3 2  /* SCoordNet.GetOutput: uncertainty = exp(ch 3), SCoordNet.py:39-44 */
#define KFN_EPI_EXP_1E2 3  /* OFlowNet.GetOutput: exp(.) * 1e-2, OFlowNet.py:56 */

#define KFN_CFG_AUTO 0
#define KFN_CFG_160x128 1  /* 4 waves, wave tile 160x32 */
#define KFN_CFG_128x128 2  /* 4 waves, wave tile 64x64 */
#define KFN_CFG_128x64 3   /* 4 waves, wave tile 64x32 */
#define KFN_CFG_128x32 4   /* 4 waves, wave tile 32x32 */
#define KFN_CFG_64x64 5    /* 4 waves, wave tile 32x32 */
#define KFN_CFG_256x32 6   /* 4 waves, wave tile 64x32 (Cout <= 32 layers) */
#define KFN_CFG_192x64 7   /* 4 waves, wave tile 96x32 (Cout == 64 layers) */
#define KFN_CFG_160x256 8  /* 8 waves, wave tile 160x32 (never chosen automatically) */
#define KFN_CFG_128x256 9  /* 4 waves, wave tile 64x128: the Winograd GEMMs' tile (fewest loads per MFMA) */
#define KFN_CFG_256x16 10  /* 16-column tiles on v_mfma_f32_16x16x4_f32 for the 16-channel layers */
#define KFN_CFG_128x16 11  /* (fp32 operands, no fused head epilogue)                               */
#define KFN_CFG_256x64 12  /* 4 waves side by side in M, wave tile 64x64: the fp16-activation kernels on 64-channel layers */
#define KFN_CFG_256x256 13    /* fp16 activations only: 4 waves, wave tile 128x128 (16 accumulators = 256 registers, one wave
                               * per SIMD): half the LDS fragment reads and half the operand staging per MFMA of 128x256 */
#define KFN_CFG_256x256_W8 14 /* fp16 activations only: 8 waves (2 x 4), wave tile 128x64, two waves per SIMD */
#define KFN_CFG_512x64 15     /* fp16 activations only: 4 waves side by side in M, wave tile 128x64 (64-channel layers) */

int kfn_conv2d_nhwc(const kfn_conv_desc* desc, const float* x, const float* w_packed,
                    const float* bias /* [Cout] or NULL */, float* y, void* stream);
/* 3x3 stride-1 SAME convolution 64 -> 64 channels on fp16 activations (x_dtype = y_dtype = KFN_ACT_F16, operand_dtype =
 * KFN_OPERAND_F16; SCoordNet's conv1b in BASELINE config 5, cnn_wrapper/SCoordNet.py:20): the weights stay in registers for
 * a workgroup's life, the workgroup walks down a strip of 128 / 192 pixels and reads every input row from the LDS once for
 * the three output rows it feeds (csrc/kfn_conv64.hip).  Same arithmetic as kfn_conv2d_nhwc on that descriptor (fp16
 * products, fp32 accumulation, bias, ReLU, one RNE rounding), another summation order.  w_packed = [2][36][64][8] halfs
 * (kfnet_amd.graph.pack_conv64_rows_kernel); x, y, w_packed, bias 16-byte aligned; ldx, ldy multiples of 8 elements.
 * kfn_conv3x3_c64_f16_supported(desc) = 1 when the launch takes the layer (KFN_ERR_UNSUPPORTED otherwise). */
int kfn_conv3x3_c64_f16_supported(const kfn_conv_desc* desc);
int kfn_conv3x3_c64_f16(const kfn_conv_desc* desc, const void* x, const void* w_packed, const float* bias, void* y,
                        void* stream);
/* Output spatial size for a descriptor (TF SAME rule); host-side shape inference. */
int kfn_conv2d_out_shape(const kfn_conv_desc* desc, int* Ho, int* Wo);
/* Which kernel instantiation kfn_conv2d_nhwc will launch for `desc`: tile config
 * (KFN_CFG_*), k-step (16|32) and workgroup count.  Used by bench.py to attribute
 * measured launch times to kernel names. */
int kfn_conv2d_plan(const kfn_conv_desc* desc, int* config, int* bk, int* tiles);

/* Which entry points the default graph (kfnet_amd.KFNet / KFNetEngine) launches, and which it does not
 *   ON the default route: kfn_first_conv_u8[_ex], kfn_conv2d_nhwc, kfn_conv3x3_c64_f16 (config 5), kfn_conv2d_winograd_fused, kfn_conv2d_winograd_f43,
 *     kfn_conv2d_winograd_s2, kfn_pad_nhwc, kfn_oflow_head[_f16], kfn_oflow_tail2[_f16], kfn_kalman_scan[_ex], kfn_eval_metrics,
 *     kfn_send_state / kfn_recv_state (multi-GPU), kfn_copy_channels (concat fallback).
 *   LEGACY -- earlier forms of the same operators, superseded on the default route, kept as tested stand-alone
 *     operators (and reachable through the Graph switches named in DESIGN.md): kfn_conv2d_winograd (+
 *     kfn_winograd_workspace_bytes / kfn_winograd_plan: the two-kernel Winograd form), kfn_cost_volume (materialising),
 *     kfn_cost_volume_conv (volume generated in conv0's loader), kfn_cost_volume_gather, kfn_flow_softargmax,
 *     kfn_flow_head, kfn_oflow_tail.  A maintainer wiring the reference to this library needs none of them.
 *   Reference API beside eval.py's path: kfn_kalman_fuse, kfn_kalman_fuse2 (KFNet.BuildKFCoord / GetKFCoord2 alone).
 *   The single-network programs (SCoordNet/eval.py, OFlowNet/eval.py) add kfn_coord_records / kfn_flow_records (ABI 12). */

/* [LEGACY: two-kernel form]  Winograd F(2x2,3x3) variant for 3x3 stride-1 SAME convolutions (same arguments and
 * result as kfn_conv2d_nhwc up to fp32 round-off, 2.25x fewer MFMA FLOPs): 16 GEMMs on the
 * MFMA kernel with the B^T d B input transform evaluated in its loader, then A^T M A +
 * bias + ReLU.  u_packed = [16][cout_pad][Cin], group g = 4*xi+nu holding (G g G^T)[xi][nu]
 * transposed to [co][ci]; workspace >= kfn_winograd_workspace_bytes(desc).
 * phases: 3 = whole convolution; 1 = only the 16 GEMMs, 2 = only the output transform
 * (lets a profiler time the two kernels separately). */
int kfn_winograd_workspace_bytes(const kfn_conv_desc* desc, size_t* bytes);
int kfn_winograd_plan(const kfn_conv_desc* desc, int* config, int* bk, int* tiles); /* cf. kfn_conv2d_plan */
int kfn_conv2d_winograd(const kfn_conv_desc* desc, const float* x, const float* u_packed,
                        const float* bias, float* y, float* workspace, int phases, void* stream);

/* Single-kernel variant of the above (csrc/kfn_wino2.hip): one wavefront = one workgroup owns a
 * block of 8x4 Winograd tiles x 32 output channels x all 16 (xi,nu) positions (16 accumulators
 * of 32x32 in registers), evaluates B^T d B on raw input patches staged once through LDS and
 * A^T M A in registers -- no workspace, no second kernel, every input pixel fetched once per
 * workgroup.  Same result as kfn_conv2d_winograd up to fp32 summation order.
 * u2_packed = [Cin/8][16][cout_pad][8]: the (G g G^T)[xi][nu] of kfn_conv2d_winograd, re-packed so
 * that the 32-channel fragment of one (8-channel k-chunk, position) is one contiguous 1 KiB read:
 *   u2[((ci/8)*16 + 4*xi+nu)*cout_pad + co][ci%8].
 * Needs Cin % 16 == 0, (H+1)/2 >= 4, cout_pad % 32 == 0, no fused head epilogue
 * (kfn_winograd_fused_supported() == 1); KFN_ERR_UNSUPPORTED otherwise.  Layers with Cout >= 128 and
 * Cin % 32 == 0 run in the four-wave form (csrc/kfn_wino3.hip: one input transform per 128 output channels,
 * shared through LDS); layers with 33 .. 64 output channels and Cin % 16 == 0 in its two-wave form (one transform
 * and one read of the input for all their channels; two images of the input below 1 GiB).  operand_dtype KFN_OPERAND_F16 (BASELINE config 5; four-wave form only, Cin % 64 == 0): u2_packed holds
 * IEEE halfs in the same layout, the input transform runs in fp32 on the fp32 activations and is rounded to fp16
 * when it is shared, the products are fp16 MFMAs with fp32 accumulation. */
int kfn_winograd_fused_supported(const kfn_conv_desc* desc);
int kfn_conv2d_winograd_fused(const kfn_conv_desc* desc, const float* x, const void* u2_packed,
                              const float* bias, float* y, void* stream);

/* 3x3 STRIDE-2 'same' convolution of an image with even H and W (tf.layers.conv2d(3, strides=2, 'same'),
 * cnn_wrapper/network.py:116-135: SCoordNet conv2a / conv3a / conv4a, cnn_wrapper/SCoordNet.py:12-27) by
 * polyphase decomposition + F(2,2) minimal filtering: 25 instead of 36 multiplies per 2x2 outputs, one launch,
 * no workspace (csrc/kfn_wino_s2.hip).  u2_packed = the 16 pre-transformed, pre-signed weight fragments
 * [Cin/8][16][cout_pad][8] (fragments 0-8: G g00 G^T of the taps w[2a][2b]; 9-11: G (w[0][1], w[2][1]);
 * 12-14: G (w[1][0], w[1][2]); 15: w[1][1]; the fragments of Winograd index 2 negated) -- kfnet_amd.graph.
 * pack_winograd_s2_kernel.  kfn_conv_desc.wino_form = KFN_WINO_FORM_S2_EIGHT_WAVE launches wino_s2b_kernel instead (two waves
 * per SIMD on 16x16x4 MFMA tiles, fp32 operands only, 1.5-2.5 % faster: what the default graph does); its weights are packed
 * per PAIR of fragments: u2b[((ci/8)*8 + f/2)*cout_pad + co][4*((ci%8)/2) + 2*(f%2) + ci%2]
 * (kfnet_amd.graph.pack_winograd_s2_kernel_b).  Needs Cin % 16 == 0, H and W even, H >= 14, cout_pad % 32 == 0, no fused head
 * epilogue (kfn_winograd_s2_supported() == 1); KFN_ERR_UNSUPPORTED otherwise.  operand_dtype KFN_OPERAND_F16
 * (BASELINE config 5): u2_packed holds IEEE halfs in the same layout, the input transform runs in fp32 and is
 * rounded to fp16 when it is shared, fp16 MFMAs with fp32 accumulation. */
int kfn_winograd_s2_supported(const kfn_conv_desc* desc);
int kfn_conv2d_winograd_s2(const kfn_conv_desc* desc, const float* x, const void* u2_packed, const float* bias,
                           float* y, void* stream);
/* Split-K form of the eight-wave stride-2 kernel (fp32 operands, u2b_packed = the pair packing; Cout % 4 == 0, ldy % 4 == 0,
 * y 16-byte aligned) for launches that leave the chip partly idle: semantics, workspace layout ([k_split][N*Ho*Wo][Cout]
 * floats) and determinism exactly as kfn_conv2d_winograd_f43_splitk below; the planes are reduced by the same second kernel. */
int kfn_winograd_s2_splitk_workspace_bytes(const kfn_conv_desc* desc, int k_split, size_t* bytes);
int kfn_conv2d_winograd_s2_splitk(const kfn_conv_desc* desc, const float* x, const void* u2b_packed, const float* bias,
                                  float* y, float* workspace, int k_split, void* stream);

/* Winograd F(4x4,3x3) for the same 3x3 stride-1 'same' convolutions (csrc/kfn_wino4.hip, round 4): 36 products per
 * 4x4 outputs -- 2.25 multiplies per output instead of 4 (F(2x2,3x3)) or 9 (direct) -- interpolation points
 * {0, +-1, +-2}, fp32 throughout, one launch, no workspace.  Meant for the layers with Cin >= 512 (SCoordNet conv3b /
 * conv4b / conv5, cnn_wrapper/SCoordNet.py:26-30), where the K loop amortises the larger transforms; the result differs
 * from kfn_conv2d_nhwc by ~3x the F(2x2,3x3) round-off (1.4e-6 on the network's coordinates, tools/experiments/
 * f43_error_budget.py).  u4_packed = [Cin/8][36][cout_pad][8]: U[6 xi + nu] = (G g G^T)[xi][nu] in fp64, rounded once,
 * u4[((ci/8)*36 + 6*xi+nu)*cout_pad + co][ci%8] (kfnet_amd.graph.pack_winograd_f43_kernel).
 * Two kernels behind the entry point, chosen by kfn_conv_desc.wino_form, and the weight layout goes with the choice:
 *   KFN_WINO_FORM_AUTO / KFN_WINO_FORM_F43_FOUR_WAVE: wino4_kernel, four waves on 32x32x2 MFMA tiles, the layout above;
 *   KFN_WINO_FORM_F43_EIGHT_WAVE: wino4b_kernel, two waves per SIMD on 16x16x4 tiles (3-13 % faster: what the default graph
 *     launches), u4_packed = [Cin/8][18 position pairs][cout_pad][4 k][2 positions][2 k-steps]:
 *     u4b[((ci/8)*18 + p/2)*cout_pad + co][4*((ci%8)/2) + 2*(p%2) + ci%2], p = 6*xi+nu
 *     (kfnet_amd.graph.pack_winograd_f43_kernel_b) -- same U, same size, a lane's operands of two positions contiguous.
 * Needs Cin % 16 == 0, H >= 29, Cout % 4 == 0, ldy % 4 == 0, ldx % 2 == 0, y 16-byte aligned, two images of the input
 * below 1 GiB, fp32 operands and activations, no fused head epilogue (kfn_winograd_f43_supported() == 1);
 * KFN_ERR_UNSUPPORTED otherwise. */
int kfn_winograd_f43_supported(const kfn_conv_desc* desc);
/* What a Winograd entry point will launch for `desc` -- the launch plan.  Every launcher above computes exactly this struct
 * first (one function per kernel family, csrc/kfn_wino*.hip) and launches from it; the *_supported functions answer "the plan
 * succeeds", kfn_winograd_lds_bytes answers its lds_bytes: nothing states a condition a second time.
 *   family     stride 2 -> kfn_conv2d_winograd_s2; stride 1 with wino_form KFN_WINO_FORM_F43_* -> kfn_conv2d_winograd_f43; any
 *              other stride-1 descriptor -> kfn_conv2d_winograd_fused.
 *   k_split    0: the plain entry point.  >= 1: the family's split-K entry point with that split (kfn_conv2d_winograd_f43_splitk /
 *              _s2_splitk; the fused family has none); k_split == 1 is the unsplit eight-wave launch.
 *   cu_count   compute units of the device (kfn_device_info); <= 0: 256.  Only the F(4,2) form reads it (its persistent kernel
 *              runs launches of at least two workgroups per CU).
 *   y_low_bits the low four bits of the output address (0 = 16-byte aligned) -- the one pointer fact that selects a path (the
 *              16-byte or the dword store epilogue) or, for the kernels without a dword epilogue, refuses the layer.  For a
 *              tensor window: 4 * (channel offset % 4).
 * plan->struct_size = sizeof(kfn_wino_plan) as the caller compiled it; the library writes that many bytes.  Returns KFN_OK, or
 * the launcher's own refusal (code and kfn_last_error text).  What a launcher checks beyond the plan is the alignment of the
 * other pointers (x, the packed weights, bias, the split-K workspace).  Host only: no device access. */
#define KFN_WINO_KERNEL_WINO2_WIDE 1   /* wino2_kernel<true>: 16-byte stores */
#define KFN_WINO_KERNEL_WINO2_DWORD 2  /* wino2_kernel<false> */
#define KFN_WINO_KERNEL_WINO3 3        /* wino3_kernel<false> */
#define KFN_WINO_KERNEL_WINO3_F16 4    /* wino3_kernel<true>: fp16 operands */
#define KFN_WINO_KERNEL_WINO3_PAIR 5   /* wino3_pair_kernel */
#define KFN_WINO_KERNEL_WINO4 6        /* wino4_kernel */
#define KFN_WINO_KERNEL_WINO4B 7       /* wino4b_kernel */
#define KFN_WINO_KERNEL_S2 8           /* wino_s2_kernel<false> */
#define KFN_WINO_KERNEL_S2_F16 9       /* wino_s2_kernel<true>: fp16 operands */
#define KFN_WINO_KERNEL_S2B 10         /* wino_s2b_kernel */
#define KFN_WINO_KERNEL_S2C 11         /* wino_s2c_kernel */
#define KFN_WINO_KERNEL_S2C_PERSISTENT 12 /* wino_s2c_pkernel */
typedef struct kfn_wino_plan {
  int32_t struct_size;
  int32_t kernel;              /* KFN_WINO_KERNEL_* */
  int32_t threads;             /* per workgroup */
  int32_t lds_bytes;           /* dynamic LDS per workgroup */
  int32_t workgroups;          /* launched: tiles_m * tiles_n * k_split, or cu_count for the persistent kernel */
  int32_t tiles_m, tiles_n;    /* tile blocks (the batch's tile rows packed) x output-channel groups */
  int32_t tiles_per_block;     /* Winograd tiles of a tile block: what tiles_m pads the image to */
  int32_t channels_per_group;  /* output channels of a workgroup: what tiles_n pads Cout to */
  int32_t n_group;             /* channel groups of one tile block adjacent in the grid (1 = tile blocks fastest) */
  int32_t wide_store;          /* 1: 16-byte store epilogue, 0: the dword one */
  int32_t k_split;             /* copies of the tile grid (1 = unsplit) */
  int32_t ss_per_split;        /* super-steps of 16 input channels per copy (fused family: of its own super-step) */
} kfn_wino_plan;
int kfn_winograd_launch_plan(const kfn_conv_desc* desc, int k_split, int cu_count, unsigned y_low_bits, kfn_wino_plan* plan);
/* Dynamic LDS (bytes per workgroup) of the kernel the matching Winograd entry point launches for `desc`: the lds_bytes of
 * kfn_winograd_launch_plan(desc, 0, 0, 0, ..).  A host compares it with kfn_device_info()'s lds_bytes_per_cu and routes around
 * kernels the device cannot hold (147-157 KB for the F(4x4,3x3) and four-wave F(2x2,3x3) forms) instead of failing in the
 * first launch.  No device access.  (ABI 6) */
int kfn_winograd_lds_bytes(const kfn_conv_desc* desc, int* bytes);
/* Split-K form of the eight-wave kernel for launches that would leave the chip idle (BASELINE configs[1], one 480x640 frame:
 * SCoordNet conv4b / conv5 / conv6 at batch 1 are 160 / 80 / 40 workgroups on 256 CUs, cnn_wrapper/SCoordNet.py:27-30): the
 * input channels are cut into k_split runs of ceil(Cin / 16 / k_split) super-steps, k_split copies of the tile grid write raw
 * partial sums into the planes of `workspace` ([k_split][N*H*W][Cout] floats, kfn_winograd_f43_splitk_workspace_bytes), a
 * second kernel adds the planes in the fixed order 0 .. k_split-1, then bias and ReLU, into y -- two stream-ordered launches,
 * no atomics, bit-stable from run to run.  u4b_packed = the eight-wave packing (kfnet_amd.graph.pack_winograd_f43_kernel_b);
 * 1 <= k_split <= Cin / 16 with no empty run; k_split == 1 is kfn_conv2d_winograd_f43's eight-wave launch (workspace unused).
 * The result differs from the unsplit launch by the summation order over the input channels only. */
int kfn_winograd_f43_splitk_workspace_bytes(const kfn_conv_desc* desc, int k_split, size_t* bytes);
int kfn_conv2d_winograd_f43_splitk(const kfn_conv_desc* desc, const float* x, const float* u4b_packed, const float* bias,
                                   float* y, float* workspace, int k_split, void* stream);
int kfn_conv2d_winograd_f43(const kfn_conv_desc* desc, const float* x, const float* u4_packed, const float* bias,
                            float* y, void* stream);

/* ---- first layers: uint8 image -> (x-128)*0.00625 -> 3x3 conv, Cin = 3 --------------
 * Replaces SCoordNet.preprocess + conv1a (SCoordNet.py:20-21,34-37) and the feature
 * tower's preprocess + feat1 (KFNet/KFNet.py:317-320) in ONE pass over the image.
 * w1 [27][C1], w2 [27][C2] = the TF HWIO kernels flattened (kh,kw,ci major, co minor).
 * C1, C2 multiples of 16; C2 may be 0 (then w2/b2/y2 are ignored).  ReLU is fused. */
int kfn_first_conv_u8(const uint8_t* img, int N, int H, int W,
                      const float* w1, const float* b1, float* y1, int C1,
                      const float* w2, const float* b2, float* y2, int C2, void* stream);
/* The same with the FIRST head's output element type chosen (KFN_ACT_F32 | KFN_ACT_F16): BASELINE config 5 keeps
 * SCoordNet's activations in fp16 from conv1a on (C1 == 64); the second head (feat1) stays fp32. */
int kfn_first_conv_u8_ex(const uint8_t* img, int N, int H, int W,
                         const float* w1, const float* b1, void* y1, int C1, int y1_dtype,
                         const float* w2, const float* b2, float* y2, int C2, void* stream);

/* ---- [LEGACY: materialising]  KFNet.BuildCoordVolume + reshape (KFNet/KFNet.py:343-359, :372) ----
 * vol[n, y, x, i, j, c] = f2[n,y,x,c] - f1[n, y+i-w/2, x+j-w/2, c]  (0 outside).
 * f1, f2: [N,H,W,C] (C % 4 == 0); vol: [N*H*W, window, window, C]. */
int kfn_cost_volume(const float* f1, const float* f2, float* vol, int N, int H, int W, int C,
                    int window, void* stream);

/* [LEGACY: Graph.factor_cost_volume = False]  BuildCoordVolume fused into OFlowNet's first conv (cnn_wrapper/OFlowNet.py:19, 3x3 SAME on
 * the 8x8 window grid): y[p, i, j, :] = act(conv0(vol)[p, i, j, :]) with vol generated inside
 * the MFMA kernel's loader (window fixed at 8, kernel 3x3); the 39 MB/frame volume never
 * exists in HBM.  f1, f2 [N,H,W,C] (C % 16 == 0); w_packed [cout_pad][9*C] as for
 * kfn_conv2d_nhwc; y [N*H*W, 8, 8, Cout] with pixel stride ldy. */
int kfn_cost_volume_conv(const float* f1, const float* f2, const float* w_packed, const float* bias,
                         float* y, int N, int H, int W, int C, int Cout, int cout_pad, int ldy,
                         int relu, int config, void* stream);

/* ---- factored cost volume + conv0 ---------------------------------------------------------
 * conv0 (cnn_wrapper/OFlowNet.py:19) is linear and V[p,cell] = f2[p] - f1[p+cell-4]
 * (KFNet/KFNet.py:343-359), hence conv0(V)[p,ci,cj] = b + S_k f2[p] - G_k(p+(ci-4,cj-4)) with
 * k = 3*rowclass(ci) + colclass(cj) (which taps stay inside the 8x8 window), S_k the sum of
 * those taps and G_k the 3x3 SAME conv of the zero-extended f1 with them.  T = b + S f2
 * [N,H,W,9*C] and Gp = G on the map extended by 2 [N,H+4,W+4,9*C] come from kfn_conv2d_nhwc
 * (kfn_pad_nhwc pads f1 by 2); this launch gathers, subtracts and applies the ReLU into the
 * [(N*H*W),8,8,C] tensor conv0 used to produce (pixel stride ldy). */
int kfn_pad_nhwc(const float* x, float* y, int N, int H, int W, int C, int pad, void* stream);
/* [LEGACY: Graph.fuse_oflow_window = False -- kfn_oflow_head / kfn_oflow_tail2 evaluate T - G where they need it] */
int kfn_cost_volume_gather(const float* T, const float* Gp, float* y, int N, int H, int W, int C,
                           int ldy, int relu, void* stream);

/* ---- [LEGACY: debug_prob path]  softmax over the window cells + soft-argmax flow ---------
 * OFlowNet.GetOutput softmax (OFlowNet.py:45-47) + KFNet.BuildOFlowNet flow
 * (KFNet/KFNet.py:381-385): flow[p] = sum_k softmax(logits[p])_k * (j-w/2, i-w/2).
 * logits [P, window*window] (row-major i,j); flow_xy [P,2]; prob [P,window^2] or NULL. */
int kfn_flow_softargmax(const float* logits, float* flow_xy, float* prob, int P, int window,
                        void* stream);

/* ---- [LEGACY: Graph.fuse_oflow_tail = False]  fused flow head: 'prediction' conv + softmax + soft-argmax ----
 * cnn_wrapper/OFlowNet.py:41 (3x3 conv C->1, SAME, no ReLU on the 8x8 window grid) +
 * OFlowNet.py:45-47 + KFNet/KFNet.py:381-385 in one kernel; the 64 logits stay on chip.
 * x [P,8,8,C] (C % 4 == 0, C <= 32); w [3,3,C] = the TF kernel [3,3,C,1] flattened;
 * bias [1] or NULL; flow_xy [P,2]; opt_logits [P,64] or NULL (debug). */
int kfn_flow_head(const float* x, const float* w, const float* bias, float* flow_xy,
                  float* opt_logits, int P, int C, void* stream);

/* [LEGACY: Graph.fuse_oflow_window = False]  OFlowNet's tail for every window in ONE launch: conv6 (3x3, 48 -> 16, ReLU; cnn_wrapper/OFlowNet.py:36-40) on
 * x = concat0 [P,8,8,48], the 'prediction' conv (3x3, 16 -> 1, linear; OFlowNet.py:41), the softmax over the 64
 * cells (OFlowNet.py:45-47) and the soft-argmax flow (KFNet/KFNet.py:381-385) -> flow_xy [P,2] (and the 64 logits
 * per window into opt_logits when given).  One wave per window, the patch resident in LDS, conv6's weights in
 * registers (csrc/kfn_oflow_tail.hip).  w6_packed = [108][64] per-lane fragments (kfnet_amd.graph.
 * pack_oflow_tail_kernel), wp = [3][3][16].  Only c_in = 48, c_mid = 16 (KFN_ERR_UNSUPPORTED otherwise). */
int kfn_oflow_tail(const float* x, const float* w6_packed, const float* b6, const float* wp, const float* bp,
                   float* flow_xy, float* opt_logits, int P, int c_in, int c_mid, void* stream);

/* ---- OFlowNet's two window-grid ends, window-resident (csrc/kfn_oflow_fused.hip) -------------------------
 * Both take the per-pixel maps of the factored cost volume (see kfn_cost_volume_gather): T [N,H,W,9*32] and
 * Gp [N,H+4,W+4,9*32], and evaluate conv0's cells (cnn_wrapper/OFlowNet.py:19 on the volume of
 * KFNet/KFNet.py:343-359) where they need them -- conv0's [N*H*W,8,8,32] output never exists in memory.
 *   kfn_oflow_head : conv0 -> conv1a (3x3 stride 2, 32 -> 32, ReLU; OFlowNet.py:20) -> y [N*H*W,4,4,32].
 *                    w1_packed [144][64] per-lane fragments (kfnet_amd.graph.pack_oflow_head_kernel).
 *   kfn_oflow_tail2: upconv0 (conv2d_transpose 3x3 stride 2, 32 -> 16, ReLU; OFlowNet.py:37) of x5 = conv5's
 *                    output [N*H*W,4,4,32], concat0 = [upconv0 | conv0], conv6, 'prediction', softmax, soft-argmax
 *                    (as kfn_oflow_tail) -> flow_xy [N*H*W,2].  wu_packed [72][64] (pack_oflow_upconv_kernel),
 *                    w6_packed / wp as for kfn_oflow_tail.
 * relu0 = conv0's activation flag.  One wave per window; all weights in registers; exact fp32 MFMAs. */
int kfn_oflow_head(const float* T, const float* Gp, int N, int H, int W, int relu0, const float* w1_packed,
                   const float* b1, float* y, void* stream);
/* kfn_oflow_head for BASELINE config 5: conv1a multiplies on v_mfma_f32_16x16x16_f16 (operands rounded to halfs where the
 * MFMA reads them / by the packer; conv0's T - G, the accumulation, bias and ReLU fp32; y fp32).  w1_packed_f16 =
 * [36][64][4] halfs (kfnet_amd.graph.pack_oflow_head_kernel_f16). */
int kfn_oflow_head_f16(const float* T, const float* Gp, int N, int H, int W, int relu0, const void* w1_packed_f16,
                       const float* b1, float* y, void* stream);
int kfn_oflow_tail2(const float* T, const float* Gp, int N, int H, int W, int relu0, const float* x5,
                    const float* wu_packed, const float* bu, const float* w6_packed, const float* b6,
                    const float* wp, const float* bp, float* flow_xy, float* opt_logits, void* stream);
/* kfn_oflow_tail2 for BASELINE config 5 ("fp16 convs"): upconv0 and conv6 multiply on v_mfma_f32_16x16x16_f16 -- their
 * operands are rounded to IEEE halfs (activations where the MFMA reads them, to nearest even; the weights by the packer), the
 * accumulation, conv0's T - G, the ReLUs, 'prediction', softmax and soft-argmax stay fp32.  wu_packed_f16 = [18][64][4]
 * halfs (kfnet_amd.graph.pack_oflow_upconv_kernel_f16), w6_packed_f16 = [27][64][4] halfs (pack_oflow_tail_kernel_f16);
 * every other argument as for kfn_oflow_tail2. */
int kfn_oflow_tail2_f16(const float* T, const float* Gp, int N, int H, int W, int relu0, const float* x5,
                        const void* wu_packed_f16, const float* bu, const void* w6_packed_f16, const float* b6,
                        const float* wp, const float* bp, float* flow_xy, float* opt_logits, void* stream);

/* ---- the recurrent part: warp + Kalman predict/update + NIS + transform/emit ----------
 * One launch scans T frames of S independent sequences (one workgroup per sequence,
 * state resident in LDS when it fits).  Per frame and pixel, in this order:
 *   KFNet.BuildOFlowNet tail (KFNet/KFNet.py:386-401): pixel_map = (x,y)+flow;
 *     x^- = bilinear(last_coord), s_l = bilinear(last_unc) (tools/util.py:36-93,
 *     clamped corners AND clamped-corner weights); P^- = max(s_l^2,eps^2)+max(s_t^2,eps^2)
 *   KFNet.BuildKFCoord (KFNet/KFNet.py:148-162): K = P^-/(P^-+R), x = max(1-K,0) x^- + K z
 *   KFNet.GetNIS (KFNet/KFNet.py:164-184)
 *   eval.py:87-126: reset when (t0+t) % reset_period == 0 (state := measurement),
 *     optional NIS gate on the OUTPUT only, record = (T.x, 1/sigma) via ApplyTransform
 *     (KFNet/util.py:12-40).
 * Grids above 10 240 pixels (state > 160 KB) run one launch per frame with the state
 * ping-ponging between `state` and `scratch`, a second copy of the state the CALLER provides
 * (kfn_kalman_scan_scratch_bytes; 0 bytes -- scratch may be NULL -- for every grid that fits
 * the LDS, which includes BASELINE's 60x80 and 68x120); results are the same function of the
 * inputs.
 */
typedef struct kfn_kalman_desc {
  int32_t S, T, H, W;
  int32_t t0;            /* global index of frame 0 of this call (reset phase) */
  int32_t reset_period;  /* eval.py: spec.sequence_length (500); <=0 = never reset */
  double min_uncertainty; /* KFNet.min_uncertainty = 1e-5, as the Python double: the variance floor is the double product
                            rounded once, float(1e-5 * 1e-5) = 0x2EDBE6FF (KFNet/KFNet.py:394,398), not 1e-5f * 1e-5f */
  float nis_gate;        /* 0 = off; eval.py --NIS uses 7.815 */
  int32_t has_transform; /* 0 = identity */
  float transform[12];   /* first 3 rows of inv(transform.txt), row-major */
} kfn_kalman_desc;

int kfn_kalman_scan_scratch_bytes(const kfn_kalman_desc* desc, size_t* bytes);
/* Which kernel instantiation kfn_kalman_scan[_ex] will launch for `desc` (cf. kfn_conv2d_plan); the launcher decides by the
 * same function.  No device access.  Only H and W decide (S > 0, H > 1, W > 1 as for the scan); with_optional_outputs != 0
 * describes a call that passes opt_temp, opt_nis or opt_kf, which gets the instantiation with those stores compiled in.
 *   form 1: H*W <= 5120, both state copies in the LDS          production 1024 threads x 5 pixels, optional outputs 768 x 7
 *   form 2: H*W <= 6144, one LDS copy, mid-frame barrier        1024 x 6  / 512 x 12
 *   form 3: H*W <= 8192, likewise                               1024 x 8  / 512 x 16
 *   form 4: H*W <= 10240, likewise                              1024 x 10 / 512 x 20
 *   form 5: above, one launch per frame, state through `scratch` (kfn_kalman_scan_scratch_bytes != 0 exactly here);
 *           threads = 256, pixels_per_thread = 1
 * threads * pixels_per_thread >= H*W in forms 1-4 (one workgroup per sequence). */
int kfn_kalman_scan_plan(const kfn_kalman_desc* desc, int with_optional_outputs, int* form, int* threads,
                         int* pixels_per_thread);
int kfn_kalman_scan(const kfn_kalman_desc* desc,
                    const float* flow_xy,     /* [S,T,H*W,2] */
                    const float* sigma_trans, /* [S,T,H*W]   */
                    const float* meas,        /* [S,T,H*W,4] = (z, sigma_z) */
                    float* state,             /* [S,H*W,4] in/out = (x, sigma) raw KF state */
                    float* records,           /* [S,T,H*W,4] = (T.x, 1/sigma) */
                    float* opt_temp,          /* [S,T,H*W,4] = (x^-, sigma^-) or NULL */
                    float* opt_nis,           /* [S,T,H*W,3] or NULL */
                    void* scratch,            /* kfn_kalman_scan_scratch_bytes() bytes, 16-byte aligned, or NULL when 0 */
                    void* stream);

/* The same scan with the extra debug outputs eval.py's log line is computed from:
 *   opt_kf [S,T,H*W,4]  the raw KF estimate (x, sigma) of every frame BEFORE the NIS gate, the reset
 *                        override and ApplyTransform (what KF_loss / KF_accuracy see, KFNet/train.py:256-257);
 *   raw_on_reset != 0   on a reset step opt_temp / opt_nis / opt_kf hold what the GRAPH computes there from
 *                        the incoming state (KFNet/eval.py:78-83 runs before the host override of :94-101);
 *                        with 0 they hold (z, 0, z) as kfn_kalman_scan writes them.
 * State, records and the NIS gate are unaffected.  kfn_kalman_scan == kfn_kalman_scan_ex(.., NULL, 0, ..). */
int kfn_kalman_scan_ex(const kfn_kalman_desc* desc, const float* flow_xy, const float* sigma_trans,
                       const float* meas, float* state, float* records, float* opt_temp, float* opt_nis,
                       float* opt_kf, int raw_on_reset, void* scratch, void* stream);

/* ---- evaluation numbers of eval.py, reduced on the device --------------------------------
 * KFNet.CoordLossWithUncertainty(downsample=True) x3 (KFNet/KFNet.py:192-232 via KFNet/train.py:252-257),
 * the NIS band count (KFNet/eval.py:10-15) and the distance maps of dist_error (eval.py:17-29) for T
 * frames, one workgroup per frame.  Inputs are the scan's buffers [T,H*W,.] (meas, temp, kf_raw, records,
 * nis as written with raw_on_reset = 1) and `labels` [L,H*W,4] = (gt xyz, mask) already nearest-down-sampled
 * (tf.image.resize_nearest_neighbor: source pixel (8y, 8x)); label_pair [T,2] = label rows of the step's
 * frame pair (KFNet/train.py:67-71: the losses see BOTH, the distances the second); reset_flags [T].
 * stats [T,16]: [0..2] masked loss sums (measure, temporal, KF), [3..5] "inaccurate" pixel counts,
 * [6] valid_pixel = sum(mask_a) + sum(mask_b) + 1, [7] NIS values > 0, [8] of those inside (0.0157, 2.706);
 * loss = stats[k]/stats[6], accuracy = (stats[6] - stats[3+k])/stats[6].  dist_maps [T,3,H*W] in cm
 * (0 where masked); the host takes the medians of the positive entries.
 * dist_threshold is the Python double 0.05: it is squared in double and the product rounded once to fp32, as TensorFlow
 * does with `dist_threshold * dist_threshold` (KFNet.py:227) -- 0x3B23D70A; a caller that rounds 0.05 to float first gets
 * 0x3B23D70B and a pixel exactly 0.05f away counted accurate.  min_uncertainty is compared as float(min_uncertainty). */
int kfn_eval_metrics(const float* meas, const float* temp, const float* kf_raw, const float* records,
                     const float* nis, const float* labels, const int32_t* label_pair,
                     const uint8_t* reset_flags, const float* transform12 /* 3x4 row-major or NULL */,
                     int T, int HW, double dist_threshold /* 0.05 */, double min_uncertainty /* 1e-5 */,
                     float* stats, float* dist_maps, void* stream);

/* KFNet.BuildKFCoord on its own (KFNet/KFNet.py:148-162) + optional KFNet.GetNIS
 * (:164-184): pred = (x^-, sigma^-), meas = (z, sigma_z), out = (x, sigma), all [P,4];
 * opt_nis [P,3] or NULL.  48 B/pixel of HBM traffic (32 read + 16 written). */
int kfn_kalman_fuse(const float* pred, const float* meas, float* out, float* opt_nis, long P,
                    void* stream);

/* KFNet.GetKFCoord2 (KFNet/KFNet.py:487-502; not on eval.py's path): the same fusion with the posterior variance in
 * the symmetric form (1-K)^2 P^- + K^2 R.  pred / meas / out packed [P,4] = (x, y, z, sigma) as for kfn_kalman_fuse. */
int kfn_kalman_fuse2(const float* pred, const float* meas, float* out, long P, void* stream);

/* Self-check of the arithmetic inside kfn_kalman_scan (ABI 10): the scan computes its two square roots and two quotients per pixel
 * with the refinement steps of the IEEE forms but without their denormal pre-scaling (csrc/kfn_kalman.hip, sqrt_rn_normal /
 * div_rn_normal: the scan is VALU-bound).  out [n,4] = (lean sqrt(a), sqrtf(a), lean a / b, a / b): the pairs must be equal bit
 * for bit for normal-range operands, and for zero / infinity / NaN as IEEE defines them. */
int kfn_kalman_arith_probe(const float* a, const float* b, float* out, long n, void* stream);

/* ---- the graph-level helpers of the reference as stand-alone launches ----------------------------------------
 * On eval.py's path they are fused into the scan (kfn_kalman_scan: warp, fuse, transform in one kernel); these entry
 * points serve Python-level callers (KFNet/eval.py:57-59 calls ApplyTransform itself).  All tensors NHWC fp32 with a
 * pixel stride `ld_*` (floats) so that channel views of packed buffers can be passed.
 *   kfn_apply_transform   KFNet/util.py:12-40: out[p,0:3] = (T [x;1])[0:3], no perspective divide.  `transform` is a DEVICE
 *                         pointer to one 4x4 (per_batch = 0) or B 4x4 (per_batch = 1) row-major matrices.
 *   kfn_pixel_map         KFNet/util.py:42-63: out[b,y,x] = (x, y); normalize != 0: ((x - u) / focal_x, (y - v) / focal_y).
 *   kfn_bilinear_sampler  tools/util.py:3-94: imgs [B,Hs,Ws,C] sampled at coords [B,Ht,Wt,2] = (x, y) -> out [B,Ht,Wt,C];
 *                         corner indices clamped to the image AND weights taken from the clamped corners (so any sample
 *                         with x < 0 or x >= Ws-1 evaluates to 0, x = Ws-1 included), sum in tf.add_n order. */
int kfn_apply_transform(const float* coords, int ld_in, const float* transform, int per_batch, int B, int H, int W,
                        float* out, int ld_out, void* stream);
int kfn_pixel_map(float* out, int ld_out, int B, int H, int W, int normalize, float u, float v, float focal_x,
                  float focal_y, void* stream);
int kfn_bilinear_sampler(const float* imgs, int ld_img, int B, int Hs, int Ws, int C, const float* coords, int ld_coords,
                         int Ht, int Wt, float* out, int ld_out, void* stream);

/* ---- records of the single-network programs (ABI 12) ------------------------------------------------
 * SCoordNet/eval.py and OFlowNet/eval.py run one network each; these two element-wise launches turn its device output into
 * the rows their .npy files hold.  Both return KFN_ERR_ARG on a null pointer, P <= 0 or a misaligned pointer.
 *   kfn_coord_records  meas [P,ld_meas] = (x, y, z, sigma) (ld_meas >= 4, 4-byte aligned) -> out [P,4] = (T.x, 1/sigma)
 *                      (16-byte aligned): bit for bit the record kfn_kalman_scan emits on a reset frame.  T.x is
 *                      ((M0 x + M1 y) + M2 z) + M3 per row, every product and sum rounded on its own; 1/sigma is the scan's
 *                      quotient (correctly rounded for normal-range sigma; below 2^-96 it may differ from IEEE in the last
 *                      place, exactly as the scan's does).  transform12 = HOST pointer to the 3x4 row-major matrix (read
 *                      during the call), or NULL for the identity.
 *   kfn_flow_records   flow_xy [P,2] = (u, v) in grid cells, sigma_trans [P] -> out [P,3] = (u, v, 1/sigma_trans); all
 *                      4-byte aligned.  The division is IEEE binary32 1.0f / sigma_trans, correctly rounded (round to nearest
 *                      even, denormals kept): equal bit for bit to numpy's np.float32(1) / sigma. */
int kfn_coord_records(const float* meas, int ld_meas, const float* transform12, float* out, long P, void* stream);
int kfn_flow_records(const float* flow_xy, const float* sigma_trans, float* out, long P, void* stream);

/* ---- Network.concat fallback (cnn_wrapper/network.py:316-318): strided channel copy -- */
int kfn_copy_channels(const float* src, int ld_src, float* dst, int ld_dst, int P, int C,
                      void* stream);

/* ---- camera poses: batched RANSAC-PnP on the scan's records (ABI 11) -----------------------------------------------
 * No reference counterpart on the device: the reference hands coord_<i>.npy to an external PnP program (README.md:132-138)
 * that it does not ship.  records [B,h,w,ld] = (x, y, z, 1/sigma) in the scene frame (the scan's output, ld >= 4 floats per
 * cell); one camera-to-world pose per frame, everything on the device (DESIGN.md "Camera poses" fixes each step):
 *   correspondence   cell (r, c) observes image pixel (cell_stride*c, cell_stride*r) with pinhole intrinsics fx, fy, u, v;
 *                    it is a candidate iff 1/sigma > min_confidence and x, y, z are finite; candidates in raster order
 *   sampling         h = lowbias32(seed ^ frame*0x9E3779B1 ^ hyp*0x85EBCA77 ^ draw*0xC2B2AE3D), frame = t0 + b (global),
 *                    candidate (uint64(h) * n) >> 32; draws continue to 4 distinct indices, at most 16 draws
 *   hypothesis       P3P (Grunert's quartic, fp64) on the first three, the fourth picks the solution; no real solution or a
 *                    point behind the camera: invalid
 *   scoring          inlier iff camera-frame Z > 0 and the reprojection error < inlier_px full-resolution pixels (fp32)
 *   selection        most inliers, ties to the lowest hypothesis index
 *   refinement       refine_iters Gauss-Newton steps (so(3) + translation) over the inliers of the current pose, fp64
 *                    normal equations in a fixed order; a step is kept only if it lowers the cost over that inlier set
 * Results are bit-identical from launch to launch, and a frame's pose does not depend on the batch it is solved in. */
#define KFN_PNP_OK 0
#define KFN_PNP_TOO_FEW_POINTS 1     /* fewer than min_points candidates */
#define KFN_PNP_NO_HYPOTHESIS 2      /* no hypothesis survived sampling and P3P */
#define KFN_PNP_MAX_HYPOTHESES 1024
typedef struct kfn_pnp_desc {
  int32_t struct_size;     /* = sizeof(kfn_pnp_desc) as the caller compiled it; grows at its end like kfn_conv_desc */
  int32_t B, h, w;         /* frames, grid rows, grid columns (h * w <= 32768) */
  int32_t ld;              /* floats per cell in `records`, >= 4 */
  int32_t t0;              /* global index of frame 0 of this call (the sampling counter) */
  uint32_t seed;
  int32_t hypotheses;      /* 1 .. KFN_PNP_MAX_HYPOTHESES */
  int32_t refine_iters;    /* Gauss-Newton iterations, 0 .. 100 */
  int32_t min_points;      /* fewer candidates: KFN_PNP_TOO_FEW_POINTS; >= 4 */
  float fx, fy, u, v;      /* pinhole intrinsics of the full-resolution image */
  int32_t cell_stride;     /* pixels per grid cell (8) */
  float min_confidence;    /* 20, as tools/io.confident_points */
  float inlier_px;         /* 10 */
} kfn_pnp_desc;
/* kfn_pnp_desc d = KFN_PNP_DESC_INIT;  -- zero everything, set struct_size */
#define KFN_PNP_DESC_INIT {(int32_t)sizeof(kfn_pnp_desc)}

/* Bytes of the caller's scratch for a ransac call on `desc` (hypothesis poses and counts). */
int kfn_pnp_scratch_bytes(const kfn_pnp_desc* desc, size_t* bytes);
int kfn_pnp_ransac(const kfn_pnp_desc* desc, const float* records,
                   float* poses,          /* [B,16] camera-to-world, row-major; NaN where status != KFN_PNP_OK */
                   int32_t* info,         /* [B,4] = (status, candidates, final inliers, best hypothesis or -1) */
                   void* scratch,         /* the scratch-bytes query's size, 16-byte aligned */
                   void* stream);
/* Probe of the first two stages, for tests: samples [B,H,4] candidate indices (-1: no 4 distinct in 16 draws, or too few
 * candidates), hyp_poses [B,H,12] = [R | t] world-to-camera in fp32 (NaN: invalid), counts [B,H] inliers (-1: invalid). */
int kfn_pnp_hypotheses(const kfn_pnp_desc* desc, const float* records, int32_t* samples, float* hyp_poses, int32_t* counts,
                       void* stream);

/* ---- uncertainty-aware poses (added exports, the ABI number stays 13) -------------------------------------------------
 * kfn_pnp_ransac_unc is kfn_pnp_ransac with the records' sigma = 1 / record[3] carried into the last stage (DESIGN.md 5c,
 * "Uncertainty").  Candidates, sampling, P3P, scoring and selection are kfn_pnp_ransac's launches.  With camera point
 * (x, y, z) = R X + t, residual r and 2x6 Jacobian J of the refinement above:
 *   S   = sigma^2 A A^T + pixel_sigma^2 I,  A = [[fx/z, 0, -fx x/z^2], [0, fy/z, -fy y/z^2]]     (2x2, inverted in fp64)
 *   weighted = 1   every iteration forms H = sum J^T S^-1 J, g = sum J^T S^-1 r, cost = sum r^T S^-1 r over the inliers of
 *                  the current pose (the unweighted rule: Z > 0, pixel error < inlier_px), S evaluated at the current pose
 *                  and held fixed for the iteration; a step is kept only if no inlier goes behind the camera and the cost
 *                  over the same inliers with the same S falls
 *   weighted = 0   the refinement is kfn_pnp_ransac's: poses and info are the same bits
 *   cov            [B,36] = (sum J^T S^-1 J)^-1 at the final pose over the final inliers (info[:,2]), 6x6 row-major and
 *                  symmetric to the last bit, in the coordinates (omega, tau) of the left perturbation of the
 *                  world-to-camera pose, R <- exp(omega) R, t <- exp(omega) t + tau.  To first order this is the covariance
 *                  of the body-frame perturbation (dtheta, drho) = -(omega, tau) of the camera-to-world pose C that `poses`
 *                  holds, C ~ C_hat [exp(dtheta) | drho]; the camera centre's covariance in the scene frame is
 *                  R_c2w Sigma_tau,tau R_c2w^T.  NaN where status != KFN_PNP_OK, and where fewer than 3 inliers remain or
 *                  the Cholesky factorisation fails (the pose is still reported then).
 *   quality        [B,2] = (sum r^T S^-1 r at the final pose, 2 * inliers - 6); NaN where status != KFN_PNP_OK
 * cov and quality may be NULL.  min_confidence must be >= 0 (sigma positive).  Same scratch as kfn_pnp_ransac; bit-identical
 * from launch to launch. */
typedef struct kfn_pnp_unc_desc {
  int32_t struct_size;     /* = sizeof(kfn_pnp_unc_desc) as the caller compiled it */
  int32_t weighted;        /* 0: kfn_pnp_ransac's refinement; 1: weighted by S^-1 */
  float pixel_sigma;       /* > 0; the floor that keeps S invertible as sigma -> 0 (1.0 pixel) */
} kfn_pnp_unc_desc;
#define KFN_PNP_UNC_DESC_INIT {(int32_t)sizeof(kfn_pnp_unc_desc), 0, 1.0f}
int kfn_pnp_ransac_unc(const kfn_pnp_desc* desc, const kfn_pnp_unc_desc* unc, const float* records, float* poses, float* cov,
                       float* quality, int32_t* info, void* scratch, void* stream);

/* ---- guided sampling: hypotheses drawn by the maps' confidence (added exports, the ABI number stays 13) -----------------
 * kfn_pnp_ransac_guided is kfn_pnp_ransac / kfn_pnp_ransac_unc with one step changed: the four cells of a hypothesis are
 * drawn in proportion to an integer weight of their confidence instead of uniformly ("Guided sampling").
 * Candidates, the hash, the 16-draw limit, P3P, scoring, selection and refinement are unchanged.
 *   weight      c = record[3]; q = (int)floorf((fminf(c, confidence_cap) - min_confidence) * 16.0f) + 1 in binary32, every
 *               operation rounded to nearest; q >= 1, c = +inf takes the cap's weight.  w = q (KFN_PNP_SAMPLE_CONFIDENCE) or
 *               q * q (KFN_PNP_SAMPLE_CONFIDENCE_SQ), unsigned 64-bit.  0 <= min_confidence < confidence_cap <= 4096.
 *   cum         cum[i] = w[0] + .. + w[i] over the n candidates in raster order, uint64; total = cum[n-1] < 2^48
 *   draw        h as above; target = floor(h * total / 2^32), the exact integer; the candidate drawn is the first i with
 *               cum[i] > target.  With equal confidences this is (uint64(h) * n) >> 32: the uniform draw, bit for bit.
 *   unc         NULL: the refinement is kfn_pnp_ransac's, cov and quality must be NULL; otherwise kfn_pnp_ransac_unc's rules
 *   scratch     kfn_pnp_guided_scratch_bytes: kfn_pnp_scratch_bytes' arrays, then cum [B][h*w] uint64 and n [B]
 * kfn_pnp_hypotheses_guided is the probe (kfn_pnp_hypotheses' three outputs) and also returns cum [B][h*w] (row b: n[b]
 * entries are written) and n [B]; either may be NULL.  Bit-identical from launch to launch. */
#define KFN_PNP_SAMPLE_CONFIDENCE 1
#define KFN_PNP_SAMPLE_CONFIDENCE_SQ 2
typedef struct kfn_pnp_sample_desc {
  int32_t struct_size;     /* = sizeof(kfn_pnp_sample_desc) as the caller compiled it */
  int32_t mode;            /* KFN_PNP_SAMPLE_CONFIDENCE or KFN_PNP_SAMPLE_CONFIDENCE_SQ */
  float confidence_cap;    /* confidences above it weigh as it does (1000); finite, > min_confidence, <= 4096 */
} kfn_pnp_sample_desc;
#define KFN_PNP_SAMPLE_DESC_INIT {(int32_t)sizeof(kfn_pnp_sample_desc), KFN_PNP_SAMPLE_CONFIDENCE, 1000.0f}
int kfn_pnp_guided_scratch_bytes(const kfn_pnp_desc* desc, const kfn_pnp_sample_desc* sample, size_t* bytes);
int kfn_pnp_ransac_guided(const kfn_pnp_desc* desc, const kfn_pnp_sample_desc* sample, const kfn_pnp_unc_desc* unc,
                          const float* records, float* poses, float* cov, float* quality, int32_t* info, void* scratch,
                          void* stream);
int kfn_pnp_hypotheses_guided(const kfn_pnp_desc* desc, const kfn_pnp_sample_desc* sample, const float* records,
                              int32_t* samples, float* hyp_poses, int32_t* counts, uint64_t* cum, int32_t* n, void* scratch,
                              void* stream);

/* ---- poses with depth: RANSAC-Kabsch (added exports, the ABI number stays 13) ------------------------------------------
 * kfn_kabsch_ransac is the sibling of kfn_pnp_ransac for RGB-D frames ("Poses with depth").  Next to the records
 * it reads cam_points [B,h,w,ldp] = (Xc, Yc, Zc, mask): the camera-frame point, in metres, of the pixel that cell (r, c)
 * observes -- what kfn_depth_labels writes at stride 8 under the identity pose.  Every candidate cell is a 3-D/3-D
 * correspondence (camera point p, scene point x), and the pose is the rigid alignment x ~ R p + t, camera to world:
 *   candidates    1/sigma > min_confidence, x finite, mask == 1 and p finite; raster order; at most 32768 cells
 *   sampling      kfn_pnp_ransac's hash; draws continue to 3 distinct indices, at most 16 draws
 *   hypothesis    the least-squares rigid transform of the three pairs, det R = +1, in fp64 (Horn's quaternion form, cyclic
 *                 Jacobi on the symmetric 4x4); invalid if |(p1 - p0) x (p2 - p0)| < 1e-6 m^2 for the camera or the scene
 *                 triangle, or if the two largest eigenvalues lie within 1e-9 of the largest magnitude; [R|t] stored in fp32
 *   scoring       inlier iff |R p + t - x|^2 < inlier_m^2 (fp32, strict)
 *   selection     most inliers, ties to the lowest hypothesis index
 *   refinement    up to refine_iters rounds in fp64: the inliers of the current pose (strict <), then the closed form over
 *                 them with weights w = 1 (weighted = 0) or w = 1 / (sigma^2 + point_sigma^2) (weighted = 1), sigma =
 *                 1 / record[3]; a round with the inlier set of the round before ends the loop; fewer than 3 inliers or an
 *                 undetermined rotation keeps the previous pose and ends it
 *   poses         [B,16] camera-to-world, row-major; NaN where status != KFN_PNP_OK
 *   cov           [B,36] = (sum w J^T J)^-1 over the final inliers at the final pose, J = [-[q]x | I], q = R^T (x - t), w =
 *                 1 / (sigma^2 + point_sigma^2) in both modes: kfn_pnp_ransac_unc's coordinates (omega, tau), symmetric to the
 *                 last bit; NaN where status != KFN_PNP_OK, with fewer than 3 inliers or a failed Cholesky factorisation
 *   quality       [B,2] = (sum w |R p + t - x|^2 over the final inliers, 3 * inliers - 6); NaN where status != KFN_PNP_OK
 *   info          [B,4] = (status KFN_PNP_*, candidates, final inliers, selected hypothesis or -1)
 * cov and quality may be NULL.  Bit-identical from launch to launch; a frame's pose depends neither on its batch nor on its
 * position in it (frame = t0 + b).  No floating-point atomics. */
typedef struct kfn_kabsch_desc {
  int32_t struct_size;     /* = sizeof(kfn_kabsch_desc) as the caller compiled it */
  int32_t B, h, w;         /* frames, grid rows, grid columns (h * w <= 32768) */
  int32_t ld;              /* floats per cell in `records`, >= 4 */
  int32_t ldp;             /* floats per cell in `cam_points`, >= 4 */
  int32_t t0;              /* global index of frame 0 of this call (the sampling counter) */
  uint32_t seed;
  int32_t hypotheses;      /* 1 .. KFN_PNP_MAX_HYPOTHESES */
  int32_t refine_iters;    /* rounds of the closed-form refinement, 0 .. 100 */
  int32_t min_points;      /* fewer candidates: KFN_PNP_TOO_FEW_POINTS; >= 3 */
  float min_confidence;    /* 20; >= 0 */
  float inlier_m;          /* 0.10: the inlier distance in metres */
  int32_t weighted;        /* 0: w = 1 in the refinement; 1: w = 1 / (sigma^2 + point_sigma^2) */
  float point_sigma;       /* > 0, metres: the floor of a point's standard deviation (0.01) */
} kfn_kabsch_desc;
#define KFN_KABSCH_DESC_INIT {(int32_t)sizeof(kfn_kabsch_desc), 0, 0, 0, 4, 4, 0, 0u, 256, 10, 16, 20.0f, 0.10f, 0, 0.01f}
int kfn_kabsch_scratch_bytes(const kfn_kabsch_desc* desc, size_t* bytes);
int kfn_kabsch_ransac(const kfn_kabsch_desc* desc, const float* records, const float* cam_points, float* poses, float* cov,
                      float* quality, int32_t* info, void* scratch, void* stream);
/* Probe of the first two stages: samples [B,H,3] candidate indices (-1: no 3 distinct in 16 draws, or too few candidates),
 * hyp_poses [B,H,12] = [R | t] camera-to-world in fp32 (NaN: invalid), counts [B,H] inliers (-1: invalid). */
int kfn_kabsch_hypotheses(const kfn_kabsch_desc* desc, const float* records, const float* cam_points, int32_t* samples,
                          float* hyp_poses, int32_t* counts, void* stream);
/* Probe of the selection rule on its own: best [B] = the first index of the maximum of counts [B,hypotheses], -1 where
 * every count is negative -- what info[:,3] reports. */
int kfn_kabsch_select(const int32_t* counts, int B, int hypotheses, int32_t* best, void* stream);

/* Random-walk error-state filter over a sequence of such poses, one sequence per lane, fp64, serial over t.  State: (R, p)
 * camera-to-world and P (6x6, the body-frame coordinates (dtheta, drho) above).  flags [S,T]:
 *   KFN_POSE_UPDATED   0   the measurement passed the gate and was fused
 *   KFN_POSE_MISSING   1   no valid measurement (a non-finite pose or covariance, or P + Sigma_z not positive definite): the
 *                          output is the prediction; does not count towards a reset
 *   KFN_POSE_REJECTED  2   NIS > gate: the output is the prediction
 *   KFN_POSE_INIT      3   the state was (re-)initialised from this measurement: the first valid one, or the max_rejects-th
 *                          consecutive rejection
 *   KFN_POSE_NONE      4   no estimate yet: the outputs are NaN
 * Per frame: P <- P + diag(rot_sigma^2 I, trans_sigma^2 I); y = (log_SO3(R^T R_z), R^T (p_z - p)), S = P + Sigma_z,
 * NIS = y^T S^-1 y (the rotation between the state's and the measurement's body frames is neglected in S);
 * K = P S^-1, delta = K y, p <- p + R drho, then R <- R exp(dtheta), P <- (I - K) P (I - K)^T + K Sigma_z K^T.
 * poses / out_poses [S,T,16] row-major 4x4, cov / out_cov [S,T,36], nis [S,T] (NaN where no test was made). */
#define KFN_POSE_UPDATED 0
#define KFN_POSE_MISSING 1
#define KFN_POSE_REJECTED 2
#define KFN_POSE_INIT 3
#define KFN_POSE_NONE 4
typedef struct kfn_pose_filter_desc {
  int32_t struct_size;     /* = sizeof(kfn_pose_filter_desc) as the caller compiled it */
  int32_t S, T;            /* sequences, frames per sequence */
  float rot_sigma;         /* rad per frame (0.02), >= 0 */
  float trans_sigma;       /* metres per frame (0.02), >= 0 */
  float gate;              /* on the NIS; 22.46 is the 99.9 % point of chi^2 with 6 degrees of freedom; > 0 */
  int32_t max_rejects;     /* consecutive rejections that force a re-initialisation (3); >= 1 */
} kfn_pose_filter_desc;
#define KFN_POSE_FILTER_DESC_INIT {(int32_t)sizeof(kfn_pose_filter_desc), 0, 0, 0.02f, 0.02f, 22.46f, 3}
int kfn_pose_filter(const kfn_pose_filter_desc* desc, const float* poses, const float* cov, float* out_poses, float* out_cov,
                    int32_t* flags, float* nis, void* stream);

/* The pose tracker: kfn_pose_filter's recursion under one of two motion models, an optional backward pass, and a state that
 * is carried from call to call (added exports; kfn_pose_filter is unchanged).  One sequence per lane, fp64, serial over t.
 * Shapes and flags are kfn_pose_filter's; out_cov and smooth_cov [S,T,36] are the 6x6 pose block.
 *   model = KFN_POSE_MODEL_WALK      kfn_pose_filter word for word: with smooth = 0 and state = NULL the four outputs are its
 *                                    bits.  Error state (dtheta, drho), P 6x6.
 *   model = KFN_POSE_MODEL_VELOCITY  the state also holds a body-frame twist xi = (omega, v) per frame; error state (dtheta,
 *                                    drho, domega, dv), P 12x12.  Predict: p <- p + R v, then R <- R exp(omega), xi kept;
 *                                    P <- F P F^T + Q with F = [[I6, I6], [0, I6]] and, per axis, Q = [[q/3, q/2], [q/2, q]]
 *                                    on (pose axis, rate axis), q = rot_sigma^2 or trans_sigma^2.  Measurement H = [I6 0]:
 *                                    y, the gate, the reject count and the flags as kfn_pose_filter, S = P[:6,:6] + Sigma_z;
 *                                    K = P[:, :6] S^-1 (12x6), delta = K y, the pose takes delta[:6] as there,
 *                                    xi <- xi + delta[6:], P in Joseph form.  (Re-)initialisation: pose and pose block from
 *                                    the measurement, xi = 0, rate block diag(rot_rate_sigma^2 I3, trans_rate_sigma^2 I3),
 *                                    cross blocks 0.  A missing or rejected frame outputs the prediction, which has moved.
 *   smooth = 1   Rauch-Tung-Striebel smoothing over the T frames of this call into smooth_poses / smooth_cov.  The last frame's
 *                smoothed estimate is its filtered one; frame t is smoothed from t+1 if both hold an estimate, t+1 is not a
 *                (re-)initialisation (KFN_POSE_INIT) and its predicted P_p is positive definite:
 *                e = (log_SO3(R_p^T R_s), R_p^T (p_s - p_p), xi_s - xi_p) of t+1, C = P_f F^T P_p^-1, d = C e,
 *                p_s = p_f + R_f d_rho, R_s = R_f exp(d_theta), xi_s = xi_f + d_xi, P_s = P_f + C (P_s,t+1 - P_p,t+1) C^T;
 *                otherwise the filtered estimate.  Frames without an estimate give NaN.  smooth_poses, smooth_cov and scratch
 *                (kfn_pose_track_scratch_bytes; 0 bytes when smooth = 0) are all non-NULL with smooth = 1, and the two
 *                outputs are NULL with smooth = 0.
 *   state        kfn_pose_track_state_bytes of device memory, or NULL for a fresh state that is thrown away.  Per sequence, in
 *                fp64: have, rejects, R, p, xi (velocity model), P.  All zero means "no estimate yet".  Read at the start and
 *                written at the end of the call: T frames run in consecutive calls of any lengths give the forward outputs of
 *                one call bit for bit.  The layout depends on model and S; the backward pass covers the frames of its own
 *                call only.
 * Approximations: F takes the adjoint of exp(-xi) and the right Jacobian as the identity, and the smoother applies a
 * correction expressed in frame t+1's predicted body frame in frame t's (both first order in one frame's motion); S as
 * kfn_pose_filter.  Bit-identical from launch to launch. */
#define KFN_POSE_MODEL_WALK 0
#define KFN_POSE_MODEL_VELOCITY 1
typedef struct kfn_pose_track_desc {
  int32_t struct_size;     /* = sizeof(kfn_pose_track_desc) as the caller compiled it */
  int32_t S, T;            /* sequences, frames per sequence in this call */
  int32_t model;           /* KFN_POSE_MODEL_* */
  int32_t smooth;          /* 1: also the backward pass over the T frames of this call */
  float rot_sigma;         /* walk: rad per frame (0.02), as kfn_pose_filter; velocity: white acceleration per frame (0.005); >= 0 */
  float trans_sigma;       /* walk: metres per frame (0.02); velocity: white acceleration per frame (0.005); >= 0 */
  float rot_rate_sigma;    /* velocity: sigma of the unknown angular rate at (re-)initialisation, rad per frame (0.05); > 0 */
  float trans_rate_sigma;  /* velocity: sigma of the unknown velocity at (re-)initialisation, metres per frame (0.05); > 0 */
  float gate;              /* as kfn_pose_filter */
  int32_t max_rejects;     /* as kfn_pose_filter */
} kfn_pose_track_desc;
#define KFN_POSE_TRACK_DESC_INIT {(int32_t)sizeof(kfn_pose_track_desc), 0, 0, KFN_POSE_MODEL_WALK, 0, 0.02f, 0.02f, 0.05f, 0.05f, 22.46f, 3}
int kfn_pose_track_state_bytes(const kfn_pose_track_desc* desc, size_t* bytes);
int kfn_pose_track_scratch_bytes(const kfn_pose_track_desc* desc, size_t* bytes);
int kfn_pose_track(const kfn_pose_track_desc* desc, const float* poses, const float* cov, void* state, float* out_poses,
                   float* out_cov, int32_t* flags, float* nis, float* smooth_poses, float* smooth_cov, void* scratch,
                   void* stream);

/* ---- multi-GPU: rank -> rank hand-off of the recurrent state (RCCL point-to-point) ----
 * No reference counterpart (the reference is single-device: KFNet/train.py:375 is its only
 * device placement).  BASELINE config 4 / SURVEY.md §8(e): a T-frame sequence is cut into
 * contiguous chunks, one per rank = GPU; everything but the scan depends on images only, so
 * the one exchange is the [H,W,4] fp32 state (what KFNet/eval.py:103-104 feeds back through
 * SetVariableByName) from the rank that finished chunk r to the rank that owns chunk r+1.
 * ncclSend / ncclRecv on `stream`, i.e. ordered behind/before the kfn_kalman_scan launches
 * on that stream; no host synchronisation.  librccl is bound at run time (dlopen).
 *   kfn_comm_available  local probe: run it on every rank BEFORE the collective kfn_comm_init, so that a rank
 *                       without RCCL is found while the others can still be told;
 *   kfn_comm_unique_id  rank 0 creates the 128-byte id and distributes it out of band
 *                       (torch.distributed / MPI / a file);
 *   kfn_comm_init       collective over all ranks; binds `device` to the calling thread;
 *   kfn_send_state /    count = H*W*4 floats; a send must be matched by the peer's recv of
 *   kfn_recv_state      the same size (kfnet_amd/dist.py pairs them by the reset rule: a
 *                       chunk that starts on a reset frame receives nothing). */
#define KFN_COMM_ID_BYTES 128
typedef struct kfn_comm kfn_comm;
int kfn_comm_available(void);   /* KFN_OK if librccl can be bound in this process (no communicator, no socket, no device) */
int kfn_comm_unique_id(void* id, size_t bytes /* == KFN_COMM_ID_BYTES */);
int kfn_comm_init(kfn_comm** comm, int rank, int nranks, const void* unique_id, int device);
int kfn_comm_destroy(kfn_comm* comm);
int kfn_comm_rank(const kfn_comm* comm, int* rank, int* nranks);
int kfn_send_state(kfn_comm* comm, int peer, const float* state /* [H,W,4] */, int H, int W, void* stream);
int kfn_recv_state(kfn_comm* comm, int peer, float* state /* [H,W,4] */, int H, int W, void* stream);

/* ---- training SCoordNet (added exports; the ABI number stays 12) ---------------------------------------------------
 * Stage 1 of the reference's procedure, "Train SCoordNet": tf.train.AdamOptimizer(lr).minimize(loss + reg_loss)
 * (KFNet/train.py:300-315) over the ScoreNet variables.  TensorFlow derives the backward graph; here it is the entry points
 * below plus the EXISTING forward kernels: the input gradient of a stride-1 convolution is kfn_conv2d_nhwc on the kernel
 * rotated by 180 degrees with its channel axes swapped, that of a stride-2 convolution of an even-sized image is the
 * transposed convolution (kfn_conv_desc.transposed = 1) with the kernel as it is.  fp32 here; fp16 operands: the section
 * "mixed-precision training" below.  DESIGN.md "Training".
 *
 * kfn_conv2d_grad_weights -- the gradient of tf.layers.conv2d (cnn_wrapper/network.py:116-135) with respect to its kernel
 * and bias.  `desc` is the FORWARD convolution's descriptor (N, H, W, Cin, ldx of its input x; Cout; kh = kw = 3 or 1;
 * stride 1 or 2; transposed = 0; fp32); desc.ldy is the pixel stride of dz, the gradient with respect to the convolution's
 * output BEFORE its ReLU, [N,Ho,Wo,Cout].  Cin % 16 == 0, any Cout >= 1.
 *   dw[kh][kw][ci][co] = sum_{n,y,x} x[n, y*s + kh - pad_t, x*s + kw - pad_l, ci] * dz[n, y, x, co]   (TF HWIO, dense)
 *   db[co]             = sum_{n,y,x} dz[n, y, x, co]                                                   (db may be NULL)
 * An implicit GEMM on v_mfma_f32_32x32x2_f32 whose reduction runs over the pixels, cut into runs of pixels whose partial
 * results go to planes of `workspace` (kfn_conv2d_grad_weights_workspace_bytes) and are added in a fixed order by a second
 * launch: no atomics, bit-identical from launch to launch, and the split depends on the shapes only. */
int kfn_conv2d_grad_weights_workspace_bytes(const kfn_conv_desc* desc, size_t* bytes);
/* What kfn_conv2d_grad_weights will launch for `desc` (cf. kfn_kalman_scan_plan); the launcher and the workspace size are
 * decided by the same function, every refusal of the launcher that the descriptor alone decides is returned here too.  No
 * device access.
 *   tn       1 (Cout <= 64: workgroup tiles of 128 k x 64 co) or 2 (128 x 128)
 *   tiles_m  ceil((kh*kw*Cin + 1) / 128), the + 1 being the bias row;  tiles_n  ceil(Cout / (64 tn))
 *   splits   runs of pixels = planes of the workspace;  chunk  pixels per run, a multiple of the stage (16 pixels with fp32
 *            operands, 32 with KFN_OPERAND_F16); the last run holds N*Ho*Wo - (splits - 1) * chunk pixels
 * workspace bytes = splits * (kh*kw*Cin + 1) * Cout * 4. */
int kfn_conv2d_grad_weights_plan(const kfn_conv_desc* desc, int* tn, int* tiles_m, int* tiles_n, int* splits, long* chunk);
int kfn_conv2d_grad_weights(const kfn_conv_desc* desc, const float* x, const float* dz, float* dw, float* db,
                            float* workspace, void* stream);
/* The same for SCoordNet.preprocess + conv1a (cnn_wrapper/SCoordNet.py:20-21,34-37) as kfn_first_conv_u8 evaluates them:
 * img [N,H,W,3] uint8, dz [N,H,W,C1] dense, dw [27][C1] (HWIO flattened), db [C1] or NULL.  C1 = 16, 32, 48 or 64.  The
 * layer has no input gradient. */
int kfn_first_conv_u8_grad_weights_workspace_bytes(int N, int H, int W, int C1, size_t* bytes);
int kfn_first_conv_u8_grad_weights(const uint8_t* img, int N, int H, int W, const float* dz, int C1, float* dw, float* db,
                                   float* workspace, void* stream);
/* Gradient of tf.nn.relu (cnn_wrapper/network.py:133), in place: dz[p][c] = y[p][c] > 0 ? dz[p][c] : 0 for P pixels of C
 * channels with pixel strides ldy / ldz. */
int kfn_relu_grad(const float* y, int ldy, float* dz, int ldz, long P, int C, void* stream);
/* The weight matrices of a layer's launches from its TF HWIO master copy [kh][kw][Cin][Cout], on the device (what
 * kfnet_amd.graph.pack_conv_kernel does on the host once; in training the weights change every step):
 *   KFN_PACK_FORWARD        [cout_pad][kh*kw*Cin]            w_packed of kfn_conv2d_nhwc for the layer itself
 *   KFN_PACK_INPUT_GRAD_S1  [cin_pad][kh*kw*cout16]          ... for its input gradient as a stride-1 convolution of dz
 *                                                            [.., cout16] -> [.., Cin]: row ci, column (a, b, co) =
 *                                                            w[kh-1-a][kw-1-b][ci][co]
 *   KFN_PACK_INPUT_GRAD_S2  [cin_pad][kh*kw*cout16]          ... as the transposed convolution: w[a][b][ci][co]
 * cout_pad / cin_pad = the count rounded up to a multiple of 32 (zero rows), cout16 = Cout rounded up to a multiple of
 * 16 (zero columns: 'prediction' has 4 output channels, its dz lives in a 16-channel buffer whose other channels are 0).
 * conv1a's forward matrix [27][C1] is the master copy itself.  kfn_pack_conv_weights_floats: the size of `out`.
 * KFN_PACK_INPUT_GRAD_S1 takes odd kh and kw only (KFN_ERR_ARG otherwise, from all three entry points): SAME padding of an
 * even kernel puts (k - 1) / 2 pixels in front and one more behind, the convolution with the rotated kernel would need the
 * larger share in front, so kfn_conv2d_nhwc on such a pack would return the input gradient shifted by one pixel. */
#define KFN_PACK_FORWARD 0
#define KFN_PACK_INPUT_GRAD_S1 1
#define KFN_PACK_INPUT_GRAD_S2 2
int kfn_pack_conv_weights_floats(int kh, int kw, int Cin, int Cout, int kind, size_t* floats);
int kfn_pack_conv_weights(const float* w_hwio, int kh, int kw, int Cin, int Cout, int kind, float* out, void* stream);

/* kfn_coord_loss_grad -- KFNet.MeasureCoordLoss restricted to the measurement term (KFNet/KFNet.py:234-254): the NLL of
 * CoordLossWithUncertainty (:192-232) plus smooth_weight * SmoothLoss (:430-467), on the labels as KFNet/train.py:274-280
 * prepares them, and the gradient with respect to the network's raw output.
 *   pred    [B,h,w,ld_pred]  'prediction' before GetOutput's exp: (x, y, z, log sigma)
 *   labels  [B,h*label_stride,w*label_stride,4] = (gt xyz, mask); cell (r, c) reads pixel (label_stride*r, label_stride*c)
 *           (tf.image.resize_nearest_neighbor); mask = (mask == 1); gt = transform [gt; 1] when has_transform
 *   img     [B,h*img_stride,w*img_stride,3] uint8, read the same way (the smoothness weights); NULL iff smooth_weight == 0
 *   sigma = exp(ch3), u = max(sigma, min_uncertainty), d = sum_c (x_c - gt_c)^2, l = 3 log u + d / (2 u^2),
 *   l = min(l, loss_clip) when has_loss_clip (KFNet.py:217 clips at -2.0), valid = sum(mask) + 1
 *   stats[8] = (L_nll = sum(mask l) / valid, L_smooth, accuracy = (valid - #{mask d > dist_threshold^2}) / valid, valid,
 *               L = L_nll + smooth_weight L_smooth, 0, 0, 0)
 *   dpred   [B,h,w,ld_dpred]: channels 0..3 = dL/dpred (through exp and the max gate; 0 where the clip is active); the
 *           other channels of a wider buffer are not written.
 * One workgroup; per-pixel terms in unfused fp32, their sums in fp64 over a fixed tree. */
typedef struct kfn_coord_loss_desc {
  int32_t struct_size;      /* = sizeof(kfn_coord_loss_desc) */
  int32_t B, h, w;
  int32_t ld_pred, ld_dpred;
  int32_t label_stride, img_stride;
  int32_t has_transform;
  float transform[12];      /* first 3 rows of transform.txt, row-major */
  int32_t has_loss_clip;
  float loss_clip;
  float smooth_weight;      /* 50 */
  double dist_threshold;    /* 0.05, the Python double: compared as float(dist_threshold * dist_threshold), one rounding */
  double min_uncertainty;   /* 1e-5: u = max(sigma, float(min_uncertainty)) */
} kfn_coord_loss_desc;
int kfn_coord_loss_grad(const kfn_coord_loss_desc* desc, const float* pred, const float* labels, const uint8_t* img,
                        float* dpred, float* stats, void* stream);

/* kfn_adam_step -- tf.train.AdamOptimizer's update of one variable (or one flat buffer) of n floats, the caller passing
 * lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t), t counting from 1:
 *   g' = g + weight_decay * w  (the gradient of l2_regularizer(weight_decay), KFNet/train.py:301-303)
 *   m <- beta1 m + (1 - beta1) g',  v <- beta2 v + (1 - beta2) g'^2,  w <- w - lr_t m / (sqrt(v) + epsilon)
 * evaluated in fp64 from the fp32 variables, each stored value rounded once. */
int kfn_adam_step(float* w, float* m, float* v, const float* g, long n, double lr_t, double beta1, double beta2,
                  double epsilon, double weight_decay, void* stream);

/* ---- mixed-precision training of SCoordNet (added exports; the ABI number stays 13) ----------------------------------
 * Tensors, master weights and Adam's slots stay fp32 in memory; the convolutions' operands are rounded to IEEE halfs (RNE)
 * while they are staged and multiplied on v_mfma_f32_32x32x16_f16 with fp32 accumulation.  Forward passes and input
 * gradients are kfn_conv2d_nhwc with operand_dtype = KFN_OPERAND_F16 and half packs.  DESIGN.md 6h.
 *
 * kfn_conv2d_grad_weights with desc.operand_dtype = KFN_OPERAND_F16: the contract above (x, dz, dw, db, workspace fp32;
 * runs of pixels fixed by the shapes; planes added in ascending order; no atomics; bit-identical launches), the products
 * being those of x and dz rounded to halfs.  Needs Cin % 32 == 0, Cout % 32 == 0, desc.ldy % 4 == 0 and a 16-byte aligned
 * dz: KFN_ERR_ARG otherwise, and nothing launched.  kfn_conv2d_grad_weights_workspace_bytes follows operand_dtype:
 * a run is a multiple of 32 pixels instead of 16.
 *
 * kfn_pack_conv_weights_f16 -- kfn_pack_conv_weights with every value rounded once (RNE) to an IEEE half: the layout of
 * the fp32 pack, kfn_pack_conv_weights_floats elements of 2 bytes, what kfnet_amd.graph.as_f16(pack_conv_kernel) makes on
 * the host and kfn_conv2d_nhwc reads under KFN_OPERAND_F16. */
int kfn_pack_conv_weights_f16(const float* w_hwio, int kh, int kw, int Cin, int Cout, int kind, void* out_halfs, void* stream);

/* Dynamic loss scaling without a read-back.  One record in DEVICE memory, written by the host once (scale a power of two,
 * both powers 1.0, every counter 0) and from then on by the launches below:
 *   kfn_loss_scale_apply          buf[i] *= scale (the gradient of the loss with respect to the prediction, after
 *                                 kfn_coord_loss_grad); exact, the scale being a power of two
 *   kfn_loss_scale_unscale_check  grads[i] *= 1 / scale; overflow |= 1 if any element was inf or NaN (an integer OR)
 *   kfn_adam_step_guarded         kfn_adam_step's arithmetic when overflow == 0, with lr_t = lr sqrt(1 - beta2_power beta2) /
 *                                 (1 - beta1_power beta1) from the record (fp64); w, m, v untouched otherwise.  Then one
 *                                 thread of a second launch: on overflow scale = max(scale / 2, 1), good_steps = 0,
 *                                 skipped += 1, overflow = 0; otherwise beta1_power *= beta1, beta2_power *= beta2,
 *                                 adam_t += 1, good_steps += 1, and after growth_interval such steps scale = min(2 scale,
 *                                 2^24), good_steps = 0.
 * The powers are products accumulated once per APPLIED step, as TensorFlow's beta1_power / beta2_power variables. */
typedef struct kfn_loss_scale_state {
  double beta1_power, beta2_power;
  float scale;
  int32_t good_steps;       /* applied steps since the scale last changed */
  int32_t overflow;         /* raised by kfn_loss_scale_unscale_check, cleared by kfn_adam_step_guarded */
  int32_t skipped;          /* steps dropped because of an overflow */
  int32_t adam_t;           /* applied steps */
  int32_t reserved;         /* 0 */
} kfn_loss_scale_state;
int kfn_loss_scale_apply(float* buf, long n, const kfn_loss_scale_state* state, void* stream);
int kfn_loss_scale_unscale_check(float* grads, long n, kfn_loss_scale_state* state, void* stream);
int kfn_adam_step_guarded(float* w, float* m, float* v, const float* g, long n, double lr, double beta1, double beta2,
                          double epsilon, double weight_decay, int growth_interval, kfn_loss_scale_state* state, void* stream);

/* ---- augmenting a training batch (added exports; the ABI number stays 13) --------------------------------------------
 * data_augmentation of the reference (KFNet/train.py:168-193): tf.image.random_brightness / random_contrast on the frames,
 * then frames and labels together through image_augmentation (KFNet/util.py:66-136) -- an in-plane rotation
 * (tf.contrib.image.rotate, NEAREST, fill 0) followed by a zoom into a box (tf.image.crop_and_resize) or by a shrink with
 * zero padding (tf.image.resize_images + resize_image_with_crop_or_pad) -- with ONE parameter set per batch.  DESIGN.md 6c
 * lists every operation; the device evaluates exactly that list in unfused fp32, so all derived constants arrive here as
 * floats the host has rounded once (kfnet_amd.augment.descriptor).  crop_size == image_size only.
 *
 * kfn_frame_channel_sums -- sums [B][4] uint32 = the exact sum of each channel of each frame of img [B,H,W,3] uint8, the
 * fourth word 0 (adjust_contrast's per-channel mean, times H W).  Integer adds: bit-identical from launch to launch.  H and
 * W multiples of 8, img 16-byte aligned. */
int kfn_frame_channel_sums(const uint8_t* img, int B, int H, int W, uint32_t* sums, void* stream);
/* kfn_augment_batch -- frames_out [B,H,W,3] uint8 and, unless labels_in and labels_out are both NULL, labels_out
 * [B,H/label_stride,W/label_stride,4] = the augmented (xyz, mask) at output pixels (label_stride r, label_stride c) from the
 * full-resolution labels_in [B,H,W,4]; label_stride 1 or 8 (the loss reads pixel (8r, 8c)).
 *   mode 0 (translate): the identity map, no rotation.  mode 1 (enlarge): in_y = y0 + i dy, 0 outside [0, H-1], taps floor /
 *   ceil.  mode 2 (shrink): ii = i - off_y, 0 unless 0 <= ii < new_h, in_y = ii scale_y, taps t = floor, min(t + 1, H - 1).
 *   value = top + (bot - top) ly with top = tl + (tr - tl) lx, bot alike; each tap is pixel (x, y) of the ROTATED image =
 *   source pixel (round(sx), round(sy)), sx = (rot0 x + rot1 y) + rot2, sy = (rot3 x + rot4 y) + rot5, round half away from
 *   zero, 0 outside the image (has_rotation == 0: the pixel itself).
 *   frames: a tap is ((p + delta) - mean) factor + mean with mean = float(sum / (H W) + delta) per frame and channel when
 *   has_colour (the fill value 0 is not adjusted), the result clamp(rint(value), 0, 255) (ties to even).
 *   labels: the four channels interpolated, then mask = value >= 1 ? 1 : 0 (KFNet/train.py:189).
 * With has_colour the call runs kfn_frame_channel_sums into `sums` [B][4] first, on the same stream; sums may be NULL
 * otherwise.  H, W >= 8 and multiples of 8.  KFN_ERR_ARG, and nothing launched: other sizes, a stride other than 1 or 8,
 * frames_out == frames_in (the gather cannot run in place), NULL where a buffer is needed, one label pointer without the
 * other, a struct_size other than sizeof(kfn_augment_desc). */
typedef struct kfn_augment_desc {
  int32_t struct_size;      /* = sizeof(kfn_augment_desc) */
  int32_t B, H, W;
  int32_t label_stride;
  int32_t mode;             /* 0 translate, 1 enlarge, 2 shrink */
  int32_t has_rotation, has_colour;
  float rot[6];             /* cos a, -sin a, xo, sin a, cos a, yo */
  float y0, dy, x0, dx;     /* enlarge: y1 (H - 1), ratio, x1 (W - 1), ratio */
  int32_t new_h, new_w, off_y, off_x;   /* shrink */
  float scale_y, scale_x;   /* H / new_h, W / new_w */
  float delta, factor;      /* brightness delta, contrast factor */
} kfn_augment_desc;
int kfn_augment_batch(const kfn_augment_desc* desc, const uint8_t* frames_in, const float* labels_in, uint8_t* frames_out,
                      float* labels_out, uint32_t* sums, void* stream);
/* kfn_augment_pixel_map -- channels 7-8 of the reference's 9-channel bundle (KFNet/train.py:181-187): the normalised pixel
 * map of get_pixel_map (:150-166) carried through the same rotation and zoom, out [H/label_stride,W/label_stride,2] at output
 * pixels (label_stride r, label_stride c).  One parameter set serves the batch, so one map serves every frame (desc->B is
 * only checked).  It is the label path above with the gathered value replaced by the analytic one: a tap at source pixel
 * (sx, sy) has the value ((float(sx) - u) inv_fx, (float(sy) - v) inv_fy), a tap outside the image (0, 0); the same three-step
 * interpolation in the same order; mode 0 gives the plain map.  inv_fx = float(1 / fx), rounded once by the host.  out 8-byte
 * aligned.  KFN_ERR_ARG, and nothing launched: kfn_augment_batch's conditions on the descriptor, a NULL buffer. */
int kfn_augment_pixel_map(const kfn_augment_desc* desc, float u, float v, float inv_fx, float inv_fy, float* out, void* stream);

/* ---- the reprojection loss (added export; the ABI number stays 13) --------------------------------------------------------
 * KFNet.ReprojectionLoss (KFNet/KFNet.py:405-428) in its masked form, which the reference adds to the three terms of its
 * loss: 50 R in MeasureCoordLoss (:246-248), 10 R in TemporalCoordLoss (:270-272), 10 R in KFCoordLoss (:292-294).  DESIGN.md
 * 6i.  For cell (r, c) of frame b and a prediction x (channels 0..2 of out[o].x):
 *   cam = M_b [x; 1], M [B,12] = the first three rows of P_b G^-1 (P_b: world to camera of frame b, G: the 4x4 by which the
 *         loss launches map the labels), formed by the host in fp64 and rounded once
 *   q   = (pixel_map[r][c][0], pixel_map[r][c][1], 1), or ((float(8 c) - u) inv_fx, (float(8 r) - v) inv_fy, 1) when pixel_map
 *         is NULL
 *   n(a) = a / sqrt(max(sum a^2, 1e-12)) (tf.nn.l2_normalize), e = n(cam) - n(q), rho = sum_c e_c^2
 *   m   = (labels[b][label_stride r][label_stride c][3] == 1), labels [B,h label_stride,w label_stride,4]
 *   R   = sum(m rho) / (valid + 1), valid = nll_stats[valid_index] = sum(m) + 1 as kfn_coord_loss_grad (word 3) and
 *         kfn_filter_loss_grad (word 10) report it: the reference divides by valid_pixel + 1 where valid_pixel already
 *         carries a + 1 (:422, :427), and so does this launch.  The unmasked form (mask = None) is not built.
 *   d(rho)/d(cam) = (2 / sqrt(s)) (n(cam) (n(cam) . n(q)) - n(q)) with s = sum cam^2 above the floor, 2e6 e at or below it;
 *   out[o].dx[..][0..2] += out[o].weight m M_b[:, :3]^T d(rho)/d(cam) / (valid + 1).  Channel 3 and any padding channel keep
 *   their bits, and so does every channel of a cell with m = 0.
 *   stats_out[8] = (R of out[0], out[1], out[2] (0 for an absent one), sum_o weight_o R_o, valid + 1, 0, 0, 0)
 * The launch ADDS, so it goes behind kfn_coord_loss_grad / kfn_filter_loss_grad on the same stream and in front of
 * kfn_loss_scale_apply / kfn_filter_backward*.  One workgroup; per-cell terms in unfused fp32, the sums in fp64 over a fixed
 * tree, no atomics: two launches give the same bits.  x and dx with ld % 4 == 0 and a 16-byte aligned base move as 16-byte
 * words.  KFN_ERR_ARG, and nothing launched: a wrong struct_size, outputs outside 1..3, a NULL required buffer (pixel_map may
 * be NULL), ld_x < 3 or ld_dx < 3, a label stride other than 1 or 8, a non-positive size or B h w >= 2^24, M not 16-byte
 * aligned. */
#define KFN_REPROJ_MAX_OUTPUTS 3
typedef struct kfn_reproj_output {
  const float* x;           /* [B,h,w,ld_x] */
  float* dx;                /* [B,h,w,ld_dx] */
  float weight;             /* multiplies dR/dx and R in stats_out[3] */
  int32_t ld_x, ld_dx;      /* floats per cell, >= 3 */
  int32_t reserved;         /* 0 */
} kfn_reproj_output;
typedef struct kfn_reproj_desc {
  int32_t struct_size;      /* = sizeof(kfn_reproj_desc) */
  int32_t B, h, w;
  int32_t label_stride;     /* 1 or 8 */
  int32_t outputs;          /* 1..3 */
  float u, v;               /* principal point */
  float inv_fx, inv_fy;     /* float(1 / fx), float(1 / fy) */
  kfn_reproj_output out[KFN_REPROJ_MAX_OUTPUTS];
} kfn_reproj_desc;
int kfn_reproj_loss_grad(const kfn_reproj_desc* desc, const float* M, const float* labels, const float* pixel_map,
                         const float* nll_stats, int valid_index, float* stats_out, void* stream);

/* ---- training labels from depth maps and poses (added exports; the ABI number stays 13) -----------------------------
 * A label is a function of a depth map and a camera-to-world pose.  The device evaluates the list below in
 * unfused fp32, without division or transcendental: every derived constant arrives as a float the host has rounded once
 * (kfnet_amd.labels.DepthCamera.descriptor).
 *
 * kfn_depth_labels -- depth [B,H,W] uint16 and poses [B][12] float (the rows of [R|t], camera to world) -> labels_out
 * [B,H/stride,W/stride,ld_out] float; the columns beyond 3 are not written.  Output pixel (r, c) is colour pixel
 * x = stride c, y = stride r (the pixel the loss reads; the PnP stage's cell (r, c) observes pixel (8c, 8r)).
 *   depth pixel: (x, y) when registration == 0; else xd = q((float(x) - u) kx + ud), yd = q((float(y) - v) ky + vd), q =
 *   round half away from zero, kx = float(fx_depth / fx): a gather; a pixel that leaves the depth image is invalid.
 *   raw = depth[b][yd][xd]; valid iff raw_min <= raw <= raw_max (1 and 65534 exclude 7-Scenes' 0 and 65535).
 *   z = float(raw) scale; X = ((float(x) - u) inv_fx) z; Y = ((float(y) - v) inv_fy) z   (depth is z, not ray length)
 *   w_i = ((P[i][0] X + P[i][1] Y) + P[i][2] z) + P[i][3], i = 0..2
 *   output (w_0, w_1, w_2, 1) where valid, (0, 0, 0, 0) otherwise.
 * At stride 1 a thread owns 8 adjacent pixels (one 16-byte depth load without registration, eight 16-byte stores when
 * ld_out is a multiple of 4); at stride 8 there is one thread per output pixel.  depth 16-byte aligned.  KFN_ERR_ARG, and
 * nothing launched: a struct_size other than sizeof(kfn_depth_labels_desc), a stride other than 1 or 8, H or W not a
 * multiple of 8 (or below 8), a NULL buffer, ld_out < 4, an empty validity window. */
typedef struct kfn_depth_labels_desc {
  int32_t struct_size;      /* = sizeof(kfn_depth_labels_desc) */
  int32_t B, H, W;
  int32_t stride;           /* 1 or 8 */
  int32_t ld_out;           /* floats per output pixel, >= 4 */
  int32_t registration;     /* 0: the depth pixel is the colour pixel */
  int32_t raw_min, raw_max; /* 1, 65534 */
  float u, v;               /* principal point of the colour camera */
  float inv_fx, inv_fy;     /* float(1 / fx), float(1 / fy) */
  float kx, ky;             /* float(fx_depth / fx), float(fy_depth / fy) */
  float ud, vd;             /* principal point of the depth camera */
  float scale;              /* float(0.001): millimetres to metres */
} kfn_depth_labels_desc;
int kfn_depth_labels(const kfn_depth_labels_desc* desc, const uint16_t* depth, const float* poses, float* labels_out,
                     void* stream);

/* kfn_label_moments -- partial [B][10] double: per frame of labels [B,h,w,ld] float, over the pixels whose mask (column
 * 3) == 1, with d = double(p) - pivot: n, sum d (x, y, z), and sum d d^T (xx, xy, xz, yy, yz, zz).  The host adds the
 * frames in index order and derives transform.txt (kfnet_amd.labels.decorrelating_transform); a pivot near the points
 * (the first frame's camera centre) keeps the second moments free of cancellation.  One workgroup per frame, a fixed
 * walk and a fixed LDS tree, no atomics: bit-identical from launch to launch.  A frame without a valid pixel gives ten
 * zeros.  KFN_ERR_ARG, and nothing launched: a wrong struct_size, a non-positive size, ld < 4, a NULL buffer. */
typedef struct kfn_label_moments_desc {
  int32_t struct_size;      /* = sizeof(kfn_label_moments_desc) */
  int32_t B, h, w;
  int32_t ld;               /* floats per label pixel, >= 4 */
  int32_t reserved;         /* 0 */
  double pivot[3];
} kfn_label_moments_desc;
int kfn_label_moments(const kfn_label_moments_desc* desc, const float* labels, double* partial, void* stream);

/* ---- labels, depth maps and frames rendered from a triangle mesh (added exports; the ABI number stays 13) -------------
 * A scene that ships a model: vertices [V,3] float (world frame), colors [V,3] uint8 or NULL (white), triangles [N,3]
 * int32, poses [B][12] float (the rows of [R|t], camera to world, as for kfn_depth_labels) -> at the samples (r, c) =
 * image pixel (stride c, stride r) of a H x W pinhole camera, each output optional (NULL):
 *   labels [B,H/stride,W/stride,ld_labels] float  (world x, y, z, mask); the columns beyond 3 are not written
 *   depth  [B,H/stride,W/stride] uint16           raw units of `scale` metres, 0 where invalid
 *   frames [B,H/stride,W/stride,3] uint8          the vertex colours, interpolated
 *   stats  [B,5] int32                            covered samples, triangles that passed culling, triangles clipped at the
 *                                                 near plane, 1 if the pose was non-finite, triangles skipped for an index
 *                                                 outside [0, V)
 * zbuf (required, kfn_render_scratch_bytes bytes, 8-byte aligned) holds one key per sample afterwards: all ones where no
 * triangle covers it, else bits(z) << 32 | triangle index of the nearest triangle, the lower index among equal depths.
 * The fp32 operations, in order (kfnet_amd/csrc/kfn_render.hip repeats them, tests/render_ref.py restates
 * them in numpy float32 and gets the same bits); every quotient is an IEEE division:
 *   transform  vertex p to the camera frame by the inverse of the pose as R^T (p - t): d = p - t, X = (P[0] d.x + P[4] d.y)
 *              + P[8] d.z, Y = (P[1] d.x + P[5] d.y) + P[9] d.z, Z = (P[2] d.x + P[6] d.y) + P[10] d.z.
 *   cull/clip  a triangle with a non-finite camera coordinate or all three Z < near is culled; one crossing Z = near is
 *              clipped to a polygon of 3 or 4 vertices (crossing of the inside vertex I and the outside O at tt = (I.z - near)
 *              / (I.z - O.z): I + tt (O - I), z = near); vertices project to sx = (x / z) fx + u, sy = (y / z) fy + v.
 *   depth      1/z = pa x' + pb y' + pc with n = (c1 - c0) x (c2 - c0), d = n . c0, (pa, pb, pc) = n / d: the plane of the
 *              UNCLIPPED triangle; at a sample w = (pa rx + pb ry) + pc with the ray rx = (px - u) inv_fx, ry = (py - v)
 *              inv_fy; w > 0; z = 1 / w.
 *   coverage   the polygon's edges, each taken in a canonical direction (from the endpoint with the lower sx, then sy), so
 *              two triangles sharing an edge evaluate the same numbers: e = ex (py - A.y) - ey (px - A.x), signed so that the
 *              polygon's next vertex is on the positive side; covered iff every edge has e > 0, or e == 0 on a left or top
 *              edge (the top-left rule: a sample on a shared edge is covered exactly once).  Both windings are rendered.
 *   visibility 64-bit integer atomic min of the key; nothing depends on the order of arrival.
 *   resolve    hit = z (rx, ry, 1); q = rint(z / scale), ties to even; raw_min <= q <= raw_max: depth q, label (R hit + t, 1)
 *              evaluated as kfn_depth_labels evaluates it; else depth 0 and label (0, 0, 0, 0).  Colour: barycentric
 *              coordinates of the hit point in the original triangle, in 3-D in the camera frame; rint, clamped to 0..255.
 * A frame whose pose has a non-finite entry gives all-zero outputs, all-ones keys and stats[b][3] = 1.  Three launches on
 * `stream` (clear, rasterise, resolve), no allocation and no synchronisation.  KFN_ERR_ARG, and nothing launched: a wrong
 * struct_size, a NULL vertices, triangles, poses or zbuf, a stride other than 1 or 8, H or W not a multiple of the stride,
 * a non-positive size, B > 65535, B (H/stride) (W/stride) >= 2^31, ld_labels < 4, near <= 0, scale <= 0, a validity window
 * outside 0..65535. */
typedef struct kfn_render_desc {
  int32_t struct_size;      /* = sizeof(kfn_render_desc) */
  int32_t B, V, N;          /* frames, vertices, triangles */
  int32_t H, W;             /* the image */
  int32_t stride;           /* 1 or 8 */
  int32_t ld_labels;        /* floats per label, >= 4 */
  int32_t raw_min, raw_max; /* the depth PNG's validity window: 1, 65534 */
  float u, v;               /* principal point */
  float inv_fx, inv_fy;     /* float(1 / fx), float(1 / fy) */
  float fx, fy;
  float near;               /* metres, > 0: 0.05 */
  float scale;              /* metres per raw unit: float(0.001) */
} kfn_render_desc;
int kfn_render_scratch_bytes(const kfn_render_desc* desc, size_t* bytes);
int kfn_render(const kfn_render_desc* desc, const float* vertices, const uint8_t* colors, const int32_t* triangles,
               const float* poses, void* zbuf, float* labels, uint16_t* depth, uint8_t* frames, int32_t* stats, void* stream);

/* ---- depth maps fused into a TSDF volume, and the scene mesh extracted from it (added exports; the ABI number stays 13) ---
 * What makes the model kfn_render draws.  The volume: lattice points (ix, iy, iz), 0 <= i < n, x fastest;
 * tsdf [nz][ny][nx] pairs of float (D, W); color, optional, [nz][ny][nx] quadruples of float (r, g, b, wc).  All zeros is the
 * empty volume.  The world position of a lattice point is p = (ox + float(ix) voxel, oy + float(iy) voxel, oz + float(iz)
 * voxel): one product and one sum per component.  Every operation below is one rounded fp32 operation, every quotient an IEEE
 * division (kfnet_amd/csrc/kfn_fuse.hip repeats them, tests/fuse_ref.py restates them in numpy float32 and gets the same bits).
 *
 * kfn_fuse_integrate: depth [B,H,W] uint16, frames [B,H,W,3] uint8 (NULL iff color is NULL), poses [B][12] float, the rows of
 * [R|t] camera to world.  For each voxel the frames b = 0 .. B-1 are applied in this order:
 *   1  a non-finite entry in poses[b] skips the frame.
 *   2  d = p - t: dx = p.x - P[3], dy = p.y - P[7], dz = p.z - P[11];  X = (P[0] dx + P[4] dy) + P[8] dz, Y = (P[1] dx + P[5] dy)
 *      + P[9] dz, Z = (P[2] dx + P[6] dy) + P[10] dz  (kfn_render's transform).
 *   3  Z < near or a non-finite coordinate: skip.
 *   4  the DEPTH camera: sx = (X / Z) dfx + du, sy = (Y / Z) dfy + dv, cf = rint(sx), rf = rint(sy), ties to even; skip unless
 *      0 <= cf <= W-1 and 0 <= rf <= H-1, compared in float before converting.
 *   5  raw = depth[b][r][c]; skip if it lies outside [raw_min, raw_max];  dm = float(raw) scale.
 *   6  s = dm - Z (the z-distance, not the ray length);  skip if s < -trunc (behind the surface);  f = min(s / trunc, 1).
 *   7  D = (W D + f) / (W + 1);  then W = min(W + 1, max_weight).
 *   8  colour, when color is given and s <= trunc: the COLOUR camera, cx = rint((X / Z) fx + u), cy = rint((Y / Z) fy + v); if
 *      that pixel lies inside the image, each channel ch = (wc ch + float(pixel)) / (wc + 1), then wc = min(wc + 1, max_weight).
 * One launch: a thread keeps its voxel in registers across the B frames, so the volume crosses memory once a call; a voxel
 * that no frame touched is not written.
 *
 * kfn_fuse_extract_count and kfn_fuse_extract: marching tetrahedra on the lattice.
 *   validity   a lattice point is valid iff W >= min_weight, inside iff it is valid and D < 0.
 *   cubes      the cube at (ix, iy, iz), i < n - 1, is cut into six tetrahedra {v, v + e_a, v + e_a + e_b, v + (1,1,1)}, one per
 *              permutation (a, b, c) of the axes in the order xyz, xzy, yxz, yzx, zxy, zyx; neighbouring cubes agree on every
 *              face diagonal.  A tetrahedron is emitted only if all four corners are valid.
 *   vertices   lattice point v owns the seven edges to v + (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1), in this
 *              order.  An owned edge carries a vertex iff its far end is in the grid, both ends are valid and exactly one is
 *              inside.  id = (the vertex counts of all lattice points with a lower linear index) + (rank among v's carrying
 *              edges).  With a the owner end and b the far end: t = Da / (Da - Db), pos = pa + t (pb - pa) per component;
 *              colour min(max(rint(ca + t (cb - ca)), 0), 255) per channel when color is given and both ends have wc > 0,
 *              otherwise 255.  A vertex that no emitted tetrahedron uses may exist (a neighbour can be invalid).
 *   triangles  with m inside corners a tetrahedron emits one triangle for m = 1 or 3, two for m = 2 (the quad split on a fixed
 *              diagonal), none for 0 or 4, wound so that (v1 - v0) x (v2 - v0) points from inside to outside.  index = (the
 *              triangle counts of all cubes with a lower linear index) + (position within the cube: tetrahedra 0..5, table
 *              order within one).  Zero-area triangles (D == 0 at a corner) are kept.
 * kfn_fuse_extract_count writes per-point and per-cube counts and their exclusive scans into scratch (kfn_fuse_scratch_bytes
 * bytes, 8-byte aligned) and the two 64-bit totals (vertices, triangles) into totals[2] on the device.  The scan is plain
 * launches (block sums, a scan of the block sums, an add): no workgroup waits for another.  kfn_fuse_extract then writes
 * vertices [V,3] float, colors [V,3] uint8 (optional) and triangles [N,3] int32 and nothing at or past the capacities it
 * is given; the host reads the totals between the two calls and refuses totals of 2^31 or more.  Everything runs on
 * `stream` with no allocation and no synchronisation.  KFN_ERR_ARG, and nothing launched: a wrong struct_size, a NULL tsdf,
 * depth or poses (scratch, totals, vertices, triangles), frames and color not both NULL or both given, a non-positive
 * dimension, nx ny nz >= 2^31, B > 65535, voxel <= 0, trunc <= 0, near <= 0, scale <= 0, max_weight < 1, min_weight < 1 (the
 * extract calls), a validity window outside 0..65535, a capacity outside 0 .. 2^31 - 1. */
typedef struct kfn_fuse_desc {
  int32_t struct_size;      /* = sizeof(kfn_fuse_desc) */
  int32_t nx, ny, nz;       /* lattice points */
  int32_t B, H, W;          /* frames of a call and their size (integrate) */
  int32_t raw_min, raw_max; /* the depth PNG's validity window: 1, 65534 */
  float ox, oy, oz;         /* world position of lattice point (0, 0, 0) */
  float voxel;              /* metres, > 0 */
  float trunc;              /* metres, > 0: 4 voxel */
  float near;               /* metres, > 0: 0.05 */
  float scale;              /* metres per raw unit: float(0.001) */
  float max_weight;         /* >= 1: the cap of W and wc */
  float min_weight;         /* >= 1: a point counts from this W on (extract) */
  float dfx, dfy, du, dv;   /* the depth camera */
  float fx, fy, u, v;       /* the colour camera */
} kfn_fuse_desc;
int kfn_fuse_scratch_bytes(const kfn_fuse_desc* desc, size_t* bytes);
int kfn_fuse_integrate(const kfn_fuse_desc* desc, float* tsdf, float* color, const uint16_t* depth, const uint8_t* frames,
                       const float* poses, void* stream);
int kfn_fuse_extract_count(const kfn_fuse_desc* desc, const float* tsdf, void* scratch, uint64_t* totals, void* stream);
int kfn_fuse_extract(const kfn_fuse_desc* desc, const float* tsdf, const float* color, const void* scratch, float* vertices,
                     uint8_t* colors, int32_t* triangles, int64_t cap_vertices, int64_t cap_triangles, void* stream);

/* ---- the camera tracked against the TSDF volume (added exports; the ABI number stays 13) ------------------------------------
 * The other half of KinectFusion: the model's surface by ray casting from the last committed pose, the new depth
 * map aligned to it by projective point-to-plane ICP, the frame integrated by kfn_fuse_integrate under the pose found.  The
 * volume is kfn_fuse's.  Every fp32 line below is one rounded operation in the order written, quotients and square roots IEEE
 * (kfnet_amd/csrc/kfn_track.hip repeats them, tests/track_ref.py restates them in numpy float32 and gets the same bits for the
 * maps and the per-pixel rows).  Poses are 12 numbers [R|t] row-major, camera to world: P[0..2], P[4..6], P[8..10] the rows of
 * R, P[3], P[7], P[11] the centre.
 *
 * Maps.  A map is [sum_l H_l W_l] quadruples of float; level l starts at quadruple sum_{k<l} H_k W_k and is row-major.  A valid
 * entry is (x, y, z, 1), an invalid one (0, 0, 0, 0): every launch tests the fourth component against 0.  Level 0 is H x W with
 * the depth camera (fx_0, fy_0, cu_0, cv_0) = (dfx, dfy, du, dv);  H_l = H_{l-1} / 2, W_l = W_{l-1} / 2 (floor), fx_l = fx_{l-1}
 * 0.5, cu_l = (cu_{l-1} - 0.5) 0.5, likewise fy, cv (pixel centres at integers: a 2 x 2 block's centre is at 2 x + 0.5).
 *
 * kfn_track_live_maps: depth [H,W] uint16 -> live_v, live_n (camera frame), `levels` levels.
 *   vertex 0   raw outside [raw_min, raw_max]: invalid.  z = float(raw) scale;  X = ((float(x) - cu_0) / fx_0) z, Y likewise.
 *   vertex l   from the block (2x, 2y), (2x+1, 2y), (2x, 2y+1), (2x+1, 2y+1) of level l-1, in this order: zmin = the least valid z;
 *              none valid: invalid.  sum = 0, cnt = 0; each valid z with z - zmin <= pyr_dist: sum = sum + z, cnt = cnt + 1.
 *              z' = sum / cnt;  X = ((float(x) - cu_l) / fx_l) z', Y likewise.
 *   normal     at (x, y) with v, r = the right neighbour, d = the lower one: invalid at the last row or column, where one of the
 *              three is invalid, or where |r.z - v.z| > jump or |d.z - v.z| > jump.  a = d - v, b = r - v per component;
 *              c = a x b: cx = ay bz - az by, cy = az bx - ax bz, cz = ax by - ay bx;  len = sqrt((cx cx + cy cy) + cz cz);
 *              invalid unless len > 0;  n = c / len per component.  It points towards the camera.
 *   There is no bilateral filter.
 *
 * kfn_track_raycast: level `level` of model_v, model_n (world frame) from tsdf and the record's COMMITTED pose, P[k] =
 * float(committed[k]).  One thread per pixel (x, y):
 *   1  qx = (float(x) - cu_l) / fx_l, qy likewise;  w = R (qx, qy, 1): wx = (P[0] qx + P[1] qy) + P[2], wy = (P[4] qx + P[5] qy)
 *      + P[6], wz = (P[8] qx + P[9] qy) + P[10].  The ray is c + t w: t is the depth along the camera's axis.
 *   2  len = sqrt((qx qx + qy qy) + 1);  dt = (trunc 0.5) / len: a step of half the truncation distance along the ray.
 *   3  lattice coordinates: gc = (P[3] - ox) / voxel ..., gd = wx / voxel ...;  the sample at t is g = gc + t gd per component.
 *   4  slab test against the box 0 .. n-1:  tmin = near, tmax = far; per axis x, y, z: i = 1 / gd, a = (0 - gc) i, b = (float(n-1) -
 *      gc) i, tmin = fmax(tmin, fmin(a, b)), tmax = fmin(tmax, fmax(a, b)) (fmin / fmax return the other operand of a NaN).
 *      Invalid unless every P[k] is finite, tmin < tmax and kf = floor((tmax - tmin) / dt) >= 0.  Samples k = 0 .. min(kf, 8191)
 *      at t_k = tmin + float(k) dt.
 *   5  a sample is usable iff floor(g) lies in 0 .. n-2 on every axis -- compared in float before the conversion -- and all
 *      eight lattice points around it have W >= min_weight.  D there is trilinear, a = g - floor(g), d_xyz the D of the point
 *      floor(g) + (x, y, z): along x first, c00 = d000 + a.x (d100 - d000), c10 = d010 + a.x (d110 - d010), c01 = d001 + a.x
 *      (d101 - d001), c11 = d011 + a.x (d111 - d011), then c0 = c00 + a.y (c10 - c00), c1 = c01 + a.y (c11 - c01), D = c0 +
 *      a.z (c1 - c0).
 *   6  walk: an unusable sample, or a usable one with D == 0 or NaN, forgets the previous one.  A usable D > 0 is remembered
 *      (Dp, tp).  The first usable D < 0 ends the walk: the surface iff the sample before it was a remembered D > 0; otherwise
 *      (a back face, or a way in from unknown space) the pixel is invalid.  No D < 0 up to the last sample: invalid.
 *   7  ts = tp + (Dp / (Dp - D)) (t - tp);  vertex = (P[3] + ts wx, P[7] + ts wy, P[11] + ts wz).
 *   8  normal: g = gc + ts gd;  the six samples at g +- (1, 0, 0), (0, 1, 0), (0, 0, 1), each by rule 5; one unusable: the normal
 *      is invalid (the vertex stays).  c = (D(+x) - D(-x), D(+y) - D(-y), D(+z) - D(-z)), len and n as for the live normal.
 *   No read leaves the volume for any pose: every index passes rule 5.  A non-finite pose gives an all-invalid map.
 *
 * kfn_track_icp_sums: level `level`, E[k] = float(estimate[k]), C[k] = float(committed[k]).  For every pixel whose live vertex v
 * and live normal nl are valid:
 *   1  p = E v: px = ((E[0] v.x + E[1] v.y) + E[2] v.z) + E[3], py, pz likewise with rows 1, 2.
 *   2  into the committed camera as kfn_fuse_integrate's step 2 (d = p - c; X = (C[0] dx + C[4] dy) + C[8] dz ...); a non-finite
 *      coordinate or Z < near: rejected.  cf = rint((X / Z) fx_l + cu_l), rf = rint((Y / Z) fy_l + cv_l); rejected unless 0 <=
 *      cf <= W_l - 1 and 0 <= rf <= H_l - 1, compared in float.  m, n = model vertex and normal there; either invalid: rejected.
 *   3  e = m - p;  dist = sqrt((ex ex + ey ey) + ez ez);  rejected unless dist <= dist_max.
 *   4  rn = R_E nl (three products, two sums a row, as step 1 without the centre);  rejected unless (rn.x n.x + rn.y n.y) + rn.z
 *      n.z >= cos_min.
 *   5  r = (n.x ex + n.y ey) + n.z ez;  J = (py n.z - pz n.y, pz n.x - px n.z, px n.y - py n.x, n.x, n.y, n.z): the row of the
 *      left-multiplied twist xi = (omega, upsilon), P <- exp(xi^) P.
 *   The 29 sums, fp64: J_a J_b for a <= b row-major (21), J_a r (6), r r, the count.  Each product of two floats is exact in fp64.
 *   Order: a thread adds its 4 pixels (index block 1024 + j 256 + thread, j ascending); a butterfly over the 64 lanes of a wave
 *   (xor 32, 16, .. 1); the four waves as (w0 + w1) + (w2 + w3); one row of 32 doubles per workgroup in scratch
 *   (kfn_track_scratch_bytes); a second launch adds the rows in index order into sums[32] (29 used).  No floating-point atomics,
 *   no workgroup waits for another: two launches give the same bits.
 *
 * kfn_track_update (one wave; fp64): writes last_pairs = count, last_share = count / (H_l W_l), last_rms = sqrt(sum r r / count)
 * (0 without pairs) and iterations += 1 into the record.  Then the iteration is REFUSED, the estimate left as it is, when count <
 * min_pairs; when the Cholesky factorisation A = L L^T of the 6 x 6 system meets a pivot d_j with not d_j > pivot_floor A_jj; or
 * when the solution of A xi = b or the new pose is not finite.  Otherwise exp(xi^) by Rodrigues' formula, theta = |omega|, K =
 * [omega]x: R = I + A K + B K^2, t = (I + B K + C K^2) upsilon, A = sin(theta) / theta, B = 2 sin^2(theta / 2) / theta^2, C = (1 -
 * A) / theta^2, and below theta = 1e-4 their series to theta^2;  estimate = exp(xi^) estimate;  the rotation is re-orthonormalised
 * by Gram-Schmidt on its columns (column 0 normalised, column 1 less its part along it, normalised, column 2 their cross product);
 * accepted += 1.
 *
 * kfn_track_commit (one wave), after the last iteration of a frame.  LOST when last_share < min_share, last_rms > max_rms,
 * accepted == 0, |centre - committed centre| > max_step_m, the angle acos((tr(R_E R_C^T) - 1) / 2) > max_step_rad, or the
 * estimate is not finite.  Tracked: committed = estimate; pose_rows[slot][0..11] = float(estimate) -- the row kfn_fuse_integrate
 * reads.  Lost: pose_rows[slot] = NaN, so integration skips the frame by its rule 1; lost += 1; estimate = committed.  Either way
 * row `frame` of trajectory [traj_rows][20] doubles (when frame < traj_rows) receives (pose[12] or NaN, lost 0 / 1, last_pairs,
 * last_share, last_rms, accepted, iterations, the step in metres, the step in radians); then frame += 1, accepted = iterations = 0.
 *
 * Everything runs on `stream`, allocates nothing and synchronises nothing; nothing is read back between the launches of a
 * frame.  KFN_ERR_ARG, and nothing launched: a wrong struct_size, a NULL or misaligned buffer, a non-positive image size, levels
 * outside 1 .. 4 or a coarsest level below 2 x 2, level outside 0 .. levels-1, a non-positive focal length or near; live maps:
 * scale <= 0, a window outside 0 .. 65535, a negative pyr_dist or jump; raycast: a lattice axis below 2 points, nx ny nz >= 2^31,
 * voxel <= 0, trunc <= 0, far <= near, min_weight < 1; icp_sums: dist_max <= 0, cos_min outside -1 .. 1; update: min_pairs < 6,
 * pivot_floor outside 0 .. 1; commit: slot outside 0 .. 65534, traj_rows < 1, min_share outside 0 .. 1, a non-positive limit. */
typedef struct kfn_track_state {
  double committed[12];     /* the last committed pose */
  double estimate[12];      /* the current estimate */
  double last_share, last_rms, last_pairs;   /* of the last iteration's sums */
  int32_t frame;            /* the trajectory row the next commit writes */
  int32_t lost;             /* frames lost so far */
  int32_t accepted;         /* iterations accepted since the last commit */
  int32_t iterations;       /* iterations run since the last commit */
} kfn_track_state;
typedef struct kfn_track_desc {
  int32_t struct_size;      /* = sizeof(kfn_track_desc) */
  int32_t nx, ny, nz;       /* the volume's lattice points (raycast) */
  int32_t H, W;             /* level 0 */
  int32_t levels;           /* 1 .. 4: 3 */
  int32_t level;            /* the level a raycast, icp_sums or update call works on */
  int32_t raw_min, raw_max; /* the depth PNG's validity window: 1, 65534 */
  int32_t min_pairs;        /* >= 6: 50 */
  int32_t traj_rows;        /* rows of the trajectory buffer (commit) */
  int32_t slot;             /* the pose row the commit writes */
  float ox, oy, oz;         /* world position of lattice point (0, 0, 0) */
  float voxel, trunc;       /* metres */
  float near, far;          /* the ray's limits in metres of depth: 0.05, 8 */
  float scale;              /* metres per raw unit: float(0.001) */
  float min_weight;         /* >= 1: a lattice point counts from this W on */
  float dfx, dfy, du, dv;   /* the depth camera at level 0 */
  float pyr_dist;           /* metres: 0.1 */
  float jump;               /* metres: 0.1 */
  float dist_max;           /* metres: 0.1 */
  float cos_min;            /* float(cos(20 degrees)) */
  float pivot_floor;        /* relative to the diagonal entry: 1e-10 */
  float min_share;          /* 0.1 */
  float max_rms;            /* metres: 0.04 */
  float max_step_m;         /* metres: 0.3 */
  float max_step_rad;       /* 0.35 */
} kfn_track_desc;
int kfn_track_scratch_bytes(const kfn_track_desc* desc, size_t* bytes);
int kfn_track_live_maps(const kfn_track_desc* desc, const uint16_t* depth, float* live_v, float* live_n, void* stream);
int kfn_track_raycast(const kfn_track_desc* desc, const float* tsdf, const kfn_track_state* state, float* model_v, float* model_n,
                      void* stream);
int kfn_track_icp_sums(const kfn_track_desc* desc, const float* live_v, const float* live_n, const float* model_v,
                       const float* model_n, const kfn_track_state* state, void* scratch, double* sums, void* stream);
int kfn_track_update(const kfn_track_desc* desc, const double* sums, kfn_track_state* state, void* stream);
int kfn_track_commit(const kfn_track_desc* desc, kfn_track_state* state, float* pose_rows, double* trajectory, void* stream);

/* ---- a lost tracker relocalised from fern-coded keyframes (added exports; the ABI number stays 13) ---------------------------
 * Keyframe relocalisation with randomised ferns (Glocker et al., TVCG 2015): every frame is coded by `ferns`
 * binary tests, the tracked frames whose code differs enough from those kept become keyframes with their pose, and after a loss
 * ICP restarts from the poses of the nearest codes and its own gates decide.  Four launches a frame beside the kfn_track_* ones,
 * in the order  live maps, ENCODE, SEARCH, SEED, ray casts, iterations, commit, SETTLE, integrate.  Each is launched every frame
 * and decides from the records on the device what to do; the arithmetic is integer or a copy of fp64 poses
 * (kfnet_amd/csrc/kfn_reloc.hip; tests/reloc_ref.py restates the rules below in numpy and gets the same bits).
 *
 * Buffers.  table [ferns][4] int32: (x, y, the bits of a float depth threshold in metres, R + 256 G + 65536 B thresholds 0 ..
 * 255);  code [ferns] uint8, the frame's code;  codes [capacity][ferns] uint8 and key_poses [capacity][12] double, the keyframes;
 * dist [capacity] int32, scratch of the search;  reloc_rows [rows][8] int32;  live_v, pose_rows, trajectory and the
 * kfn_track_state as in the kfn_track_* block.  Level sizes as there: H_l = H_{l-1} / 2, W_l = W_{l-1} / 2 (floor).
 *
 * kfn_reloc_encode: one byte per fern f from live_v at level reloc_level and, iff colour = 1, the staged frame [H,W,3] uint8.
 *   range    unless 0 <= x <= W_l - 1 and 0 <= y <= H_l - 1 the byte is 0 and nothing is read: the kernel tests it before any use.
 *   bit 0    v = the live vertex at (x, y) of the level: 1 iff v is valid (fourth component != 0) and v.z > threshold (float).
 *   bits 1-3 (colour = 1) for channel c = R, G, B: s = the int32 sum of the channel over the full-resolution pixels (x 2^l + i,
 *            y 2^l + j), 0 <= i, j < 2^l, l = reloc_level (they lie inside the frame because the sizes halve by floor); bit
 *            1 + c is 1 iff s > threshold_c 4^l.  With colour = 0 bits 1-3 are 0.
 *
 * kfn_reloc_search: n = min(max(state.n, 0), capacity).  For every keyframe i < n, d_i = the number of ferns f with code[f] !=
 * codes[i][f] (one wave per slot into dist; slots >= n exit, nothing is read beyond).  Then one workgroup writes into the state
 * cand_d[r], cand_index[r], r = 0 .. 3: the r-th least pair (d_i, i), ascending in d and, for equal d, in i, for r < min(tries,
 * n); (ferns + 1, -1) for every other r.  candidates = min(tries, n); min_d = cand_d[0] (ferns + 1 when n = 0).
 *
 * kfn_reloc_seed (one wave), before the ray casts.  n as above, c = min(max(state.candidates, 0), min(tries, n)).  It acts only
 * when streak > 0, c > 0 and i = cand_index[(streak - 1) mod c] lies in 0 .. n-1:  the tracker's committed = estimate =
 * key_poses[i];  seeded = 1;  seed_key = i.  Otherwise it writes nothing.
 *
 * kfn_reloc_settle (one wave), after kfn_track_commit and before kfn_fuse_integrate.  row = track.frame - 1, the trajectory row
 * the commit just wrote; TRACKED iff 0 <= row < traj_rows and trajectory[row][12] == 0;  n, c as above, streak = max(streak, 0),
 * SEEDED iff state.seeded == 1.  With first = 1 (the settle of frame 0, no commit before it) the frame is TRACKED and not
 * SEEDED, and the trajectory is not read.
 *   tracked, not seeded   streak = 0.  Harvest iff (n == 0 or min_d > harvest) and n < capacity:  codes[n] = code, key_poses[n]
 *                         = the tracker's committed pose, n += 1.
 *   tracked and seeded    verified iff last_share >= reloc_min_share and last_rms <= reloc_max_rms (as doubles).  Verified:
 *                         streak = 0, recovered += 1, no harvest.  Not verified: DEMOTED -- pose_rows[slot] = NaN (integration
 *                         skips the frame), trajectory[row][0..11] = NaN and [12] = 1, track.lost += 1, and the frame goes on
 *                         as a lost one.
 *   lost (or demoted)     if streak == 0 and not seeded: anchor = the tracker's committed pose, the last one truly tracked.
 *                         streak += 1.  If seeded: the tracker's committed = estimate = anchor.
 *   either way            seeded = 0, and reloc_rows[row] (when 0 <= row < rows) = (min_d, cand_index[0] or -1 when c == 0, seed_key
 *                         or -1 when not seeded, the keyframe added or -1, streak after, c, demoted 0 / 1, 0).
 *   So while streak > 0 the committed pose is the anchor on entry to the seed launch, and a keyframe's pose never outlives the
 *   frame it was tried on unless ICP's gates and the verification accepted it.
 *
 * Every index taken from a record is compared against its bound before use (n against capacity, a keyframe index against n, a
 * candidate against c, a row against rows and traj_rows): a record of garbage cannot cause an access out of range.  Everything
 * runs on `stream`, allocates nothing and synchronises nothing; no floating-point atomics, no workgroup waits for another: two
 * launches give the same bits.  KFN_ERR_ARG, and nothing launched: a wrong struct_size, a NULL or misaligned buffer (table,
 * live_v 16 bytes; state, track, key_poses, trajectory 8; dist, pose_rows, reloc_rows 4), a non-positive image size, levels
 * outside 1 .. 4 or a coarsest level below 2 x 2, reloc_level outside 0 .. levels-1, ferns outside 1 .. 4096, capacity outside
 * 1 .. 65536, tries outside 1 .. 4, rows < 1, harvest outside 0 .. ferns, colour not 0 / 1; encode: colour = 1 without a frame
 * or a frame with colour = 0; settle: slot outside 0 .. 65534, traj_rows < 1, first not 0 / 1, reloc_min_share outside 0 .. 1,
 * reloc_max_rms not positive and finite. */
typedef struct kfn_reloc_state {
  double anchor[12];        /* the last truly tracked pose, captured when a streak begins */
  int32_t n;                /* keyframes stored */
  int32_t streak;           /* lost frames in a row */
  int32_t seeded;           /* 1 between a seed that acted and the settle of its frame */
  int32_t seed_key;         /* the keyframe the last seed took */
  int32_t candidates;       /* min(tries, n) of the last search */
  int32_t min_d;            /* the least distance of the last search, ferns + 1 without keyframes */
  int32_t recovered;        /* seeded frames verified so far */
  int32_t reserved;         /* 0 */
  int32_t cand_d[4];        /* the nearest keyframes' distances, ascending */
  int32_t cand_index[4];    /* and their indices, -1 where there is none */
} kfn_reloc_state;
typedef struct kfn_reloc_desc {
  int32_t struct_size;      /* = sizeof(kfn_reloc_desc) */
  int32_t H, W;             /* level 0, as kfn_track_desc's */
  int32_t levels;           /* of the live maps, as kfn_track_desc's */
  int32_t reloc_level;      /* the level the ferns sit on: levels - 1 */
  int32_t ferns;            /* 1 .. 4096: 500 */
  int32_t capacity;         /* keyframe slots, 1 .. 65536: 1024 */
  int32_t tries;            /* 1 .. 4: 3 */
  int32_t harvest;          /* 0 .. ferns: floor(0.2 ferns) */
  int32_t rows;             /* rows of reloc_rows */
  int32_t traj_rows;        /* rows of the trajectory buffer (settle) */
  int32_t slot;             /* the pose row a demotion overwrites (settle) */
  int32_t first;            /* 1 for the settle of frame 0 */
  int32_t colour;           /* 1: the table's colour thresholds are used and a frame is given */
  float reloc_min_share;    /* the verification gates: the tracker's min_share and max_rms */
  float reloc_max_rms;
} kfn_reloc_desc;
int kfn_reloc_encode(const kfn_reloc_desc* desc, const int32_t* table, const float* live_v, const uint8_t* frame, uint8_t* code,
                     void* stream);
int kfn_reloc_search(const kfn_reloc_desc* desc, const uint8_t* code, const uint8_t* codes, kfn_reloc_state* state, int32_t* dist,
                     void* stream);
int kfn_reloc_seed(const kfn_reloc_desc* desc, kfn_reloc_state* state, kfn_track_state* track, const double* key_poses, void* stream);
int kfn_reloc_settle(const kfn_reloc_desc* desc, kfn_reloc_state* state, kfn_track_state* track, const uint8_t* code, uint8_t* codes,
                     double* key_poses, float* pose_rows, double* trajectory, int32_t* reloc_rows, void* stream);

/* ---- fine-tuning SCoordNet through the Kalman filter, OFlowNet frozen (added exports; the ABI number stays 13) ---------
 * Stage 3 of the reference under --fix_flownet (KFNet/train.py:268-298, KFNet.GetKFCoordBatch KFNet/KFNet.py:102-146;
 * DESIGN.md 6e).  A step sees S groups of T frames.  The forward filter is kfn_kalman_scan_ex with opt_temp and opt_kf, a
 * reset on frame 0 of every group, raw_on_reset = 0, no NIS gate and no transform: training and eval share that launch.
 *
 * kfn_measurement_map -- meas [pixels][4] = (x, y, z, exp(log sigma)) from SCoordNet's raw output pred [pixels][ld_pred]
 * (KFNet.GetMeasureCoord, KFNet/KFNet.py:60-68): what the scan reads as the measurement.  meas 16-byte aligned. */
int kfn_measurement_map(const float* pred, int ld_pred, float* meas, long pixels, void* stream);

/* kfn_filter_loss_grad -- L = weight_measure L_m + weight_temporal L_t + weight_kf L_KF (0.2, 0.2, 0.6: KFNet/train.py:293-295),
 * each term CoordLossWithUncertainty (KFNet/KFNet.py:192-232) + smooth_weight SmoothLoss (:430-467) of one of the three
 * outputs (MeasureCoordLoss :234-254, TemporalCoordLoss :256-278, KFCoordLoss :280-300) on the labels kfn_coord_loss_grad
 * reads, with one valid = sum(mask) + 1 over the whole batch.
 *   pred    [B,h,w,ld_pred]  the raw prediction (x, y, z, log sigma): sigma = exp(ch3)
 *   temp, kf [B,h,w,4]       the scan's opt_temp / opt_kf, B = S T: (x, sigma), the uncertainty u = max(sigma, min_uncertainty)
 *   labels, img, the clip, the threshold and the smoothness: as for kfn_coord_loss_grad
 *   dpred   [B,h,w,ld_dpred] channels 0..3 = weight_measure dL_m/dpred, as kfn_coord_loss_grad writes them
 *   d_temp, d_kf [B,h,w,4]   the DIRECT gradients dL/d(x, sigma) of the two filter outputs (kfn_filter_backward's input)
 *   stats[16] = (L, NLL of m / t / KF, smoothness of m / t / KF, accuracy of m / t / KF, valid, [11] not written here,
 *               the three terms NLL + smooth_weight smoothness, 0); L is formed in fp32 from the three rounded terms.
 * One workgroup, any grid; per-pixel terms in unfused fp32, sums in fp64 over a fixed tree; the smoothness never reaches
 * across a frame seam.  With weights (1, 0, 0) stats and dpred equal kfn_coord_loss_grad's bit for bit. */
typedef struct kfn_filter_loss_desc {
  int32_t struct_size;      /* = sizeof(kfn_filter_loss_desc) */
  int32_t B, h, w;
  int32_t ld_pred, ld_dpred;
  int32_t label_stride, img_stride;
  int32_t has_transform;
  float transform[12];      /* first 3 rows of transform.txt, row-major */
  int32_t has_loss_clip;
  float loss_clip;
  float smooth_weight;      /* 50 */
  float weight_measure, weight_temporal, weight_kf;   /* 0.2, 0.2, 0.6 */
  double dist_threshold;    /* 0.05: compared as float(dist_threshold * dist_threshold), 0x3B23D70A */
  double min_uncertainty;   /* 1e-5 */
} kfn_filter_loss_desc;
int kfn_filter_loss_grad(const kfn_filter_loss_desc* desc, const float* pred, const float* temp, const float* kf,
                         const float* labels, const uint8_t* img, float* dpred, float* d_temp, float* d_kf, float* stats,
                         void* stream);

/* kfn_filter_backward -- the reverse scan t = T-1 .. 0 per sequence: d_temp[t] and d_kf[t] go back through BuildKFCoord
 * (KFNet/KFNet.py:148-162: K, both max(1-K, 0) gates, the square root) to (z_t, sigma_z,t) and to (x^-, sigma^-); sigma^- through
 * the variance chain (:393-401) to s_l, zero where s_l^2 is below the floor float(min_uncertainty^2); (x^-, s_l) through the
 * transpose of tools.util.bilinear_sampler (tools/util.py:36-93, clamped corners, weights from the clamped corners) onto
 * KF_{t-1}, added to d_kf[t-1].  At t = 0 d_temp[0] + d_kf[0] fall on the measurement (KFNet.py:122-126).  The measurement's
 * gradients are added to dpred: channels 0..2 as they are, channel 3 times sigma_z.  Flow and sigma_trans are constants.
 *   flow_xy [S,T,HW,2], meas / temp / kf [S,T,HW,4]: the scan's inputs and outputs; frame 0's flow is not read
 *   d_temp  [S,T,HW,4] in;  d_kf [S,T,HW,4] in / out: on return the total gradient with respect to every KF_t
 *   dpred   [S T HW, ld_dpred] in / out;  scratch: kfn_filter_backward_scratch_bytes(), 16-byte aligned
 *   stats   word 11 receives, as a uint32, the number of pixels of frames >= 1 with |u| or |v| > radius (or NaN): their
 *           gradient would be lost, the caller must refuse the step when it is not 0.
 * The transpose is a gather: every source cell sums, rows then columns ascending, the targets within radius + 1 of it,
 * recomputing their corners and weights from the flow -- no floating-point atomics, so the result is bit-identical from
 * launch to launch and correct for every flow inside the radius.  T stream-ordered launches of S HW threads, any grid. */
typedef struct kfn_filter_backward_desc {
  int32_t struct_size;      /* = sizeof(kfn_filter_backward_desc) */
  int32_t S, T, H, W;
  int32_t ld_dpred;
  int32_t radius;           /* >= 4: the soft-argmax over offsets -4..3 cannot leave 4 */
  int32_t reserved;         /* 0 */
  double min_uncertainty;   /* 1e-5, as kfn_kalman_desc's */
} kfn_filter_backward_desc;
int kfn_filter_backward_scratch_bytes(const kfn_filter_backward_desc* desc, size_t* bytes);
int kfn_filter_backward(const kfn_filter_backward_desc* desc, const float* flow_xy, const float* meas, const float* temp,
                        const float* kf, const float* d_temp, float* d_kf, float* dpred, float* stats, void* scratch,
                        void* stream);

/* kfn_filter_backward_joint -- kfn_filter_backward for joint stage 3, where OFlowNet is trained too (KFNet/train.py:282-303):
 * the same descriptor, scratch size and launches, and on dpred, d_kf and stats word 11 the same bits.  Beside them it emits the
 * gradients with respect to the process model's two inputs (KFNet/KFNet.py:361-403 with tools/util.py:36-94), per frame
 * t >= 1 and cell q, from values the reverse scan holds already:
 *   av     [4]  the gradient with respect to the value (x^-, s_l) sampled from KF_{t-1} (s_l's is 0 where s_l^2 <= eps2)
 *   v_xy   [4]  KF_{t-1} at the forward's clamped corner (x = 0|1, y = 0|1); w_x0 = x1s - px, w_x1 = px - x0s, likewise in y
 *   d_flow[q] = (dL/du, dL/dv):  the weights' derivatives by px are -1 and +1, corner indices, floor and the clamps are
 *               piecewise constant (tools/util.py:36-59), so
 *               dL/du = sum_c av_c (w_y0 (v10_c - v00_c) + w_y1 (v11_c - v01_c))
 *               dL/dv = sum_c av_c (w_x0 (v01_c - v00_c) + w_x1 (v11_c - v10_c))
 *               two corners that clamp to one cell give 0 by themselves
 *   d_sigma_trans[q] = [sigma_trans^2 > eps2] d_lvar 2 sigma_trans, d_lvar the gradient with respect to sigma^-^2 and
 *               eps2 = float(min_uncertainty^2), the floor of kfn_kalman_scan_ex
 * Frame 0 of every group receives zeros in both.  ORDER: unfused fp32; inside the brackets the w_.0 product first; the sum over
 * c runs c = 0, 1, 2, 3 (x, y, z, sigma), ((t0 + t1) + t2) + t3.  No floating-point atomics: two launches give the same bits.
 *   sigma_trans [S,T,HW] in;  d_flow [S,T,HW,2] out, 8-byte aligned;  d_sigma_trans [S,T,HW] out;  the rest as above */
int kfn_filter_backward_joint(const kfn_filter_backward_desc* desc, const float* flow_xy, const float* sigma_trans,
                              const float* meas, const float* temp, const float* kf, const float* d_temp, float* d_kf,
                              float* dpred, float* d_flow, float* d_sigma_trans, float* stats, void* scratch, void* stream);

/* ---- training OFlowNet: stage 2 of the reference's procedure (added exports; the ABI number stays 13) -------------------
 * The backward pass of the Temporal scope (cnn_wrapper/OFlowNet.py:17-57, KFNet/KFNet.py:315-403) outside its convolutions,
 * and the loss of stage 2 (the reference's OFlowNet/train.py is absent, the loss is a stated deviation).
 * A step sees P pairs (a, b) of frames on the grid h x w = H/8 x W/8.  No floating-point atomics in any of the four: two
 * launches give the same bits.
 *
 * kfn_cost_volume_backward -- the transpose of kfn_cost_volume with window 8 (KFNet.BuildCoordVolume, KFNet/KFNet.py:343-359):
 *   d_vol [N H W, 8, 8, C] in;  d_f2, d_f1 [N,H,W,C] out (C % 4 == 0, all three 16-byte aligned)
 *   d_f2[p] =   sum_{i,j} d_vol[p, i, j]
 *   d_f1[q] = - sum_{i,j} d_vol[q - (i-4, j-4), i, j]   over the (i, j) whose cell q - (i-4, j-4) lies in q's frame
 * Both are gathers.  ORDER: each output element starts from +0.0f and adds its terms one by one in fp32, i ascending and j
 * ascending inside i; d_f1 skips the cells outside the grid and negates the finished sum.  A float32 restatement with the
 * same sequential adds is bit-identical. */
int kfn_cost_volume_backward(const float* d_vol, float* d_f2, float* d_f1, int N, int H, int W, int C, void* stream);

/* kfn_flow_head_backward -- through kfn_flow_softargmax (softmax over the 64 cells, cnn_wrapper/OFlowNet.py:45-47; flow =
 * sum_k prob_k o_k with o_k = (j-4, i-4), k = 8 i + j, KFNet/KFNet.py:381-385) and through sigma_trans = exp(pre) 1e-2
 * (OFlowNet.py:56):
 *   d_flow [N,2], prob [N,64], d_sigma [N], sigma_trans [N] in
 *   d_logits [N 64, ld_logits]: channel 0 of row 64 n + k = prob_k (o_k . g - sum_j prob_j o_j . g), g = d_flow[n]; the
 *            other ld_logits - 1 channels are zeroed (the padded gradient buffer of 'prediction'; ld_logits % 4 == 0)
 *   d_pre    [N, ld_pre]: channel 0 = d_sigma sigma_trans, the others zeroed (the padded gradient buffer of 'uncertainty') */
int kfn_flow_head_backward(const float* d_flow, const float* prob, const float* d_sigma, const float* sigma_trans,
                           float* d_logits, int ld_logits, float* d_pre, int ld_pre, long N, void* stream);

/* kfn_l2norm_backward -- through tf.nn.l2_normalize over feat7's channels (KFNet/KFNet.py:335-338),
 * y = x r with r = rsqrt(max(sum x^2, 1e-12)):  dx = r (g - y (y . g)) where sum x^2 > 1e-12, dx = 1e6 g where it is not.
 *   x [pixels, ldx] the tower's output BEFORE the normalisation, g [pixels, ldg] = dL/dy, dx [pixels, ld_dx]; C = 32 only;
 *   strides multiples of 4, buffers 16-byte aligned. */
int kfn_l2norm_backward(const float* x, int ldx, const float* g, int ldg, float* dx, int ld_dx, long pixels, int C,
                        void* stream);

/* kfn_flow_loss_grad -- the loss of stage 2 and its gradients.  Pair p is frames a = 2p and b = 2p + 1 of `labels`.
 *   flow_xy [P,h,w,2] = (u, v), sigma_trans [P,h,w]: OFlowNet's outputs for the pair, on frame b's grid
 *   labels  [2P, h label_stride, w label_stride, 4] = (gt xyz, mask), read as kfn_coord_loss_grad reads them; m = (mask == 1);
 *           no transform: the loss is invariant under a rigid one
 *   (px, py) = (x + u, y + v);  x^- = tools.util.bilinear_sampler (tools/util.py:36-93: clamped corners, weights from the
 *           clamped corners, add_n order) of label a's xyz at (px, py)
 *   valid_a = 1 where the four unclamped corners (floor px, floor py) + {0,1}^2 lie in the grid and have m_a = 1
 *   sigma^- = sqrt(eps2 + max(sigma_trans^2, eps2)), eps2 = float(min_uncertainty^2);  u = max(sigma^-, min_uncertainty)
 *   M = m_b valid_a,  d = sum_c (x^-_c - g_b,c)^2,  l = 3 log u + d / (2 u^2),  l = min(l, loss_clip) when has_loss_clip
 *   L = sum(M l) / (sum(M) + 1) over the whole batch
 *   d_flow  [P,h,w,2] = dL/d(u, v) through the sampler's weights (corner indices and M piecewise constant)
 *   d_sigma [P,h,w]   = M / (sum M + 1) (3/u - d/u^3) [sigma^- > min_uncertainty] [sigma_trans^2 > eps2] sigma_trans / sigma^-
 *   stats[16] = (L, accuracy = (valid - #{M d > dist_threshold^2}) / valid, valid = sum M + 1, #{valid_a == 0}, 0 ...)
 * One workgroup, any grid; per-cell terms in unfused fp32, sums in fp64 over a fixed tree. */
typedef struct kfn_flow_loss_desc {
  int32_t struct_size;      /* = sizeof(kfn_flow_loss_desc) */
  int32_t P, h, w;
  int32_t label_stride;
  int32_t has_loss_clip;
  float loss_clip;
  int32_t reserved;         /* 0 */
  double dist_threshold;    /* 0.05: compared as float(dist_threshold * dist_threshold), 0x3B23D70A */
  double min_uncertainty;   /* 1e-5: the floor of u, and squared (rounded once) the floor of both variances */
} kfn_flow_loss_desc;
int kfn_flow_loss_grad(const kfn_flow_loss_desc* desc, const float* flow_xy, const float* sigma_trans, const float* labels,
                       float* d_flow, float* d_sigma, float* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KFNET_HIP_H_ */

/*
 * tauv-vision_amd — C ABI of the MI355X (gfx950) CenterNet detection hot path.
 *
 * Drop-in boundary for TAUV-Vision's per-frame CenterNet path (reference
 * Tartan-AUV/TAUV-Vision @ 2024_10_08). The reference is pure Python on PyTorch; each
 * entry point below replaces the reference interface cited next to it. Plain pointers
 * and sizes only (device pointers are HIP device addresses, e.g. a torch tensor's
 * data_ptr()); `stream` is a hipStream_t (NULL = default stream). No exceptions cross
 * this ABI: every call returns TV_OK or a TV_E* code and sets a thread-local message
 * readable with tv_last_error().
 *
 * Layouts
 *   image input   fp32 NCHW [B,3,in_h,in_w], ImageNet-normalised (Centernet.forward,
 *                 centernet.py:65) — or raw u8 frames NHWC [B,in_h,in_w,3] with the
 *                 node's ToTensor+Normalize fused (centernet_node.py:90-92).
 *   head output   fp32 NHWC [B,out_h,out_w,out_cpad]; channel order = the reference
 *                 get_head_channels() order (centernet.py:114-142), out_cpad = round
 *                 up of the channel total to 4. Prediction fields are channel slices.
 *   records       fp32 [B][K][10] = label, score, y, x, h, w, depth (NaN if absent),
 *                 flat peak index (label*H*W + y*W + x), aux0, aux1 (optional pair
 *                 gathered at (label, y, x), e.g. the keypoint affinity of
 *                 decode.py:121-122; NaN if absent); counts int32 [B] = number of
 *                 records with score >= threshold (the host loop's break, decode.py:207).
 */
#ifndef TAUV_VISION_AMD_H
#define TAUV_VISION_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TV_OK 0
#define TV_EINVAL 1    /* bad argument (maps to ValueError / AssertionError) */
#define TV_ESHAPE 2    /* shape the reference would also reject */
#define TV_EHIP 3      /* HIP runtime error */
#define TV_ENOTFOUND 4 /* missing state_dict key */
#define TV_ENOMEM 5

/* TV_F32X3: fp32 activations and weights, each conv product on the pipelined implicit GEMM as three
 * fp16 MFMAs (hi = fp16(x), lo = fp16(x - hi): a_hi*b_hi + a_hi*b_lo + a_lo*b_hi, fp32 accumulation,
 * ~22-bit operands): within the fp32 path's 1e-4 golden tolerance, ~2x its throughput; TV_F32 is the
 * exact-f32 MFMA path. */
typedef enum tv_dtype { TV_F32 = 0, TV_F16 = 1, TV_BF16 = 2, TV_F32X3 = 3 } tv_dtype;

/* Model description: the fields of ModelConfig (config.py:6-35) plus the head list of
 * get_head_channels() (centernet.py:114-142). `arch` selects the network family:
 * TV_ARCH_CENTERNET = Centernet(DLABackbone(heights, channels, downsamples)) (centernet.py:32-92,
 * dla.py:393-416); TV_ARCH_DLA34 = CenterpointDLA34 (centerpoint_dla.py:544-578: DLA-34 base,
 * DLAUp/IDAUp with DCNv2, down ratio 4, head_conv 256; n_levels/heights/channels/downsamples
 * are ignored); TV_ARCH_PROTONET = the YOLACT protonet Masknet (masknet.py:8-55): channels[0] =
 * feature_depth, head_channels[0] = n_prototype_masks, (in_h, in_w) = the fpn[0] feature size;
 * tv_engine_forward takes fpn[0] as fp32 NCHW [B, feature_depth, in_h, in_w] and writes the
 * prototypes as fp32 NHWC [B, 4 in_h, 4 in_w, out_cpad]; TV_ARCH_CENTERNET_BACKBONE = the
 * DLABackbone alone (dla.py:393-416, DLABackbone.forward): the parameters are the "backbone.*"
 * keys of TV_ARCH_CENTERNET, n_heads / head_channels are ignored, and the output is the
 * IDAUpReverse feature map as fp32 NHWC [B, in_h / 2^downsamples, in_w / 2^downsamples,
 * channels[0]].
 *
 * TV_ARCH_YOLACT_HEAD = everything of Yolact.forward after the backbone (model.py:34-60):
 * FeaturePyramid (feature_pyramid.py:8-58), Masknet on fpn[0] and the one PredictionHead
 * (prediction_head.py:9-143) shared by every level; TV_ARCH_YOLACT_FPN = the FeaturePyramid alone.
 * Both take several inputs and write several outputs (tv_engine_forward_multi; the single-pointer
 * entry points return TV_EINVAL for them). Encoding:
 *   n_levels            len(in_depths), the number of backbone maps (1..TV_MAX_IO)
 *   channels[0]         feature_depth F;  channels[1 + i] = in_depths[i]
 *   downsamples         n_fpn_downsample_layers (n_levels + downsamples <= TV_MAX_IO)
 *   n_maps, map_h[i], map_w[i]   the size of backbone map i — independent inputs (a ResNet gives
 *                       69 / 35 / 18 at 550 x 550, not exact halvings); n_maps must equal n_levels
 *   in_h, in_w          ignored
 *   TV_ARCH_YOLACT_HEAD only (ignored by TV_ARCH_YOLACT_FPN):
 *   heights[0..3]       n_prediction_head_layers, n_classification_layers, n_box_layers, n_mask_layers
 *   n_heads = 2, head_channels[0] = n_prototype_masks k, head_channels[1] = n_classes C
 *   n_aspect_ratios     len(anchor_aspect_ratios) (>= 1)
 * Inputs: backbone map i as fp32 NCHW [B, in_depths[i], map_h[i], map_w[i]].
 * Outputs of TV_ARCH_YOLACT_FPN: level l < n_levels + downsamples as fp32 NHWC [B, h_l, w_l, F]
 * (h_l = map_h[l] for the first n_levels, then (h + 1) / 2 per stride-2 level).
 * Outputs of TV_ARCH_YOLACT_HEAD, all fp32 and contiguous, A = sum over levels of h_l w_l n_aspect_ratios:
 *   0 classification [B, A, C + 1]   1 box_encoding [B, A, 4]   2 mask_coeff [B, A, k] (tanh applied)
 *   3 mask_prototype NHWC [B, 4 map_h[0], 4 map_w[0], k rounded up to 4]
 * Row order of 0-2: levels in order, within a level (y * w_l + x) * n_aspect_ratios + a — the
 * reference's permute(0, 2, 3, 1).reshape (prediction_head.py:112-113). Parameters: the reference
 * Yolact state_dict keys without "_backbone.*" ("_feature_pyramid.*", "_masknet.*",
 * "_prediction_head.*"; the Bottleneck blocks in torchvision's layout conv1, bn1, conv2, bn2, conv3,
 * bn3 with bias-free convs); for TV_ARCH_YOLACT_FPN the FeaturePyramid's own keys, unprefixed.
 *
 * TV_ARCH_RESNET18 = the YOLACT backbone (yolact/model/backbone.py:9-32: torchvision's resnet18
 * tapped at layer2.1.bn2, layer3.1.bn2 and layer4.1.bn2 — the outputs of the last block's second
 * BatchNorm, before the residual add and the ReLU). Only in_h, in_w and compute_dtype are read.
 * Input: fp32 NCHW [B, 3, in_h, in_w] (tv_engine_forward_multi with one input). Outputs: the three
 * taps as fp32 NHWC [B, h, w, 128 / 256 / 512], (h, w) by the conv arithmetic: (in - 1) / 2 + 1 for
 * the stem, the max-pool and each of layer2..4 (550 -> 275, 138, 69, 35, 18). Parameters:
 * torchvision's resnet18 keys without "fc.*", unprefixed, in registration order ("conv1.weight",
 * "bn1.*", "layer1.0.conv1.weight", ..., "layer2.0.downsample.0.weight", "layer2.0.downsample.1.*",
 * ...; bias-free convs). in_h, in_w >= 1 (a 1 x 1 image gives 1 x 1 taps).
 *
 * TV_ARCH_YOLACT = the whole Yolact.forward (model.py:34-60) from the image: TV_ARCH_RESNET18, then
 * TV_ARCH_YOLACT_HEAD on its taps, which never leave the arena. Input: the image as for
 * TV_ARCH_RESNET18. Outputs: the four of TV_ARCH_YOLACT_HEAD over the taps' sizes. Head fields as
 * for TV_ARCH_YOLACT_HEAD (channels[0], downsamples, heights[0..3], n_heads, head_channels,
 * n_aspect_ratios); the backbone depths are fixed at (128, 256, 512): n_levels, channels[1..],
 * n_maps, map_h, map_w are ignored. Parameters: the whole reference state_dict, the backbone's keys
 * under "_backbone._feature_extractor.", then "_feature_pyramid.*", "_masknet.*",
 * "_prediction_head.*". Several outputs: the single-pointer entry points return TV_EINVAL. */
#define TV_ARCH_CENTERNET 0
#define TV_ARCH_DLA34 1
#define TV_ARCH_PROTONET 2
#define TV_ARCH_CENTERNET_BACKBONE 3
#define TV_ARCH_YOLACT_HEAD 4
#define TV_ARCH_YOLACT_FPN 5
#define TV_ARCH_RESNET18 6
#define TV_ARCH_YOLACT 7
#define TV_MAX_IO 8
typedef struct tv_model_desc {
  int32_t n_levels;          /* len(backbone_heights) */
  int32_t heights[8];        /* backbone_heights */
  int32_t channels[9];       /* backbone_channels, n_levels + 1 entries */
  int32_t downsamples;       /* ModelConfig.downsamples */
  int32_t n_heads;
  int32_t head_channels[16]; /* get_head_channels(object_config) */
  int32_t in_h, in_w;        /* ModelConfig.in_h / in_w */
  int32_t compute_dtype;     /* tv_dtype: TV_F32 = exact-f32 parity mode, TV_F32X3 its three-fp16-MFMA form */
  int32_t arch;              /* TV_ARCH_* */
  /* TV_ARCH_YOLACT_HEAD / TV_ARCH_YOLACT_FPN only (zero for the other archs) */
  int32_t n_maps;            /* number of (map_h, map_w) entries: must equal n_levels */
  int32_t map_h[TV_MAX_IO], map_w[TV_MAX_IO];
  int32_t n_aspect_ratios;   /* len(ModelConfig.anchor_aspect_ratios) */
} tv_model_desc;

typedef struct tv_engine tv_engine;

typedef struct tv_weight_view {
  const char* name;  /* reference state_dict key, e.g. "backbone.dla_down.projection_layer.0.weight" */
  const float* data; /* host fp32, contiguous, PyTorch layout */
  int64_t numel;
} tv_weight_view;

/* Reference state_dict layout of Centernet(DLABackbone(...)) in registration order
 * (what nn.Module.state_dict() yields; replaces model.state_dict() key/shape discovery,
 * centernet.py:32-61, dla.py:8-416). num_batches_tracked entries have ndim 0. */
int tv_model_param_count(const tv_model_desc* desc, int32_t* count);
int tv_model_param_info(const tv_model_desc* desc, int32_t index, char* name, int32_t name_cap,
                        int64_t shape[4], int32_t* ndim);
/* Algorithmic FLOPs per frame (2*MAC over every conv / conv-transpose) and output geometry. */
int tv_model_geometry(const tv_model_desc* desc, double* flops_per_frame, int32_t* out_h, int32_t* out_w,
                      int32_t* out_channels, int32_t* out_cpad);

/* Build an engine from reference-layout weights (replaces Centernet(...).to(device) +
 * load_state_dict(torch.load(...)) + eval(), centernet_node.py:46-48). BatchNorm is
 * folded (eval semantics, eps 1e-5); the engine owns its device copy and is immutable
 * after create, so concurrent forwards on different streams are safe. */
int tv_engine_create(const tv_model_desc* desc, const tv_weight_view* weights, int32_t n_weights,
                     int32_t device, tv_engine** out);
/* Diagnostics only (kernel A/B experiments, tools/): tv_engine_create with kernel-choice
 * overrides given explicitly as "NAME=VALUE;NAME=VALUE" (TV_C3_TW, TV_LAT, TV_SLICES, ... — the
 * list in engine.cpp); an unknown name is TV_EINVAL. The product entry point above takes none
 * and reads no environment variable. */
int tv_engine_create_diag(const tv_model_desc* desc, const tv_weight_view* weights, int32_t n_weights,
                          int32_t device, const char* knobs, tv_engine** out);
int tv_engine_destroy(tv_engine* engine);
/* Workspaces: the first forward of a batch size on a stream allocates that (stream, batch)
 * pair's activation arena (hipMalloc: not inside a graph capture) and keeps it for later calls;
 * a caller that cycles through many batch sizes or streams bounds the device memory with
 * tv_engine_trim. */
/* Allocate the per-(stream, batch) workspace up front (required before graph capture). */
int tv_engine_prepare(tv_engine* engine, int32_t batch, void* stream);
/* Free every cached workspace (synchronises the device; no forward on this engine may be in
 * flight or concurrent, and graphs captured over the freed arenas must not be replayed). */
int tv_engine_trim(tv_engine* engine);
/* Centernet.forward(img) -> Prediction heads (centernet.py:65-92). Async on `stream`. */
int tv_engine_forward(tv_engine* engine, const float* img_nchw, int32_t batch, float* out_nhwc, void* stream);
/* The caller's buffers of a desc, per frame: *n_in inputs, input i fp32 NCHW of in_shape[i] =
 * (C, H, W); *n_out outputs, output j fp32 NHWC of out_shape[j] = (H, W, C, cpad) — cpad the stored
 * channel count, C of them meaningful (a TV_ARCH_YOLACT_HEAD anchor-indexed output is (A, 1, width,
 * width)). One of each for the single-input archs. */
int tv_model_io(const tv_model_desc* desc, int32_t* n_in, int32_t in_shape[TV_MAX_IO][3], int32_t* n_out,
                int32_t out_shape[TV_MAX_IO][4]);
/* The forward of an arch with several inputs and outputs (any arch: n_in / n_out must be those of
 * tv_model_io): inputs[i] / outputs[j] device pointers to `batch` frames each, contiguous. Async on
 * `stream`; a batch that runs as concurrent slices advances every pointer by its own per-frame size. */
int tv_engine_forward_multi(tv_engine* engine, const float* const* inputs, int32_t n_in, float* const* outputs,
                            int32_t n_out, int32_t batch, void* stream);
/* tv_engine_profile over the same buffers. */
int tv_engine_profile_multi(tv_engine* engine, const float* const* inputs, int32_t n_in, float* const* outputs,
                            int32_t n_out, int32_t batch, void* stream, float* ms, double* flops, int32_t cap,
                            int32_t* n_ops);
/* tv_engine_forward_multi from raw u8 RGB camera frames NHWC [batch, in_h, in_w, 3] (any byte alignment)
 * with T.ToTensor + T.Normalize(ImageNet) fused into the first kernel (yolact_node.py:109-119 at the
 * model size: TV_ARCH_YOLACT, TV_ARCH_RESNET18; any arch whose one input is the image). A batch that runs
 * as concurrent slices advances the frame pointer by in_h * in_w * 3 bytes per frame. An arch that takes
 * feature maps (TV_ARCH_PROTONET, TV_ARCH_YOLACT_HEAD / _FPN) returns TV_EINVAL before any launch. */
int tv_engine_forward_multi_u8(tv_engine* engine, const uint8_t* frames_nhwc, int32_t batch, float* const* outputs,
                               int32_t n_out, void* stream);
/* tv_engine_profile_multi and tv_engine_op_outputs_multi over the same u8 frames (yolact_node.py:109-119);
 * tv_engine_op_kernel then names the kernel instances this input kind ran. */
int tv_engine_profile_multi_u8(tv_engine* engine, const uint8_t* frames_nhwc, int32_t batch, float* const* outputs,
                               int32_t n_out, void* stream, float* ms, double* flops, int32_t cap, int32_t* n_ops);
int tv_engine_op_outputs_multi_u8(tv_engine* engine, const uint8_t* frames_nhwc, int32_t batch,
                                  float* const* outputs, int32_t n_out, void* stream, void* const* dst, int32_t n_dst);
/* Same from raw u8 RGB frames with ToTensor + Normalize fused (centernet_node.py:90-92). */
int tv_engine_forward_u8(tv_engine* engine, const uint8_t* frames_nhwc, int32_t batch, float* out_nhwc,
                         void* stream);
/* Per-launch timing of one forward (HIP events on `stream`, synchronous): ms[i], flops[i]
 * per launch i < *n_ops (cap entries max); label(i) describes launch i. */
int tv_engine_profile(tv_engine* engine, const float* img_nchw, int32_t batch, float* out_nhwc, void* stream,
                      float* ms, double* flops, int32_t cap, int32_t* n_ops);
/* The same over raw u8 frames (the tv_engine_forward_u8 path). */
int tv_engine_profile_u8(tv_engine* engine, const uint8_t* frames_nhwc, int32_t batch, float* out_nhwc,
                         void* stream, float* ms, double* flops, int32_t cap, int32_t* n_ops);
/* Diagnostic: one forward_u8 exactly as it runs (concurrent slices, grouped launches) with a HIP
 * event before each launch on its slice's stream (synchronous): ms[k * cap + i] = in-situ duration
 * of op i's launch in slice k (a grouped launch's on its first op, 0 for the others), *n_slices
 * slices (tv_engine_slices). The durations include waiting for CUs the other slices hold, which is
 * what rocprofv3's kernel trace of the same run reports. */
int tv_engine_forward_insitu_u8(tv_engine* engine, const uint8_t* frames_nhwc, int32_t batch, float* out_nhwc,
                                void* stream, float* ms, int32_t cap, int32_t* n_slices);
/* Diagnostic: while on, every forward records the group events tv_engine_forward_insitu uses, also
 * into a graph captured meanwhile (event record nodes); tv_engine_insitu_read returns the times the
 * B-frame forward on `stream` (its workspaces' key: the capture stream) last recorded, e.g. after
 * a replay, in the ms[k * cap + i] layout above. */
int tv_engine_set_insitu(tv_engine* engine, int32_t on);
int tv_engine_insitu_read(tv_engine* engine, int32_t batch, void* stream, float* ms, int32_t cap, int32_t* n_slices);
/* The same over the normalised fp32 NCHW input (the tv_engine_forward path). */
int tv_engine_forward_insitu(tv_engine* engine, const float* img_nchw, int32_t batch, float* out_nhwc, void* stream,
                             float* ms, int32_t cap, int32_t* n_slices);
const char* tv_engine_op_label(tv_engine* engine, int32_t index);
/* What op `index` launches in a `batch`-frame workspace (its route): the kernel instance as a
 * profiler demangles it, e.g. "tv::c3::conv3x3<_Float16, _Float16, 32, 1, 0, 0, 4, 4, 8>" (a
 * split-K launch with " split-K n" appended; the stem kernels' input-mode argument — the last one of
 * stem_conv, stem_s2 and stem7s2_pool, 0 for the fp32 image — follows the input kind of the last
 * profile or op-outputs call), "prep" for the staging launch, or a parenthesised note for an op done
 * inside another op's launch, e.g. "(fused into the 3x3 heads)". "" before the batch's workspace
 * exists or past the last op. Diagnostic (roofline attribution, route table test). */
const char* tv_engine_op_kernel(tv_engine* engine, int32_t batch, int32_t index);
/* Diagnostic (per-layer tests): what op i < *n_ops of the `batch`-frame workspace on `stream` stores,
 * shape[i] = (H, W, C, element bytes) of its NHWC [batch, H, W, C] output tensor as stored (compute
 * dtype, 4 bytes for fp32 tensors; the op that writes the caller's output reports that buffer).
 * All zeros for an op whose output is never stored because another launch does its work: staging
 * inside the stem, the stem inside stem_s2, the 3x3 heads with the 1x1 heads in their epilogue,
 * fused DCN sampling, the ConvTranspose phases done by the phase-(0,0) launch. cap entries max.
 * Makes the workspace if it does not exist (allocates: not inside a stream capture). */
int tv_engine_op_shapes(tv_engine* engine, int32_t batch, void* stream, int32_t (*shape)[4], int32_t cap,
                        int32_t* n_ops);
/* Diagnostic: one forward of `batch` frames as tv_engine_profile runs it (one op per launch in
 * execution order, no slices) from `input` (input_u8 = 0: normalised fp32 NCHW, 1: u8 NHWC frames);
 * after op i < n_dst with dst[i] != NULL its stored tensor (tv_engine_op_shapes) is copied to the
 * device buffer dst[i] on `stream`, before the next op is launched. The data of the op that
 * writes the caller's output comes from out_nhwc (dst[i] may be out_nhwc itself: no copy). Archs
 * with one input and one output. Asynchronous like tv_engine_forward. */
int tv_engine_op_outputs(tv_engine* engine, const void* input, int32_t input_u8, int32_t batch, float* out_nhwc,
                         void* stream, void* const* dst, int32_t n_dst);
/* tv_engine_op_outputs over the buffers of tv_engine_forward_multi (any arch; an op that writes one of
 * the caller's outputs is read from that buffer; TV_ARCH_YOLACT_HEAD's scatter ops store no tensor). */
int tv_engine_op_outputs_multi(tv_engine* engine, const float* const* inputs, int32_t n_in, float* const* outputs,
                               int32_t n_out, int32_t batch, void* stream, void* const* dst, int32_t n_dst);
/* How a forward of `batch` frames is launched: as *n_slices (1..TV_MAX_SLICES) concurrent slices
 * of slice_batch[0..n_slices) frames, the rest of slice_batch zeroed (diagnostic: per-launch
 * roofline attribution). */
#define TV_MAX_SLICES 8
int tv_engine_slices(tv_engine* engine, int32_t batch, int32_t* n_slices, int32_t slice_batch[TV_MAX_SLICES]);

/* The node's preprocessing of camera frames (centernet_node.py:90-92): T.ToTensor (u8 / 255) ->
 * T.Resize((dst_h, dst_w)) (torchvision 0.15.2 tensor path: bilinear, align_corners=False, no
 * antialias, evaluated as torch's CPU upsample_bilinear2d does) -> T.Normalize(ImageNet). u8 RGB
 * frames NHWC [B, src_h, src_w, 3] -> normalised fp32 NCHW [B, 3, dst_h, dst_w], the input of
 * tv_engine_forward. (Frames already at the model size take tv_engine_forward_u8 instead: the
 * resize is then the identity and ToTensor + Normalize are fused into the stem.) */
int tv_preprocess_u8(const uint8_t* frames, int32_t B, int32_t src_h, int32_t src_w, int32_t dst_h, int32_t dst_w,
                     float* img_nchw, void* stream);

/* heatmap_nms(sigmoid?(heat), k) (decode.py:239-252) over any strided [B,C,H,W] fp32
 * view; `out` is dense [B,C,H,W]. k must be odd and >= 1 (else TV_EINVAL, like the
 * reference's assert). */
int tv_heatmap_nms(const float* heat, const int64_t strides[4], int32_t B, int32_t C, int32_t H, int32_t W,
                   int32_t kernel_size, int32_t apply_sigmoid, float* out, void* stream);
/* heatmap_detect (decode.py:255-279) on a dense [B, n] map: exact top-K per row,
 * descending, ties to the smaller flat index. */
int tv_heatmap_topk(const float* peaks, int32_t B, int64_t n, int32_t K, float* score, int32_t* index,
                    void* stream);
/* heatmap_detect()'s index [B,K,2] (y, x) and label [B,K] (int64) from flat indices
 * (decode.py:271-277; integer division, identical to the reference's float32 division
 * while C*H*W < 2^24). */
int tv_index_split(const int32_t* flat, int32_t B, int32_t K, int32_t H, int32_t W, int64_t* index, int64_t* label,
                   void* stream);
/* decode() (decode.py:179-236) / the object and keypoint parts of decode_keypoints()
 * (decode.py:56-135).
 * mode 0: y = (R*iy + offset_y)/in_h, depth = 1/sigmoid(d) - 1; mode 1: y = iy/out_h,
 * depth = 1/sigmoid(d), offset unused. Strides are element strides of the [B,C,H,W]
 * heatmap view and of the [B,H,W,ch] size/offset/depth views (depth may be NULL).
 * aux (may be NULL): pair gathered per record at element (b, label, j, y, x) with
 * aux_strides[5] (the [B,K,2,H,W] keypoint_affinity view).
 * workspace: tv_decode_workspace_size() bytes of device memory, ZERO-FILLED before its first use
 * (it carries the per-image peak keys and the arrival counters of the call's single launch, which
 * leaves the counters at zero again for the next call) — one call at a time per workspace. The
 * counters sit at fixed offsets (a 512 KiB head: one pair per image index up to 65535), so one
 * zero-filled workspace serves every later call whose tv_decode_workspace_size() it covers, at
 * any B or heatmap geometry. */
int tv_decode_workspace_size(int32_t B, int32_t C, int32_t H, int32_t W, int32_t K, int64_t* bytes);
int tv_decode(const float* heat, const int64_t heat_strides[4], const float* size, const int64_t size_strides[4],
              const float* offset, const int64_t offset_strides[4], const float* depth,
              const int64_t depth_strides[4], int32_t B, int32_t C, int32_t H, int32_t W, int32_t K,
              int32_t mode, int32_t ratio, int32_t in_h, int32_t in_w, float score_threshold,
              const float* aux, const int64_t aux_strides[5], float* records, int32_t* counts, void* workspace,
              int64_t workspace_bytes, void* stream);

/* Roll, pitch and yaw of the detections tv_decode wrote: the reference's angle_decode (decode.py:291-316,
 * the inverse of angle_loss's encoding, loss.py:334-376) evaluated at the records' peaks only — the step
 * its decode() leaves as "TODO: Decode angles". One small launch after tv_decode; device pointers, async
 * on `stream`, no workspace, no host synchronisation (graph-capturable).
 * records [B, K, rec_stride] fp32 (rec_stride >= 8) with counts [B] int32 (clamped to [0, K]), as written by
 * tv_decode in either mode: label, y and x of a record come from its flat peak index in column 7
 * (label*H*W + y*W + x, exact in fp32 while C*H*W < 2^24; TV_EINVAL otherwise).
 * Per axis, in Prediction order roll, pitch, yaw: the bin head and the offset head, [B, H, W, 4] fp32 views
 * with element strides[4] ([outside, inside] logits of bin 0 then bin 1; [sin, cos] offsets of bin 0 then
 * bin 1). Both pointers NULL: the head is absent. theta_range [3, C] fp32 on the device: the period of
 * axis a for label c (ObjectConfig.{roll,pitch,yaw}.modulo), NaN = not decoded for this label.
 * Per record and axis, in fp32, with b the four logits and o the four offsets at (b, y, x):
 *   s0 = softmax(b[0:2])[1], s1 = softmax(b[2:4])[1]; bin 1 is used when s1 > s0 (strict, on the fp32
 *   scores: two scores saturated to 1.0f choose bin 0);
 *   angle = use1 ? -pi/2 + atan2(o[2], o[3]) : pi/2 + atan2(o[0], o[1]);
 *   angles = remainder(angle, 2 pi) * (theta_range / (2 pi))      (torch.remainder: in [0, 2 pi))
 * The training bins' overlap does not enter the decode.
 * Output angles [B, K, 3] fp32 (roll, pitch, yaw), every element written by every call: NaN for rows
 * d >= counts[b], for an absent head, for a NaN theta_range, and for a flat index outside [0, C*H*W).
 * Packed layout (the Python DeviceDecoder's `packed`, the buffer RecordGather gathers): one allocation of
 * 4-byte elements — records [B, K, 10] fp32, then counts [B] int32, then, with the angles option, angles
 * [B, K, 3] fp32 — so one device-to-host copy or one collective carries all three; without the option the
 * buffer ends after the counts.
 * TV_EINVAL before any launch: null records, counts, theta_range or angles; rec_stride < 8; a bin head
 * without its offset head or the reverse; a present head without strides; non-positive C, H, W or K; B < 0;
 * C*H*W >= 2^24. B == 0 succeeds and launches nothing. */
int tv_decode_angles(const float* records, int32_t rec_stride, const int32_t* counts, const float* roll_bin,
                     const int64_t roll_bin_strides[4], const float* roll_offset, const int64_t roll_offset_strides[4],
                     const float* pitch_bin, const int64_t pitch_bin_strides[4], const float* pitch_offset,
                     const int64_t pitch_offset_strides[4], const float* yaw_bin, const int64_t yaw_bin_strides[4],
                     const float* yaw_offset, const int64_t yaw_offset_strides[4], const float* theta_range, int32_t B,
                     int32_t C, int32_t H, int32_t W, int32_t K, float* angles, void* stream);

/* YOLACT post-processing (reference src/tauv_vision/yolact/model/), fp32,
 * device pointers, async on `stream`.
 * box_decode (boxes.py:55-61): enc [B,A,4] (y, x, h, w encodings), anchor [anchor_batch,A,4]
 *   (anchor_batch 1 broadcasts like the reference's [1,A,4] anchors), out [B,A,4]. */
int tv_yolact_box_decode(const float* box_encoding, const float* anchor, int32_t B, int32_t A, int32_t anchor_batch,
                         float variance0, float variance1, float* box, void* stream);
/* box_encode (boxes.py:45-53): box [B,A,4] (y, x, h, w), anchor [anchor_batch,A,4] -> encodings [B,A,4]. */
int tv_yolact_box_encode(const float* box, const float* anchor, int32_t B, int32_t A, int32_t anchor_batch,
                         float variance0, float variance1, float* box_encoding, void* stream);
/* nms (nms.py:7-29): class-agnostic fast NMS of batch 0 — classification [A, C+1] logits and
 * box [A, 4] of batch 0; writes the kept anchor indices (descending confidence) to det[<= top_k]
 * (int64) and their number to *n_det (device int32). Any anchor count; the sort workspace is
 * allocated stream-ordered (hipMallocAsync) — use the batched entry point under graph capture. */
int tv_yolact_fast_nms(const float* classification, int32_t A, int32_t n_classes_with_bg, const float* box,
                       int32_t top_k, float iou_threshold, float confidence_threshold, int64_t* det, int32_t* n_det,
                       void* stream);
/* The same for B images at once (the reference's nms applied to every image of a batch):
 * classification [B,A,C+1], box [B,A,4] -> det [B][min(top_k, A)] int64 (row b: n_det[b] kept
 * indices), n_det [B] int32; workspace of tv_yolact_nms_workspace_size() bytes. */
int tv_yolact_nms_workspace_size(int32_t B, int32_t A, int32_t top_k, int64_t* bytes);
int tv_yolact_fast_nms_batched(const float* classification, int32_t B, int32_t A, int32_t n_classes_with_bg,
                               const float* box, int32_t top_k, float iou_threshold, float confidence_threshold,
                               int64_t* det, int32_t* n_det, void* workspace, int64_t workspace_bytes, void* stream);
/* assemble_mask (masks.py:8-21): prototypes [K,H,W] at element strides proto_strides (k, y, x) —
 * contiguous NCHW or the protonet's NHWC output view —, coefficients [n,K], box [n,4] (y, x, h, w
 * normalised) or NULL -> mask [n,H,W] = sigmoid(coeff . proto) x inclusive box mask. K <= 37. */
int tv_yolact_assemble_mask(const float* mask_prototype, const int64_t proto_strides[3], int32_t K, int32_t H,
                            int32_t W, const float* mask_coeff, const float* box, int32_t n, float* mask,
                            void* stream);
/* The same for B images: prototypes at strides (b, k, y, x), coefficients [B][n_max][K], boxes
 * [B][n_max][4] or NULL, counts [B] (device int32, detections per image; NULL = n_max) ->
 * masks [B][n_max][H][W] (rows d >= counts[b] untouched). */
int tv_yolact_assemble_masks(const float* mask_prototype, const int64_t proto_strides[4], int32_t B, int32_t K,
                             int32_t H, int32_t W, const float* mask_coeff, const float* box, const int32_t* counts,
                             int32_t n_max, float* mask, void* stream);
/* The node's mask step straight from the batched NMS output (yolact_node.py:134:
 * assemble_mask(proto[b], mask_coeff[b, det], box[b, det])): coefficients [B][A][K] and boxes
 * [B][A][4] (or NULL) of every anchor, det [B][n_max] int64 kept anchors and counts [B] as written
 * by tv_yolact_fast_nms_batched (n_max = its min(top_k, A)) -> masks [B][n_max][H][W]. */
int tv_yolact_assemble_masks_indexed(const float* mask_prototype, const int64_t proto_strides[4], int32_t B,
                                     int32_t K, int32_t H, int32_t W, const float* mask_coeff, const float* box,
                                     int32_t A, const int64_t* det, const int32_t* counts, int32_t n_max, float* mask,
                                     void* stream);

/* The node's per-detection outputs for the kept anchors of B images in one launch (yolact_node.py:129
 * F.softmax(classification), :139-141 classification_max / confidence of the detections): classification
 * [B,A,C+1] logits, box [B,A,4], det [B][n_max] int64 and counts [B] int32 as written by
 * tv_yolact_fast_nms_batched -> records [B][n_max][8] fp32 (16-byte aligned): the anchor index, the
 * class id (argmax of the logits over all C+1 columns, column 0 the background, the lowest index on an
 * exact tie), the softmax probability of that class, the largest foreground probability (max over
 * columns 1..C: the value nms.py:10 ranks by), the box y, x, h, w copied bit for bit. confidence (may be
 * NULL) [B][n_max][C+1]: the whole softmax row. Softmax in fp32, max-subtracted. Every row of both
 * outputs is written by every call; rows d >= counts[b] are zero. TV_EINVAL before any launch: null
 * pointers, A < 1 or A > 2^24 (the index would not be exact in fp32), C+1 < 2. B * n_max == 0 succeeds
 * and launches nothing. */
int tv_yolact_detection_records(const float* classification, const float* box, const int64_t* det,
                                const int32_t* counts, int32_t B, int32_t A, int32_t n_classes_with_bg, int32_t n_max,
                                float* records, float* confidence, void* stream);

/* Depth localisation of detections: the per-detection loops of the two reference nodes that turn
 * a detection into a camera-frame point, on the raw mono16 depth image. Device pointers, async on
 * `stream`, no workspace, no host synchronisation (graph-capturable).
 * depth [depth_batch, dh, dw] uint16 millimetres (depth_batch 1 broadcasts one image to all B). A
 * pixel is selected when it lies in the detection's region and its depth is not 0; n_pixels is
 * their number and sum_mm their exact 64-bit integer sum. depth_sum = sum_mm / 1000, z = sum_mm /
 * n_pixels / 1000 (double). The detection is invalid if n_pixels == 0, depth_sum < min_depth_sum
 * or z < min_z; otherwise x = (e_x - cx) * (z / fx), y = (e_y - cy) * (z / fy) (double).
 * out [B, K, 8] fp32 (16-byte aligned): x, y, z, valid (1 / 0), n_pixels, depth_sum, e_x, e_y.
 * Invalid rows carry x = y = z = 0 with their true n_pixels and depth_sum; rows k >= counts[b]
 * are all zero. Every row is written by every call.
 * TV_EINVAL: null pointers, non-positive sizes, depth_batch not 1 or B, fx or fy == 0.
 * B * K == 0 succeeds and launches nothing.
 *
 * tv_localize_boxes (centernet_node.py:139-178: the cv2.rectangle mask of +-0.4 w, +-0.4 h around
 * the centre, np.sum / np.mean of depth[(mask > 0) & (depth > 0)], the `< 10` and `z < 1`
 * skips and the back-projection): records [B, K, rec_stride] as written by tv_decode (y, x, h, w
 * in columns 2-5; rec_stride >= 6), counts [B]. In double, uncontracted, as the node's Python
 * floats: e_x = x dw, e_y = y dh, corners trunc(e_x -+ box_scale w dw), trunc(e_y -+ box_scale h dh)
 * (toward zero, like int()); the region is the filled rectangle between the corners, both
 * inclusive, in either order, clipped to the image. The node hard-codes 640 x 360, its depth size;
 * here dw, dh are the depth image's. A non-finite x, y, w or h selects nothing (valid = 0). The
 * node passes fx, fy, cx, cy = M_projection[0,0], [1,1], [0,2], [1,2], min_depth_sum 10, min_z 1. */
int tv_localize_boxes(const float* records, int32_t rec_stride, const int32_t* counts, int32_t B, int32_t K,
                      const uint16_t* depth, int32_t depth_batch, int32_t dh, int32_t dw, double box_scale, double fx,
                      double fy, double cx, double cy, double min_depth_sum, double min_z, float* out, void* stream);
/* tv_localize_masks (yolact_node.py:135,143,177-193: F.interpolate (nearest) of every mask to the
 * raw image size, the [n, H, W] copy to the host, np.nanmean(np.where(mask > 0.5, depth, nan)) with
 * zero depth as NaN, and the back-projection): masks [B, n, mh, mw] fp32 contiguous, det [B, n]
 * int64 and counts [B] as written by tv_yolact_fast_nms_batched, box [B, A, 4] (y, x, h, w);
 * e_y = box[b, det, 0] dh, e_x = box[b, det, 1] dw. The region is every depth pixel (yy, xx) with
 * masks[b, d, sy(yy), sx(xx)] > 0.5, sx(xx) = min((int)floorf((float)xx * ((float)mw / (float)dw)),
 * mw - 1) and likewise sy — torch's nearest map, in fp32; the up-sampled mask is never stored. A
 * det entry outside [0, A) gives an all-zero row. bound_by_box != 0 scans only the rows and columns
 * that can map into the detection's box crop (for masks assembled with that box, which are zero
 * outside it: the same result, fewer pixels read); 0 for masks assembled without a box. The node
 * passes the camera intrinsics and min_depth_sum = min_z = 0. */
int tv_localize_masks(const float* masks, int32_t mh, int32_t mw, const int32_t* counts, const int64_t* det,
                      const float* box, int32_t A, int32_t B, int32_t n, const uint16_t* depth, int32_t depth_batch,
                      int32_t dh, int32_t dw, int32_t bound_by_box, double fx, double fy, double cx, double cy,
                      double min_depth_sum, double min_z, float* out, void* stream);

/* The YOLACT instance masks at the size of the camera frame: what both reference callers do with the
 * assembled masks. evaluate_batch.py:98-102 runs F.interpolate(mask, (in_h, in_w), mode="bilinear") and
 * mask > 0.5; yolact_node.py:135,143 runs F.interpolate(mask, (H_raw, W_raw)) (nearest), copies [n, H, W]
 * fp32 to the host and uses mask_np > 0.5 (:184); both then blend every mask into the colour frame
 * (utils/plot.py:148-152, restated in evaluate_batch.py:136-139). Device pointers, async on `stream`, no
 * workspace, no host synchronisation (graph-capturable). The up-sampled fp32 mask is never stored.
 * masks [B, n, mh, mw] fp32 contiguous and counts [B] as tv_yolact_assemble_masks_indexed /
 * tv_yolact_fast_nms_batched write them; (H, W) the frame size; mode TV_FRAME_BILINEAR or
 * TV_FRAME_NEAREST. A frame pixel (y, x) of detection d < counts[b] is selected when its up-sampled
 * value is > 0.5 (strict; a NaN is not). Nearest: masks[b, d, sy(y), sx(x)] with tv_localize_masks' map
 * sx(x) = min((int)floorf((float)x * ((float)mw / (float)W)), mw - 1), likewise sy. Bilinear: torch's
 * align_corners=False arithmetic in fp32 per axis — scale = (float)in / (float)out, src = max(fma(scale,
 * dst + 0.5, -0.5), 0), i0 = (int)src, i1 = min(i0 + 1, in - 1), weights l1 = src - i0 and l0 = 1 - l1 —
 * and the value fma(t0, h0, t1 * h1) of the row blends t = fma(left, w0, right * w1) (tv_preprocess_u8's
 * arithmetic).
 * Every element of every output is written by every call:
 *   bits [B, n, H, ceil(W / 32)] uint32: pixel x is bit x % 32 of word x / 32; bits at x >= W are 0; rows
 *     d >= counts[b] are all zero.
 *   area [B, n] int32: the number of set bits of each row (0 past the count).
 *   overlay [B, H, W, 3] uint8, with frames [B, H, W, 3] uint8 (both NULL or both given; they may be the
 *     same buffer): a pixel starts from the frame's value and, for d = 0 .. counts[b] - 1 in that order,
 *     where its bit is set, each channel becomes (pix + colour[c]) >> 1 — exactly numpy's
 *     uint8(0.5 colour + 0.5 pix), which truncates. colour = palette[min(class_id, n_colours - 1)] (what
 *     ListedColormap returns for an index past its end; a negative id takes row 0), class_id = column 1 of
 *     records [B, n, 8] (tv_yolact_detection_records), palette [n_colours, 3] uint8 on the device.
 * bound_by_box != 0 (with det [B, n] int64, box [B, A, 4] as for tv_localize_masks, for masks assembled
 * with that box, which are zero outside it): a wave of 64 frame columns skips a detection whose box crop
 * — widened by one prototype pixel for bilinear, whose value above 0.5 needs a non-zero tap — cannot reach
 * its row and columns. Bit-equal to bound_by_box == 0. A det entry outside [0, A) is not bounded.
 * TV_EINVAL before any launch: null masks, counts, bits or area; non-positive mh, mw, H, W; an unknown
 * mode; bound_by_box without det, box or A >= 1; frames without overlay, records or palette (or overlay
 * without frames); n_colours < 1 with frames. B * n == 0 succeeds and launches nothing. */
#define TV_FRAME_BILINEAR 0
#define TV_FRAME_NEAREST 1
int tv_yolact_frame_masks(const float* masks, int32_t mh, int32_t mw, const int32_t* counts, int32_t B, int32_t n,
                          int32_t H, int32_t W, int32_t mode, int32_t bound_by_box, const int64_t* det, const float* box,
                          int32_t A, const uint8_t* frames, const float* records, const uint8_t* palette,
                          int32_t n_colours, uint32_t* bits, int32_t* area, uint8_t* overlay, void* stream);

/* The greedy keypoint-to-object matching of decode_keypoints() (decode.py:100-135) for B images in
 * one launch, on what tv_decode (mode 1) writes. Device pointers, async on `stream`, no workspace,
 * no host synchronisation (graph-capturable).
 * obj_records [B, K, 10] with obj_counts [B]; kp_records [B, K_kp, 10] with kp_counts [B] (label in
 * column 0, y, x in 2, 3, the affinity pair ay, ax in 8, 9); owner_label / owner_slot int32
 * [n_keypoints]: the object label and that object's keypoint slot of each flat keypoint index
 * (ObjectConfigSet.decode_keypoint_index); max_slots: the most keypoints any object has.
 * The keypoints of image b are taken in rank order 0 .. kp_counts[b]-1 (the record order is the
 * reference's score order, the count its `break`). The candidates of keypoint k with label kl are the
 * object records d < obj_counts[b] with label == owner_label[kl] whose slot owner_slot[kl] is still
 * free; without one, k stays unmatched. Otherwise err[d] = |atan2(ay, ax) - atan2(ky - y_d, kx - x_d)|
 * in double on the fp32 record values (the reference's Python floats; no wrap-around handling, as
 * there), the candidate of the smallest error wins, the smaller rank on a tie (errs.index(min(errs))),
 * the first candidate when the affinity is NaN (every error is NaN then), and its slot becomes taken.
 * A keypoint label outside [0, n_keypoints), or an owner slot outside [0, max_slots), has no candidate.
 * Outputs, every element written by every call:
 *   kp_det [B, K_kp] int32   the object rank keypoint k went to; -1 if unmatched or k >= kp_counts[b]
 *   slot_kp [B, K, max_slots] int32   the keypoint rank held by (object, slot), or -1
 *   n_matched [B, K] int32   the number of slots of the object that are held
 * One workgroup per image: the K_kp x K errors are computed in parallel into an LDS table when
 * K_kp * K <= 4096, inside the serial walk otherwise, with identical results.
 * TV_EINVAL before any launch: null pointers, B < 0, n_keypoints < 1, max_slots outside 1..32,
 * K outside 1..256, K_kp outside 1..1024. B == 0 succeeds and launches nothing. */
int tv_match_keypoints(const float* obj_records, const int32_t* obj_counts, const float* kp_records,
                       const int32_t* kp_counts, const int32_t* owner_label, const int32_t* owner_slot,
                       int32_t n_keypoints, int32_t max_slots, int32_t B, int32_t K, int32_t K_kp, int32_t* kp_det,
                       int32_t* slot_kp, int32_t* n_matched, void* stream);

/* The pose stage of decode_keypoints() (decode.py:137-172, cv2.solvePnP(SOLVEPNP_ITERATIVE) there) for
 * B x K detections in one launch, on what tv_decode (mode 1) and tv_match_keypoints leave on the device.
 * Device pointers, async on `stream`, no workspace, no host synchronisation (graph-capturable).
 * obj_records [B, K, 10] with obj_counts [B] and kp_records [B, K_kp, 10] with kp_counts [B] (counts
 * clamped to [0, K] / [0, K_kp]); slot_kp [B, K, max_slots] int32 (tv_match_keypoints'); model_points
 * [n_labels, max_slots, 3] fp32, the object's keypoints in its own frame, a NaN row = no such slot.
 * The points of detection (b, d), d < obj_counts[b], label L = (int)obj_records[b, d, 0]: the slots s with
 * model_points[L, s] free of NaN and k = slot_kp[b, d, s] in [0, min(kp_counts[b], K_kp)), in slot order;
 * image point u = (double)kp[b, k, 3] * in_w, v = (double)kp[b, k, 2] * in_h (decode.py:155), object point
 * model_points[L, s]. A label outside [0, n_labels) has no points.
 * With n >= min_points points the pose is the (R, t) that minimises sum (fx Xc/Zc + cx - u)^2 +
 * (fy Yc/Zc + cy - v)^2, Xc = R X + t, in double on the fp32 inputs: a linear start in the normalised
 * coordinates ((u - cx) / fx, (v - cy) / fy) on centred and scaled object points - a homography and its
 * decomposition when the smallest eigenvalue of the centred 3 x 3 scatter is below 1e-6 of the middle one
 * (coplanar), the 12-parameter DLT otherwise; the sign that makes the mean depth positive; the rotation
 * part replaced by the nearest rotation - polished by Levenberg-Marquardt on a rotation-vector increment
 * (R <- exp([w]x) R) and t with analytic Jacobians. It ends on a step of at most 1e-12 (1 + |t|) or when no
 * damping lowers the cost; every loop is bounded (30 Jacobi sweeps, 50 LM iterations of at most 12
 * dampings). Only fx, fy, cx, cy of the camera are used; no distortion. A planar target has two minima:
 * which one is returned is decided by the linear start. This is the minimiser defined here, not a
 * restatement of OpenCV's iteration.
 * poses [B, K, 16] fp32, every element written by every call:
 *   0-8 R row-major, 9-11 t, 12 valid (1 / 0), 13 n (the points used), 14 RMS reprojection error in
 *   pixels (sqrt(sum / n)), 15 LM iterations.
 * valid = 0 - columns 0-11 and 14 NaN - when n < min_points, when a point or the start is not finite (NaN
 * keypoints), when all object points or all pixels of the detection are equal, without convergence in 50
 * iterations, or when a point ends at depth <= 0.
 * Rows d >= obj_counts[b] have n = 0 and valid = 0.
 * One wave per detection; the matrices live in LDS.
 * TV_EINVAL before any launch: null pointers, B < 0, K outside 1..256, K_kp outside 1..1024, max_slots
 * outside 1..32, n_labels < 1, min_points outside 6..32, non-positive in_h / in_w, fx or fy not finite or
 * zero. B == 0 succeeds and launches nothing. */
int tv_solve_poses(const float* obj_records, const int32_t* obj_counts, const float* kp_records,
                   const int32_t* kp_counts, const int32_t* slot_kp, const float* model_points, int32_t n_labels,
                   int32_t max_slots, int32_t B, int32_t K, int32_t K_kp, int32_t in_h, int32_t in_w, float fx, float fy,
                   float cx, float cy, int32_t min_points, float* poses, void* stream);

/* The detection-to-truth matching of the reference's evaluation scripts (centernet/scripts/evaluate.py:
 * 188-203, evaluate_keypoints.py:143-153) for B images in one launch, and the counts of their precision
 * and recall for T score thresholds at once. Device pointers (cols is a host array), async on `stream`,
 * no workspace, no host synchronisation (graph-capturable).
 * records [B, K, rec_stride] fp32 with counts [B] int32 (clamped to [0, K]); cols[6]: the columns of label,
 * score, y, x, h, w (a tv_decode record: 0, 1, 2, 3, 4, 5; a tv_yolact_detection_records row: 1, 3, 4, 5, 6,
 * 7). Truths of image b: truth_valid [B, N] u8 (bool), truth_label [B, N] int64, truth_center [B, N, 2]
 * fp32 (y, x), truth_size [B, N, 2] fp32 (h, w; may be NULL when mode == 1). score_thresholds [T] fp32, in
 * any order.
 * The records of an image are walked in descending score, the LATER record first among equal scores
 * (reversed(sorted(.., key=score)): a stable sort, reversed); the records need not arrive sorted. Each
 * takes the first truth, in truth order, that is valid, not yet taken, has int(label) equal to its own and
 * passes the match test; that truth is then taken. The first qualifying truth wins, not the best one.
 *   mode 0 (box, evaluate.py:106-130): ya = max(y1 - h1/2, y2 - h2/2), xa likewise, yb = min(y1 + h1/2,
 *     y2 + h2/2), xb likewise, inter = abs(max(yb - ya, 0) * max(xb - xa, 0)), iou = 0 if inter == 0 else
 *     inter / (w1 h1 + w2 h2 - inter); the pair passes when iou >= match_threshold. With match_threshold
 *     <= 0 every pair of equal labels passes, disjoint boxes included, as in the reference.
 *   mode 1 (centre, evaluate_keypoints.py:61-71): the pair passes unless sqrt((y1 - y2)^2 + (x1 - x2)^2) >
 *     match_threshold. Only label, score, y, x of the records are read.
 * Both in double on the fp32 values, uncontracted, in the order written (Python's max / min: the first
 * argument unless the second is strictly beyond it).
 * The detections of the reference at score threshold t are the records with score >= t (fp32 compare, an
 * equal score counts): a prefix of the walk, so one walk serves every threshold. A NaN score passes no
 * threshold and walks last (the reference never produces one: outside its behaviour).
 * Outputs:
 *   det_truth [B, K] int32   the truth index record k took, or -1; rows k >= counts[b] are -1. Every
 *                            element is written by every call.
 *   totals [2T + 1] int64    n_tp[T], n_detections[T], n_truth. The call ADDS to them (integer atomics):
 *                            n_tp[t] += records with score >= t that took a truth, n_detections[t] += records
 *                            with score >= t, n_truth += valid truths. A data set is a run of calls on one
 *                            zeroed buffer, in any order. precision = n_tp / n_detections (1 when there is
 *                            no detection), recall = n_tp / n_truth.
 * One workgroup per image; the K x N match tests run in parallel into 64-bit masks in LDS, one wave walks.
 * TV_EINVAL before any launch, with nothing written: null pointers (truth_size only when mode == 0), B < 0,
 * K outside 0..1024, N outside 1..256, T outside 1..64, mode not 0 or 1, rec_stride < 1, a column outside
 * [0, rec_stride). B == 0 or K == 0 succeeds and launches nothing (nothing is added). */
int tv_evaluate_detections(const float* records, int32_t rec_stride, const int32_t* counts, const int32_t cols[6],
                           int32_t B, int32_t K, const uint8_t* truth_valid, const int64_t* truth_label,
                           const float* truth_center, const float* truth_size, int32_t N, int32_t mode,
                           double match_threshold, const float* score_thresholds, int32_t T, int32_t* det_truth,
                           int64_t* totals, void* stream);

/* YOLACT evaluation, step 1 of 2: the pixel counts behind the mask IoU of every (detection, truth) pair of
 * B images. Device pointers, async on `stream`, no workspace, no allocation, no host synchronisation
 * (graph-capturable).
 * bits [B, K, H, ceil(W / 32)] uint32 in tv_yolact_frame_masks' layout (pixel x is bit x % 32 of word
 * x / 32), counts [B] int32 (clamped to [0, K]), seg [B, H, W] uint8, truth_valid [B, N] u8 (bool).
 * The reference's truth is one seg map (segmentation_dataset.py:97-100, read as seg == match_index in
 * loss.py:86), so the truth masks are disjoint:
 *   truth t of image b owns the pixels with seg == t, provided t < N and truth_valid[b, t];
 *   seg == 254 is invalid image (img_valid = seg != 254): such a pixel is left out of every count;
 *   every other value is background, a value < N whose truth is not valid included.
 * Outputs, every element written by every call:
 *   inter [B, K, N] int32     valid pixels where bit d is set and truth t owns the pixel;
 *   det_area [B, K] int32     valid pixels with bit d set;
 *   truth_area [B, N] int32   pixels truth t owns.
 * Rows d >= counts[b] are not read and give zeros, whatever the buffer holds there; bits at x >= W are not
 * counted, whatever they hold. Two launches: the zeroing and the pass (a workgroup per image and band of 8
 * rows, a lane per detection, popcounts into LDS, integer atomics at the end: reproducible).
 * TV_EINVAL before any launch, with nothing written: a null pointer, B outside 1..65535, K outside 1..256,
 * N outside 1..64, H or W < 1, W > 2^30, H * W > 2^31 - 1. */
int tv_yolact_mask_overlap(const uint32_t* bits, const int32_t* counts, const uint8_t* seg, const uint8_t* truth_valid,
                           int32_t B, int32_t K, int32_t N, int32_t H, int32_t W, int32_t* inter, int32_t* det_area,
                           int32_t* truth_area, void* stream);

/* YOLACT evaluation, step 2 of 2: the detection-to-truth matching behind box and mask average precision at
 * T IoU thresholds, for B images in one launch (one workgroup per image) plus a one-thread launch that adds
 * B to the cursor. Device pointers, async on `stream`, no allocation, no host synchronisation
 * (graph-capturable).
 * confidence [B, K, C + 1] fp32: the softmax rows of tv_yolact_detection_records; records [B, K, 8] of the
 * same call, of which only the box in columns 4..7 (y, x, h, w) is read; counts [B] int32 (clamped to
 * [0, K]); truth_valid [B, N] u8, truth_label [B, N] int64, truth_box [B, N, 4] fp32 (y, x, h, w); inter,
 * det_area, truth_area of tv_yolact_mask_overlap; iou_thresholds [T] fp32 in any order.
 * Rules:
 *   - A detection's label is 1 + argmax over the foreground columns 1..C (a strict `>` scan from column 1:
 *     the lowest index on a tie, and a NaN never replaces the running best); its score is that
 *     probability. The background column never names a detection; records column 1 is not used (its argmax
 *     includes the background).
 *   - Walk order: descending score; among equal scores the lower record index first; a NaN score last.
 *     The rank is computed from the scores: the records need not be sorted.
 *   - Per kind (0 box, 1 mask) and threshold tau_j, independently: the detection takes the truth with the
 *     largest IoU among the truths that are valid, still free at (kind, j), carry its label and have
 *     IoU >= (double)tau_j; the lowest truth index wins a tie. It is then a true positive at j and the
 *     truth is taken at j.
 *   - Mask IoU = double(inter) / double(det_area + truth_area - inter), 0 when that union is 0.
 *   - Box IoU in double on the fp32 values, uncontracted, in this order: corners c - s / 2 and c + s / 2;
 *     sides min(upper) - max(lower), clamped at 0 (s > 0 ? s : 0); inter = sy * sx; a_d = h_d * w_d,
 *     a_t = h_t * w_t; den = a_d + a_t - inter; IoU = 0 when den <= 0, else inter / den.
 *   - A valid truth whose label is outside 1..C matches nothing and is counted in n_bad_label only.
 * Outputs:
 *   det_truth [B, K, 2, T] int32   the truth each record took per (kind, threshold), or -1; rows
 *                                  k >= counts[b] are -1. Every element is written by every call.
 *   log [capacity, K, 4] 32-bit words, 16-byte aligned: image b of the call writes row cursor[0] + b (the
 *                                  cursor as it is when the launch runs), all K records: word 0 the score
 *                                  (fp32), word 1 the label (int32), word 2 the tp word (uint32: bit j box
 *                                  true positive at threshold j, bit 16 + j mask), word 3 = 1; a record
 *                                  k >= counts[b] is four zero words. A row at or past `capacity` is not
 *                                  written; the cursor advances all the same.
 *   cursor [1] int64               += B, by a launch of its own behind the matching (stream-ordered).
 *   totals [C + 2] int64           ADDED to (integer atomics): n_truth[label] for label 0..C (entry 0 stays
 *                                  0), then n_bad_label.
 * TV_EINVAL before any launch, with nothing written: a null pointer, B < 1, K outside 1..256, N outside
 * 1..64, C outside 1..254, T outside 1..16, capacity < 0, a log that is not 16-byte aligned. (Any B >= 1 is
 * taken here; tv_yolact_mask_overlap, which comes first, refuses B > 65535.) */
int tv_yolact_evaluate_match(const float* confidence, const float* records, const int32_t* counts,
                             const uint8_t* truth_valid, const int64_t* truth_label, const float* truth_box,
                             const int32_t* inter, const int32_t* det_area, const int32_t* truth_area,
                             const float* iou_thresholds, int32_t B, int32_t K, int32_t N, int32_t C, int32_t T,
                             int64_t* cursor, int32_t* log, int64_t capacity, int32_t* det_truth, int64_t* totals,
                             void* stream);

/* Training augmentation of B u8 camera frames in two launches: one sample of the reference's A.Compose
 * pipelines (yolact/scripts/train.py:413-455, centernet/scripts/train.py:144-167) per frame, applied in
 * ONE resampling, then colour, noise, blur and Normalize. Device pointers, async on `stream`, no
 * allocation, no host synchronisation (graph-capturable). The result is a pure function of (frames, seg,
 * records, seed): no atomics, every sum in a fixed order, so a rerun is bit-identical.
 * frames [B, Hs, Ws, 3] uint8; seg [B, Hs, Ws] uint8 with seg_out [B, Hd, Wd] uint8 (both NULL or both
 * given); img_out [B, 3, Hd, Wd] fp32; mean[3], std[3]: host arrays (Normalize); seed: the noise key.
 * records [B, 32] fp32 on the device, one per frame, unused slots zero:
 *   0-8    minv, row-major: the inverse homography, destination to source continuous coordinates (pixel
 *          i covers [i, i + 1), centre i + 0.5)
 *   9-11   perm: output channel c takes source channel perm[c] (clamped to 0..2)
 *   12-14  brightness, contrast, saturation factors (1 = identity)
 *   15     hue, a fraction of a turn;  16, 17  sat_shift, val_shift, added to HSV s and v in [0, 1]
 *   18     noise_sigma in u8 units (0 = none);  19  blur_k in {1, 3, 5, 7} (clamped to that set)
 * Destination pixel (b, y, x), (X, Y) = (x + 0.5, y + 0.5), everything in fp32 as written, no contraction:
 *   w = (m6 X + m7 Y) + m8, u = ((m0 X + m1 Y) + m2) / w, v = ((m3 X + m4 Y) + m5) / w;
 *   inside = w > 0 && 0 <= u < Ws && 0 <= v < Hs;  seg_out = inside ? seg[b, (int)v, (int)u] : 254.
 *   Outside, the value p before the blur is 0 (the padding takes no colour and no noise). Inside: bilinear
 *   at (u - 0.5, v - 0.5) with tv_preprocess_u8's clamped taps and blend on the u8 values (0..255, never
 *   rounded back to u8), channels through perm; c = clamp(c brightness, 0, 255); c = clamp(contrast c +
 *   (1 - contrast) mu_b, 0, 255), mu_b the mean over the whole source frame of gray(clamp(brightness
 *   perm(src))), gray = (0.299 r + 0.587 g) + 0.114 b; c = clamp(saturation c + (1 - saturation) gray(c),
 *   0, 255); if hue, sat_shift or val_shift is non-zero: RGB / 255 -> HSV, h = frac(h + hue), s and v
 *   shifted and clamped to [0, 1], back to RGB * 255; c = clamp(c + noise_sigma n_c, 0, 255) with
 *   Philox4x32-10 (key = seed, counter = (x, y, b, 0), outputs o0..o3), u_i = ((float)(o_i >> 8) + 0.5f)
 *   2^-24, n_R = sqrt(-2 ln u0) cos(2 pi u1), n_G the same with sin, n_B = sqrt(-2 ln u2) cos(2 pi u3).
 *   q = mean of p over the blur_k x blur_k window, reflect-101 at the destination border (a reflected
 *   position is evaluated like any other, noise included; blur_k <= min(Hd, Wd) is the caller's to
 *   ensure: further out the position is clamped); q = inside ? q : 0;
 *   img_out[b, c, y, x] = (q / 255 - mean[c]) / std[c].
 * workspace: tv_augment_workspace_size(B, Hs, Ws) bytes, 8-byte aligned, uninitialised: the partial sums
 * of mu_b (one double per 4096 source pixels per frame; frames with contrast == 1 skip them).
 * Every element of img_out and seg_out is written by every call.
 * TV_EINVAL before any launch: null frames, records, mean, std, img_out or workspace; seg without seg_out
 * or the reverse; B < 1 or > 65535; a non-positive size; Hs Ws 3 or Hd Wd >= 2^31; a zero std; a
 * workspace that is too small or misaligned. */
int tv_augment_workspace_size(int32_t B, int32_t src_h, int32_t src_w, int64_t* bytes);
int tv_augment_frames(const uint8_t* frames, const uint8_t* seg, int32_t B, int32_t src_h, int32_t src_w,
                      int32_t dst_h, int32_t dst_w, const float* records, uint64_t seed, const float mean[3],
                      const float std[3], float* img_out, uint8_t* seg_out, void* workspace, int64_t workspace_bytes,
                      void* stream);

/* Training targets of the CenterNet loss (loss.py:31-135), fp32, device pointers, async on `stream`.
 * generate_heatmap (loss.py:31-72): valid [B,n_objects] u8 (bool), label [B,n_objects] int64,
 *   center [B,n_objects,2] fp32 (y, x normalised) -> heatmap [B,n_labels,in_h/ratio,in_w/ratio]:
 *   per valid object exp(-((x-cx)^2 + (y-cy)^2) / (2 sigma^2)) maxed into its label's plane, with
 *   (cy, cx) = floor(center * in / ratio) and sigma = max(sigma, 0.1) (the reference passes
 *   TrainConfig.keypoint_heatmap_sigma); nan_to_num. A label outside [0, n_labels) is skipped
 *   (the Python wrapper raises IndexError first, like the reference's indexing). */
int tv_train_heatmap(const uint8_t* valid, const int64_t* label, const float* center, int32_t B, int32_t n_objects,
                     int32_t n_labels, int32_t in_h, int32_t in_w, int32_t downsample_ratio, double sigma,
                     float* heatmap, void* stream);
/* generate_keypoint_heatmap (loss.py:75-135): keypoint instances [B,n_instances] (valid u8, label
 * int64, center fp32 x2, owning object index int64 into center [B,n_objects,2]) -> heatmap and
 * affinity_weight [B,n_keypoints,H,W] (Gaussians of heatmap_sigma / affinity_sigma, max), affinity
 * [B,n_keypoints,2,H,W] (unit displacement from the owning object's center to each cell, of the
 * instance nearest to that cell; the earliest instance wins ties); nan_to_num of all three. */
int tv_train_keypoint_targets(const uint8_t* keypoint_valid, const int64_t* keypoint_label,
                              const float* keypoint_center, const int64_t* keypoint_object_index, const float* center,
                              int32_t B, int32_t n_instances, int32_t n_objects, int32_t n_keypoints, int32_t in_h,
                              int32_t in_w, int32_t downsample_ratio, double heatmap_sigma, double affinity_sigma,
                              float* heatmap, float* affinity_weight, float* affinity, void* stream);

/* The CenterNet training loss (loss.py:178-390) with its gradients, in three launches on `stream`:
 * dense, objects, finalize, in that order. Device pointers; fp32 arithmetic; no host synchronisation;
 * no float atomics and no waiting between workgroups, so two calls on the same inputs give the same bits.
 *
 * One description serves the three calls. tensor[i] is prediction tensor i (TV_LOSS_*): `data` in
 * `dtype` (TV_F32 / TV_F16 / TV_BF16, the same for all) with element strides `stride`, and `grad`, a
 * buffer of the same dtype and shape with element strides `grad_stride` that receives the gradient.
 * The stride order is [b, c, y, x] for the heatmaps ([B, n_labels | n_keypoints, H, W]),
 * [b, k, 2, y, x] for the affinity and [b, y, x, c] for the object heads ([B, H, W, 2 | 4 | 1]); any
 * non-negative strides are taken (NCHW-contiguous, NHWC views, channel slices), nothing is copied.
 * data == NULL: the head is absent (heatmap, size and offset must be present; the affinity needs the
 * keypoint heatmap; an angle's bin and offset go together). grad == NULL for every tensor: values only.
 * H = in_h / downsample_ratio, W = in_w / downsample_ratio. Truth: valid u8 [B, n_objects], label int64
 * in [0, n_labels), center / size fp32 [B, n_objects, 2], roll / pitch / yaw / depth fp32
 * [B, n_objects] (needed where the head is present), the keypoint instances as in
 * tv_train_keypoint_targets (needed with the keypoint heatmap). angle_range: fp32 [3, n_labels], the
 * modulo of roll, pitch, yaw per label (0 where the label has none: a NaN term, as in the reference).
 * bins: angle_get_bins(angle_bin_overlap) as (center, min, max) of bin 0 and bin 1.
 *
 * tv_centernet_loss_dense: every cell of every heatmap plane once. The cell's target is computed as
 *   tv_train_heatmap / tv_train_keypoint_targets compute it (sigma clamped to 0.1 for the object
 *   heatmap only) and never stored. Focal terms (loss.py:302-317): p = sigmoid(z), positive where
 *   isclose(target, 1), log(clamp(., 1e-4)) with the clamp's gradient 0 below the bound; affinity:
 *   weight * (pred - target)^2. Writes d(-(loss_p + loss_n)) / dz and 2 weight (pred - target), not
 *   yet scaled, to the gradients, zero-fills the object heads' gradients, and stores each workgroup's
 *   sums (positive, negative, squared error, positive count) to `workspace`. 8- or 16-byte vector
 *   accesses where all dense tensors and gradients are contiguous in (y, x) and aligned to four
 *   elements. focal alpha, beta >= 1 (below 1 the reference's 0 * inf at saturated cells is not kept).
 * tv_centernet_loss_objects: one thread per sample walks its objects in order: gathers every object
 *   head at out_index_for_position(center), forms the size / offset L1, angle_loss and depth_loss
 *   terms and stores their gradients, already scaled by lambda / n_valid with
 *   n_valid = min(valid count, 1) (angles: times the valid count, over all objects, as the reference
 *   has it), over the zero-filled gradients; the gradients of objects that share a cell are summed in
 *   fp32 in object order and stored once. Must follow tv_centernet_loss_dense on the stream. Per-sample sums go to `workspace`.
 * tv_centernet_loss_finalize: one workgroup sums the partial sums in a fixed order and writes
 *   out[0..15]: total (= heatmap + every other term, added in the reference's order), keypoint_heatmap,
 *   keypoint_affinity, offset, size, roll, pitch, yaw, depth, avg_size_error, max_size_error, the
 *   heatmap term alone, N of the heatmap, N of the keypoint heatmap, the valid count, 0;
 *   out[16..31]: the factor that scales tensor i's stored gradient (1 / N or 0 when N == 0 for the
 *   heatmap, lambda / N for the keypoint heatmap, lambda for the affinity, 1 for the object heads).
 * TV_EINVAL before any launch: null desc / workspace / out, a null pointer for a present head's truth,
 * B < 1, an empty map, negative strides, a missing required head, an unknown dtype, or a workspace
 * smaller than tv_centernet_loss_workspace_size. */
enum { TV_LOSS_HEATMAP = 0, TV_LOSS_KEYPOINT_HEATMAP, TV_LOSS_KEYPOINT_AFFINITY, TV_LOSS_SIZE, TV_LOSS_OFFSET,
       TV_LOSS_ROLL_BIN, TV_LOSS_ROLL_OFFSET, TV_LOSS_PITCH_BIN, TV_LOSS_PITCH_OFFSET, TV_LOSS_YAW_BIN,
       TV_LOSS_YAW_OFFSET, TV_LOSS_DEPTH, TV_LOSS_TENSORS };
typedef struct tv_loss_tensor {
  const void* data;
  void* grad;
  int64_t stride[5];
  int64_t grad_stride[5];
} tv_loss_tensor;
typedef struct tv_loss_desc {
  int32_t dtype, B, n_objects, n_instances, n_labels, n_keypoints, in_h, in_w, downsample_ratio;
  double keypoint_heatmap_sigma, keypoint_affinity_sigma, focal_alpha, focal_beta;
  double lambda_keypoint_heatmap, lambda_keypoint_affinity, lambda_size, lambda_offset, lambda_angle, lambda_depth;
  double bins[2][3];
  tv_loss_tensor tensor[TV_LOSS_TENSORS];
  const uint8_t* valid;
  const int64_t* label;
  const float *center, *size, *roll, *pitch, *yaw, *depth;
  const uint8_t* keypoint_valid;
  const int64_t *keypoint_label, *keypoint_object_index;
  const float* keypoint_center;
  const float* angle_range;
} tv_loss_desc;
int tv_centernet_loss_workspace_size(const tv_loss_desc* desc, int64_t* bytes);
int tv_centernet_loss_dense(const tv_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream);
int tv_centernet_loss_objects(const tv_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream);
int tv_centernet_loss_finalize(const tv_loss_desc* desc, const void* workspace, int64_t workspace_bytes, float* out,
                               void* stream);
/* The backward pass of the loss: grad[i] *= *scale for the n elements of one dense gradient buffer of `dtype`
 * that tv_centernet_loss_dense / _objects wrote (16-byte aligned). `scale` is a device fp32 scalar
 * ((gradient of total + gradient of the tensor's term) * the tensor's factor from out[16..]); the product
 * is formed in fp32 and rounded once. One pass, no recomputation. TV_EINVAL: null or misaligned pointers,
 * n < 0, an unknown dtype. */
int tv_centernet_loss_scale(void* grad, int32_t dtype, int64_t n, const float* scale, void* stream);

/* The YOLACT training loss (yolact/model/loss.py:8-124) with its gradients, in seven launches on `stream`
 * whatever B, T and the number of positive anchors. One description serves every call. Calls, in order:
 * tv_yolact_loss_match: per (sample, anchor) iou_matrix (boxes.py:64-85, the same fp32 operation
 *   sequence, no contraction) times truth_valid, the max over T (lowest truth index wins ties), positive =
 *   iou >= iou_pos_threshold, negative = iou <= iou_neg_threshold (a NaN IoU is neither) into match_index /
 *   positive / negative, and the background softmax probability, the mining key, into `workspace`.
 * tv_yolact_loss_select: per sample the positives in anchor order into a list, k = min(
 *   negative_example_ratio * n_positive, n_negative), the exact k negatives of smallest background
 *   probability (lowest anchor index wins ties); selected = positive | mined.
 * tv_yolact_loss_anchors: cross-entropy (log-softmax) at the selected anchors against the matched truth's
 *   class at positives and 0 elsewhere; smooth-L1 (beta 1) of box_encoding against box_encode(
 *   truth_box[match], anchor) (boxes.py:45-52) at positives. Writes softmax - onehot / the smooth-L1
 *   derivative into the gradient buffers, zeros elsewhere, and the zero rows of d mask_coeff.
 * tv_yolact_loss_mask_sums: per (sample, truth index t) the sum of (truth_seg_map == t) resized to h x w by
 *   upsample_bilinear2d (align_corners false).
 * tv_yolact_loss_mask: per positive, sigmoid(sum_p coeff_p proto_p) clamped to [1e-4, 1 - 1e-4], BCE against
 *   the resized truth mask (clamped alike), weighted by box_to_mask(truth_box[match]) (boxes.py:88-103) times
 *   truth_img_valid resized by upsample_nearest2d, divided by the resized mask's sum; positives whose sum
 *   is 0 are skipped. Writes d mask_prototype (every element once).
 * tv_yolact_loss_mask_coeff: the positives' rows of d mask_coeff. Needs gradient buffers (else TV_EINVAL).
 * tv_yolact_loss_finalize: out[0..3] = total, classification, box, mask (each sum divided by (1 + ratio) *
 *   n_positive resp. n_positive over the batch, or left as it is without a positive); out[4..6] = the
 *   batch's positive, negative and selected counts; out[8..11] = the factor that scales the stored gradient
 *   of classification, box_encoding, mask_coeff, mask_prototype; the rest of out[0..15] is 0.
 * Prediction tensors are fp32 with element strides (classification [B,A,C], box_encoding [B,A,4],
 * mask_coeff [B,A,P], anchor [A,4], mask_prototype [B,P,h,w]); the gradient buffers (all four or none) have
 * strides of their own and receive unscaled gradients (tv_centernet_loss_scale applies the factors). The
 * truth is contiguous: truth_valid u8 [B,T], truth_classification int64 [B,T] (in [0, C) where valid:
 * the caller checks), truth_box fp32 [B,T,4], truth_seg_map [B,in_h,in_w] of seg_itemsize bytes (1: uint8;
 * 2, 4, 8: signed), truth_img_valid u8 [B,in_h,in_w]. match_index int32 [B,A], positive / negative /
 * selected u8 [B,A] are outputs.
 * TV_EINVAL before any launch, with nothing written: a null description, pointer or workspace, B, A, C, P
 * or T < 1, an empty grid, negative_example_ratio < 0, a negative stride, some but not all gradient
 * buffers, or a workspace smaller than tv_yolact_loss_workspace_size. */
typedef struct tv_yolact_loss_desc {
  int32_t B, A, C, P, T, h, w, in_h, in_w, seg_itemsize, negative_example_ratio, reserved;
  double iou_pos_threshold, iou_neg_threshold, box_variances[2];
  const void *classification, *box_encoding, *mask_coeff, *anchor, *mask_prototype;
  void *grad_classification, *grad_box_encoding, *grad_mask_coeff, *grad_mask_prototype;
  const uint8_t* truth_valid;
  const int64_t* truth_classification;
  const float* truth_box;
  const void* truth_seg_map;
  const uint8_t* truth_img_valid;
  int32_t* match_index;
  uint8_t *positive, *negative, *selected;
  int64_t classification_stride[3], box_encoding_stride[3], mask_coeff_stride[3], anchor_stride[2];
  int64_t mask_prototype_stride[4];
  int64_t grad_classification_stride[3], grad_box_encoding_stride[3], grad_mask_coeff_stride[3];
  int64_t grad_mask_prototype_stride[4];
} tv_yolact_loss_desc;
int tv_yolact_loss_workspace_size(const tv_yolact_loss_desc* desc, int64_t* bytes);
int tv_yolact_loss_match(const tv_yolact_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream);
int tv_yolact_loss_select(const tv_yolact_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream);
int tv_yolact_loss_anchors(const tv_yolact_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream);
int tv_yolact_loss_mask_sums(const tv_yolact_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream);
int tv_yolact_loss_mask(const tv_yolact_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream);
int tv_yolact_loss_mask_coeff(const tv_yolact_loss_desc* desc, void* workspace, int64_t workspace_bytes, void* stream);
int tv_yolact_loss_finalize(const tv_yolact_loss_desc* desc, void* workspace, int64_t workspace_bytes, float* out,
                            void* stream);

/* Diagnostics (GPU tests): one DeformConv2d(x, offset, sigmoid(mask)) (DeformConv.forward,
 * centerpoint_dla.py:389-391: 3x3, stride 1, pad 1) + bias + activation (0 none, 1 ReLU, 2 leaky)
 * through the kernel the engine uses for DLA-34's DeformConv layers. x: compute-dtype NHWC
 * [B,H,W,C]; om: compute-dtype NHWC [B,H,W,om_ldc] = (dy, dx) per tap (18) + 9 mask logits (the
 * engine's fused offset/mask conv output); weight: host fp32 [N][C][3][3], bias host fp32 [N];
 * out: compute-dtype NHWC [B,H,W,N]. variant: 0 = fused dcn_gemm (32-channel k-steps),
 * 1 = fused dcn_gemm64 (tile by size), 2 = dcn_gemm64 with 64-pixel tiles, 3 = unfused sampling +
 * implicit GEMM (the fp32 path; the only variant for TV_F32), 4 = dcn_win (the LDS-window kernel the
 * engine uses for C == N == 64; TV_EINVAL otherwise), 5 = dcn_gemm64d (gathers two k-steps ahead),
 * 6 / 7 / 8 = dcn_gemm64 on 64-pixel tiles with split-K over 3 / 4 / 9 tap ranges (the engine's
 * small-batch form). Synchronous; allocates. */
int tv_diag_dcn_conv(const void* x, const void* om, int32_t B, int32_t H, int32_t W, int32_t C, int32_t om_ldc,
                     const float* weight, const float* bias, int32_t N, int32_t act, int32_t dtype, int32_t variant,
                     void* out, void* stream);

/* Diagnostics (GPU tests): a Root-style 1x1 conv (dla.py:58-76: Conv2d(sum C, N, 1) over
 * torch.cat(children, 1) + bias + activation) through conv1x1_stream, the kernel the engine runs for
 * stride-1 1x1 layers. src[k]: compute-dtype [M][ldc[k]] pixel rows of segment k (C[k] channels,
 * a multiple of 64); weight: host fp32 [N][sum C] in segment order; bias: host fp32 [N]; out:
 * compute-dtype [M][out_ldc], N channels (N a multiple of 8, <= 512). TV_F16 / TV_BF16 only.
 * Synchronous; allocates. Returns TV_EINVAL for shapes the kernel does not take. */
int tv_diag_conv1x1(const void* const* src, const int32_t* C, const int32_t* ldc, int32_t nseg, int32_t M,
                    const float* weight, const float* bias, int32_t N, int32_t act, int32_t dtype, void* out,
                    int32_t out_ldc, void* stream);

/* Diagnostics (GPU tests): one conv over nseg concatenated-K segments through conv_burst, the
 * engine's one-shot kernel for the small pyramid levels (Tree convs with the fused 1x1
 * conv_residual dla.py:8-52, Roots dla.py:58-76, IDAUp convs dla.py:212-284). Segment k:
 * src[k] compute-dtype NHWC [B, H, W, ldc] with geom[6k..6k+5] = H, W, C, ldc, kernel (1 or 3,
 * padding kernel / 2), stride; a 3x3 segment must be stride 1 over the output grid. weight: host
 * fp32 [N][K] (K segment-major, tap-major, channel-minor), bias: host fp32 [N]; out: compute-dtype
 * [B, Ho, Wo, out_ldc]. TV_F16 / TV_BF16; TV_EINVAL for layers the kernel does not take.
 * Synchronous; allocates. */
int tv_diag_conv_burst(const void* const* src, const int32_t* geom, int32_t nseg, int32_t B, int32_t Ho, int32_t Wo,
                       const float* weight, const float* bias, int32_t N, int32_t act, int32_t dtype, void* out,
                       int32_t out_ldc, void* stream);

/* Diagnostics (host only, no GPU needed): conv_burst's launch plan for a layer geometry (geom as
 * tv_diag_conv_burst, N output channels). out[0] = 1 when the kernel takes the layer, out[1] its
 * dynamic LDS bytes, out[2] the end of the highest LDS byte any of its accesses touches over every
 * tile position (the kernel's own index arithmetic; <= out[1], else the plan refuses the layer),
 * out[3] the LDS the layer's staging would need. */
int tv_diag_burst_plan(const int32_t* geom, int32_t nseg, int32_t B, int32_t Ho, int32_t Wo, int32_t N, int32_t* out);

/* Diagnostics (host only, no GPU needed): op `op` of the model's plan as tv_engine_create would
 * upload it: BatchNorm folded, packed [Npad][Kpad] in the compute dtype. desc / weights as
 * tv_engine_create, knobs as tv_engine_create_diag (NULL: none); the engine is configured for 256
 * compute units. info = {ops in the plan, the op's kind, Npad, Kpad, its segment count} (info[0] is
 * set even when `op` is out of range: TV_EINVAL); label: the op's label (NULL: skipped); segs[i], for
 * the first seg_cap segments = {kernel height, kernel width (a row-expanded source: its taps per
 * pixel), the source's stored channels, ci0, cin, k-steps}; size = the bytes of the weight, the fp32
 * bias and the extra buffer: the convt3 fragments of a whole ConvTranspose2d, or the fused 1x1
 * heads' fragments followed by their fp32 bias and the int32 head_row0[16], head_nrows[16]. A
 * non-NULL weight / bias / extra is filled when its cap[] equals that size. An op without weights
 * reports zeros. TV_ENOTFOUND: a state_dict key is missing or has the wrong element count. */
int tv_diag_pack_op(const tv_model_desc* desc, const tv_weight_view* weights, int32_t n_weights, const char* knobs,
                    int32_t op, int32_t info[5], char* label, int32_t label_cap, int32_t (*segs)[6], int32_t seg_cap,
                    int64_t size[3], void* weight, void* bias, void* extra, const int64_t cap[3]);

/* Diagnostics (GPU tests): one narrow-channel Conv2d(C, N, 3, stride, padding 1) + bias + activation
 * (DLA-34's full-resolution base levels, centerpoint_dla.py:242-246 `_make_conv_level`) through
 * conv_small, the engine's kernel for them: C -> N in {16 -> 16, 16 -> 32, 32 -> 32 (stride 1),
 * 32 -> 64 (stride 2)}. src: compute-dtype NHWC [B, H, W, ldc]; weight: host fp32 [N][C][3][3];
 * bias: host fp32 [N]; out: compute-dtype NHWC [B, Ho, Wo, out_ldc]. variant: 0 = per-lane register
 * gathers, 1 = LDS-halo tiles (a tile per workgroup), 2 = LDS-halo tiles on a persistent grid. TV_F16 / TV_BF16; TV_EINVAL for shapes the kernel does not take.
 * Synchronous; allocates. */
int tv_diag_conv_small(const void* src, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldc, const float* weight,
                       const float* bias, int32_t N, int32_t stride, int32_t act, int32_t dtype, int32_t variant,
                       void* out, int32_t out_ldc, void* stream);

/* Diagnostics (GPU tests): one ConvTranspose2d(C, N, 3, stride 2, padding 1, output_padding 1) +
 * bias + activation (YOLACT protonet up-sampling, masknet.py:21,33) through convt3, the engine's
 * kernel for it. src: compute-dtype NHWC [B, H, W, ldc], C channels (a multiple of 32); weight: host
 * fp32 [C][N][3][3] (nn.ConvTranspose2d layout), N a multiple of 64; bias: host fp32 [N]; out:
 * compute-dtype NHWC [B, 2H, 2W, out_ldc]. tile_w x tile_h: the input tile (<= 256 pixels, halo
 * (tile_w + 1)(tile_h + 1) <= 307), 0 = the kernel's choice. TV_F16 / TV_BF16; TV_EINVAL for shapes
 * the kernel does not take. Synchronous; allocates. */
int tv_diag_convt3(const void* src, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldc, const float* weight,
                   const float* bias, int32_t N, int32_t act, int32_t dtype, int32_t tile_w, int32_t tile_h, void* out,
                   int32_t out_ldc, void* stream);

/* Test-only: one ConvTranspose2d(128, 128, s, stride s) + pad_to_match + skip add through convt.hip (the
 * IDAUp / IDAUpReverse up-step), also at targets no plan reaches (larger than the up-sampled map). src:
 * compute-dtype NHWC [B, h, w, src_ldc]; weight: host fp32 [128][128][s][s] (nn.ConvTranspose2d layout);
 * bias: host fp32 [128]; add (the skip tensor) [B, tH, tW, add_ldc]; out [B, tH, tW, out_ldc], which may be
 * add. Input pixel (iy, ix) writes the target pixels (iy s + py + sy, ix s + px + sx) that lie inside the
 * target; every other pixel of out keeps its value. cus: the CU count the launch is scheduled for (0 = the
 * device's); *np (may be null): the phases per workgroup that schedule chose, the kernel instance
 * convt_add<T, np>. 1 <= s <= 16, sy, sx >= 0, ldc >= 128 in whole 16-byte chunks, TV_F16 / TV_BF16, else
 * TV_EINVAL. Synchronous; allocates. */
int tv_diag_convt_add(const void* src, int32_t B, int32_t h, int32_t w, int32_t src_ldc, const float* weight,
                      const float* bias, int32_t s, const void* add, int32_t add_ldc, void* out, int32_t out_ldc,
                      int32_t tH, int32_t tW, int32_t sy, int32_t sx, int32_t dtype, int32_t cus, int32_t* np,
                      void* stream);

/* Diagnostics (GPU tests): the FeaturePyramid's top-down step (feature_pyramid.py:49-50) through
 * bilinear_add, the engine's kernel for it: dst += F.interpolate(src, (dst_h, dst_w), mode="bilinear")
 * (align_corners=False: source coordinate max(0, (d + 0.5) in / out - 0.5), second tap clamped to
 * in - 1; any per-axis ratio), in place. src: compute-dtype NHWC [B, src_h, src_w, src_ldc], dst:
 * compute-dtype NHWC [B, dst_h, dst_w, dst_ldc], C channels of each (C and both pixel strides whole
 * 16-byte vectors, else TV_EINVAL). Async on `stream`; allocates nothing. */
int tv_diag_bilinear_add(const void* src, int32_t B, int32_t src_h, int32_t src_w, int32_t src_ldc, void* dst,
                         int32_t dst_h, int32_t dst_w, int32_t dst_ldc, int32_t C, int32_t dtype, void* stream);

/* Diagnostics (GPU tests): the ResNet-18 backbone's bandwidth kernels (resnet.hip) on their own.
 * Compute-dtype NHWC device tensors, C channels in whole 16-byte vectors (else TV_EINVAL). Async on
 * `stream`; allocate nothing.
 * tv_diag_maxpool3x3s2: MaxPool2d(3, 2, 1) (floor mode; taps outside the image are ignored):
 *   src [B, H, W, C] -> out [B, (H - 1) / 2 + 1, (W - 1) / 2 + 1, C].
 * tv_diag_add_relu: out = relu(a + b), one rounding, over n elements (a multiple of the vector). */
int tv_diag_maxpool3x3s2(const void* src, int32_t B, int32_t H, int32_t W, int32_t C, void* out, int32_t dtype,
                         void* stream);
int tv_diag_add_relu(const void* a, const void* b, void* out, int64_t n, int32_t dtype, void* stream);

/* Diagnostics (GPU tests): CenterpointDLA34's bandwidth kernels (dla34.hip) on their own. Compute-dtype
 * NHWC device tensors, C channels in whole 16-byte chunks (else TV_EINVAL, nothing written). Async on
 * `stream`; allocate nothing.
 * tv_diag_maxpool2: MaxPool2d(2, 2, ceil_mode=True): src [B, H, W, C] -> out [B, (H + 1) / 2, (W + 1) / 2, C].
 * tv_diag_dwconvt_add: out = pad_to_match(ConvTranspose2d(C, C, 2f, stride f, padding f / 2, groups = C,
 *   no bias)(src)) + add (IDAUp.forward, centerpoint_dla.py:453-460). src [B, h, w, C]; weight: device
 *   fp32 [2f][2f][C] (tap-major, channel-minor); add [B, tH, tW, add_ldc] (add_ldc >= C, whole chunks);
 *   out [B, tH, tW, C], no alias of src or add. Target pixel (y, x) reads the up-sampled map at
 *   (y - sy, x - sx), zero outside it; sy, sx >= 0 (else TV_EINVAL). f = 2, 4, 8 on a power-of-two
 *   chunk count take the shift-and-mask kernel, everything else the generic one. */
int tv_diag_maxpool2(const void* src, int32_t B, int32_t H, int32_t W, int32_t C, void* out, int32_t dtype,
                     void* stream);
int tv_diag_dwconvt_add(const void* src, int32_t B, int32_t h, int32_t w, int32_t C, const float* weight, int32_t f,
                        const void* add, int32_t add_ldc, void* out, int32_t tH, int32_t tW, int32_t sy, int32_t sx,
                        int32_t dtype, void* stream);

const char* tv_last_error(void);
const char* tv_version(void);

#ifdef __cplusplus
}
#endif
#endif

/* davo_hip.h — C ABI of libdavo_hip.so: DAVO frame-to-frame pose inference on MI355X (gfx950).
 *
 * The reference (BassyKuo/DAVO, TensorFlow 1.13) has no plugin/FFI layer: this path sits
 * behind the Python class DAVO (reference davo.py:30).  Each entry point below names the
 * reference interface it stands in for; davo_amd/davo.py is the ctypes host side that keeps
 * the reference's call surface on top of it.  Plain pointers and sizes only — no torch, no
 * TF types.  A context is NOT thread-safe: one context per GPU per host thread (the reference
 * drives sess.run from a single thread, test_kitti_pose.py:133-145).
 *
 * Every function returns 0 on success and a negative davo_status on failure; the message is
 * available from davo_last_error().  Tensor layouts are the reference's: NHWC, float32 unless
 * stated, HWIO convolution kernels, [in,out] dense kernels.
 */
#ifndef DAVO_HIP_H
#define DAVO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct davo_ctx davo_ctx;

typedef enum {
    DAVO_OK = 0,
    DAVO_ERR_INVALID = -1,      /* bad argument / shape / unsupported variant */
    DAVO_ERR_HIP = -2,          /* a HIP runtime call failed                   */
    DAVO_ERR_NOT_READY = -3,    /* forward before every weight was loaded      */
    DAVO_ERR_NOMEM = -4,
    DAVO_ERR_RANGE = -5,        /* f16x3: a layer's activations left the fp16-pair storage range */
    DAVO_ERR_COMM = -6          /* librccl could not be loaded, or an RCCL call failed           */
} davo_status;

/* What the reference derives from the --version string (davo.py:1010-1102,1117-1450);
 * davo_amd/version.py:parse_version() fills it.  Field order is ABI. */
typedef struct {
    int32_t cin_per_frame;  /* 5: rgb+flow ("v1", davo.py:1062-1065) | 3: rgb only ("v0")        */
    int32_t cnv6_out;       /* -cnv6_(\d+), default 128 (davo.py:1052-1053); multiple of 32       */
    int32_t se_act;         /* 0 relu | 1 tanh | 2 leaky_relu(0.2)   (davo.py:1077-1085)          */
    int32_t norm_flow;      /* (f-0.32140523)/15.384229 on the SE input (davo.py:1089-1091)       */
    int32_t abs_mode;       /* 0 none | 1 |f_x| | 2 |f_y| | 3 |f|      (davo.py:1094-1102)        */
    int32_t att_source;     /* 0 ones (-no_segmask) | 1 se_flow | 2 static, tgt=1 | 3 static, all  (davo.py:1385-1400)
                             * class tables, a per-frame SE descriptor -> dense -> dense -> sigmoid over 19 classes
                             * (davo.py:1274-1374; "tgt=1": target map ones, otherwise the target's own table):
                             *   4 -se_seg_wo_tgt               label histogram 19 -> 19 -> 19, tgt=1   (scope se_seg)
                             *   5 -se_rgb_wo_tgt_to_seg        rgb mean 3 -> 8 -> 19, tgt=1            (scope se_rgb)
                             *   6 -se_rgb_to_seg               rgb mean 3 -> 8 -> 19                   (scope se_rgb)
                             *   7 -se_SegFlow_to_seg_wo_tgt    histogram + flow mean 21 -> 19 -> 19, tgt=1 (scope se_segflow)
                             *   8 -se_SegFlow_to_seg           21 -> 19 -> 19                          (scope se_segflow)
                             *   9 -se_SegFlow_to_seg_8_wo_tgt  21 -> 8 -> 19, tgt=1                    (scope se_segflow)
                             *  10 -se_SegFlow_to_seg_8         21 -> 8 -> 19                           (scope se_segflow)
                             * depth class tables (davo.py:1109, 1211-1227): the descriptor of frame i is the mean of
                             * depth_i + depth_tgt (the reference's `list + tensor' broadcasts the target's depth onto every
                             * frame).  They read a fourth input, the depth planes: the `_depth' entry points below.
                             *  11 -se_depth_wo_tgt_to_seg      depth mean 1 -> 8 -> 19, tgt=1          (scope se_depth)
                             *  12 -se_depth_to_seg             depth mean 1 -> 8 -> 19                 (scope se_depth)
                             * depth-split flow attention (davo.py:1136-1155): se_flow's squeeze, two excitations on it, and per
                             * pixel of a source frame the near or the far table by depth < depth_threshold (float32, strict; a NaN
                             * depth is far); the target's map is ones.  It reads the depth planes too (`_depth' entry points):
                             *  13 -se_flow_on_depthseg_seplayers  flow mean 2 -> 8 -> 19 twice, tgt=1   (scopes se_flow_near,
                             *                                   se_flow_far; scalar pose_exp_net/se_flow/depth_threshold)
                             * pooled flow attention (davo.py:1181-1210; nets/attention_module.py:68-86, 137-167): se_flow's scope,
                             * transform and target map (ones); the descriptor is a grid of window means of the transformed flow
                             * (davo_pool_plan below), 2 values per cell, dense D -> nh -> 19:
                             *  14 -se_gp2x2_flow_nobottle      four quadrants, 8 -> 19 -> 19            (davo.py:1181-1186)
                             *  15 -se_spp21_flow               SPP levels [2, 1], 10 -> 8 -> 19          (:1193-1198)
                             *  16 -se_spp2_flow                SPP level [2], 8 -> 8 -> 19               (:1199-1204)
                             *  17 -se_spp864_flow              SPP levels [8, 6, 4], 232 -> 8 -> 19      (:1205-1210) */
    int32_t mask_rgb;       /* rgb_k *= att_k                          (davo.py:1419-1423)        */
    int32_t mask_info;      /* flow_k *= att_k  (-segmask_all)         (davo.py:1430-1434)        */
} davo_variant;

/* Replaces DAVO(version).setup_inference(img_height, img_width, 'davo', 3, batch_size, ...)
 * (davo.py:1533-1551 -> build_pose_test_graph_davo, davo.py:955-1494): creates the device
 * context (workspace for up to max_batch triplets of H x W frames) on HIP device `device`.
 * H and W must be multiples of 4. */
int davo_create(davo_ctx** out, int device, int H, int W, int max_batch, const davo_variant* v);

/* The se_block inside the PoseNN (davo.py:1010-1017 -> nets/posenn.py:225-236), which is not part of davo_variant (its eight
 * fields are ABI).  mode 0 = none (the default), 1 = insert (`-se_insert', "Ours w/ feature attention"): inside the loop over
 * the heads `rotation', `translation' the reference re-binds cnv5 = se_block(cnv5, 'cnv5_se_attention', ratio=8) and convolves
 * that (nets/posenn.py:227-228; nets/attention_module.py:9-52: mean over (h, w), dense 256 -> 32 ReLU, dense 32 -> 256 sigmoid,
 * x * s), so rotation/cnv6 reads cnv5 * s_r and translation/cnv6 reads (cnv5 * s_r) * s_t with s_t computed from the ALREADY
 * scaled tensor.  The variant gains the variables pose_exp_net/pose/{rotation,translation}/cnv5_se_attention/
 * {bottleneck_fc,recover_fc}/{kernel,bias}: (256,32), (32,), (32,256), (256,).  Valid with att_source 0 (`-no_segmask', the
 * published combination) only, and only before the first davo_load_weight and the first forward (it changes the set of
 * variables, cnv6's weight layout and the workspace): afterwards DAVO_ERR_INVALID.  Inputs and every other entry point are
 * unchanged; `-se_skipadd' and `-se_replace' are not built. */
int davo_set_posenn_se(davo_ctx* ctx, int mode);

/* The PoseNN's topology (davo.py:1027-1049), which is not part of davo_variant either.  DAVO_POSENN_PAIRS (the default) is
 * `-sharedNN-dilatedPoseNN', decouple_sharednet_v0_dilation: two (tgt, src) images per window through shared weights.
 * DAVO_POSENN_TRIPLET is `-dilatedPoseNN' without `-sharedNN', decouple_net_v0_dilation (nets/posenn.py:69-131): ONE image
 * concat(tgt, src0, src1) per window, one pass through cnv1..cnv7, and a pred of 3 * 2 outputs per head:
 *   pose[b][s][3 * head + k] = 0.01 * mean(pred_head)[b][3 * s + k],  s = 0 for tgt->src0, 1 for tgt->src1, head 0 = rotation.
 * The variables keep their names; pose_exp_net/cnv1/weights becomes (7,7,3 * cin_per_frame,16), each head's pred/weights
 * (1,1,256,6) and pred/biases (6,).  Inputs, their layouts and the [B,2,6] output are unchanged, and every pose entry point
 * works as before in both label and both flow formats (davo_forward, davo_forward_device, davo_submit / davo_wait,
 * davo_calibrate, the three `_frames' calls), with the same range recovery.  The masking is davo.py:1415-1450's: with v1 the
 * network reads tgt rgb*att_t | 0 0 | src0 rgb*att_0 | flow0*att_0 | src1 rgb*att_1 | flow1*att_1.  On the device the two zero
 * channels are dropped and the packed tensor has 16 channels per pixel, in this order:
 *   tgt rgb (3) | src0 rgb (3) | flow0 (2) | src1 rgb (3) | flow1 (2) | 0 0 0      (v0: the flow slots are zero)
 * davo_debug_read sizes "packed" as [B,H,W,16] and "cnv1".."cnv7" by B images.
 * Valid only before the first davo_load_weight and the first forward, like davo_set_posenn_se: afterwards DAVO_ERR_INVALID.
 * DAVO_ERR_INVALID as well on a context whose att_source is 11..13 (the depth sources have no three-frame form), after
 * davo_set_posenn_se(ctx, 1), after davo_set_pairs with anything but DAVO_PAIRS_BOTH, with impl 1 set or an export switched on.
 * On a triplet context davo_set_pairs accepts DAVO_PAIRS_BOTH only (one pass yields both poses), davo_set_impl(ctx, 1),
 * davo_set_posenn_se(ctx, 1), davo_set_feature_export(ctx, 1) and davo_set_heat_export(ctx, 1) return DAVO_ERR_INVALID (the
 * exports of the three-frame network are a follow-up), cnv7 is stored and the pose head runs as two launches: the option
 * "fuse_pose" 1 is accepted and has no effect (a six-column fused epilogue is a follow-up).  cnv1 runs on an LDS-patch kernel of
 * its own or on the implicit GEMM at 16 input channels: option "patch_cnv1_t" below. */
enum { DAVO_POSENN_PAIRS = 0, DAVO_POSENN_TRIPLET = 1 };
int davo_set_posenn_topology(davo_ctx* ctx, int topology);

/* The PoseNN's heads (davo.py:1027-1049), not part of davo_variant either.  DAVO_POSENN_HEADS_DECOUPLED (the default) is the
 * rotation head and the translation head of the two decoupled networks.  DAVO_POSENN_HEADS_COUPLED is
 * `-sharedNN-dilatedCouplePoseNN', couple_sharednet_v0_dilation (nets/posenn.py:133-187): the pair network's trunk cnv1..cnv5, then
 * ONE cnv6 (3x3, rate 2, 256 -> cnv6_out), ONE cnv7 (3x3, stride 2, reading ALL cnv6_out channels -> 256) and one linear pred of
 * six columns per pair image n:
 *   pose[pair_pose_row(n)][k] = 0.01 * mean_{H3,W3}(pred)[n][k],  k = 0..5 unpermuted (rz ry rx tx ty tz).
 * The trunk's variables keep their names; the head's are pose_exp_net/pose/{cnv6,cnv7,pred}/{weights,biases}: (3,3,256,cnv6_out),
 * (cnv6_out,), (3,3,cnv6_out,256), (256,), (1,1,256,6), (6,) - there is no rotation/ or translation/ scope, and the variables of
 * those scopes are refused ("not part of this variant"), as the coupled names are on a decoupled context.
 * Inputs, their layouts, the [B,2,6] output and everything in front of cnv6 are unchanged: every attention source, both label, flow
 * and depth formats, davo_set_flip, davo_set_pairs (one selected pair still writes +0.0 into the other row), davo_set_impl(ctx, 1)
 * and every pose entry point (window, `_depth', device, davo_submit / davo_wait, davo_calibrate, the three `_frames' calls) work as
 * on the flagship, with the same range recovery.  davo_debug_read sizes "cnv6" as [images,H/4,W/4,cnv6_out] and "cnv7" as
 * [images,H/8,W/8,256].
 * Valid only before the first davo_load_weight and the first forward, like its two neighbours: afterwards DAVO_ERR_INVALID.
 * DAVO_ERR_INVALID as well for a value outside {0, 1}, after davo_set_posenn_topology(ctx, DAVO_POSENN_TRIPLET) (the three-frame
 * coupled network, couple_net_v0_dilation, is not built), after davo_set_posenn_se(ctx, 1) (the block has no coupled form) and
 * while a feature or heat export is on (the reference returns (cnv6, cnv6) there; not built).  Symmetrically, on a coupled context
 * davo_set_posenn_topology(ctx, DAVO_POSENN_TRIPLET), davo_set_posenn_se(ctx, 1), davo_set_feature_export(ctx, 1) and
 * davo_set_heat_export(ctx, 1) return DAVO_ERR_INVALID.
 * The pose head.  f16x3 with the option "fuse_pose" 1 (the default), on maps of at least 128 cnv7 pixels per image: the six columns
 * are fused into cnv7's epilogue like the flagship's three per head (the six-column instantiation of that epilogue; cnv7 is not
 * stored, davo_debug_read("cnv7") returns DAVO_ERR_NOT_READY, "fold_tails" 1 lets the launch's last workgroup write the poses).
 * float32 mode, smaller maps and "fuse_pose" 0 keep the two-pass head (pose_head_partial over the stored cnv7, then a fixed-order
 * finish): a six-column fused epilogue is not built for float32 mode. */
enum { DAVO_POSENN_HEADS_DECOUPLED = 0, DAVO_POSENN_HEADS_COUPLED = 1 };
int davo_set_posenn_heads(davo_ctx* ctx, int heads);

/* Label format.  A label map is a class id per pixel, and nothing on the path reads more of it than "class 0..18, or none"; the
 * reference's preprocessing stores it as float32 [B,3,H,W,1] (data_loader.py:313-317), which is what every entry point takes by
 * default (DAVO_LABELS_F32).  davo_set_label_format(ctx, DAVO_LABELS_U8) makes the context take bytes instead: uint8 [B,3,H,W,1],
 * same plane order (src0, tgt, src1).  A byte L < 19 selects class L; 19..255 select no class (Cityscapes' ignore label 255 among
 * them).  The float32 rule folded into a byte - a finite value in (-1, 19) becomes its truncation toward zero, anything else 255
 * (davo_amd.labels_to_u8) - selects the same class for every pixel, so poses, layer tensors and exports are bit-identical to the
 * float32 context's on the converted maps.  The kernels read the bytes natively (no widening pass, no float copy on the device).
 * On a DAVO_LABELS_U8 context the `seg' / `d_seg' argument of EVERY entry point below points at bytes (a C caller casts the
 * pointer): davo_forward, davo_forward_device, davo_submit, davo_calibrate, their `_depth' forms, davo_forward_features and
 * davo_forward_heat; and everything the context sizes by a window's label maps follows - the host entry points' copies (3 H W
 * bytes per window instead of 12 H W: a 128x416 window is 1,437,696 B across the link instead of 1,757,184), the staging sets of
 * the streaming slots, the range guard's input snapshots and its re-issues.  Device label maps must be 16-byte aligned in either
 * format (every kernel then loads a 4-pixel unit of labels with one aligned load: H W is a multiple of 16).  A `-no_segmask'
 * context accepts the call and reads no label byte.  The depth planes have a format of their own (davo_set_depth_format).
 * Like davo_set_posenn_se this is called right after davo_create: once any call has taken inputs (or a staging set or the
 * snapshot ring exists) it returns DAVO_ERR_INVALID, and so does any other value of fmt.  davo_get_label_format reads it back. */
enum { DAVO_LABELS_F32 = 0, DAVO_LABELS_U8 = 1 };
int davo_set_label_format(davo_ctx* ctx, int fmt);
int davo_get_label_format(const davo_ctx* ctx);

/* Flow format.  The optical flow is what FlowNet2 estimates, to about a pixel; the reference's dump stores it as float32
 * [B,4,H,W,2] (24 significant bits), which is what every entry point takes by default (DAVO_FLOW_F32).
 * davo_set_flow_format(ctx, DAVO_FLOW_F16) makes the context take IEEE binary16 instead, in the same layout: 11 significant
 * bits, a rounding error of at most 2^-12 relative - under 0.004 px at 15 px; above 2048 px the spacing is 2 px and more.
 * davo_amd.flow_to_f16 is the one rule by which float32 flow becomes halves: round to nearest even, finite values beyond
 * +-65504 go to +-65504 (a finite flow stays finite), NaN stays NaN.  The kernels read the halves natively: a 4-pixel unit is
 * one aligned 16-byte load, widened value by value (exact for every binary16 value, subnormals, signed zeros and infinities
 * included; NaN stays NaN), and every float32 expression and summation order behind the widening is the float32 format's.  So
 * for any binary16 array h, a DAVO_FLOW_F16 context on h and a DAVO_FLOW_F32 context on (float)h give the same bits in every
 * tensor: attention tables, the packed input, cnv1..cnv7, poses, range records, feature and heat exports, in both precisions.
 * On a DAVO_FLOW_F16 context the `flow' / `d_flow' / `flow2' argument of EVERY entry point below points at halves (a C caller
 * casts the pointer): davo_forward, davo_forward_device, davo_submit, davo_calibrate, their `_depth' forms, the three `_frames'
 * forms ([N,2,H,W,2]), davo_forward_features and davo_forward_heat; and everything the context sizes by a window's flow follows -
 * the host entry points' copies and their sub-batching, the staging sets of the streaming slots, the frame layout's gather, the
 * range guard's input snapshots and its re-issues (as issued, re-calibrated or on the float32 kernels).  Device flow buffers
 * must be 16-byte aligned (DAVO_ERR_INVALID otherwise).  A variant that reads no flow (`v0' with a flow-free attention
 * source) accepts the call; every variant still takes the pointer.
 * Bytes across the link per window at 128x416, both pairs, byte labels: the window form sends 479,232 (strip) + 425,984 (two
 * binary16 flow planes; 851,968 as float32) + 106,496 (two label maps) = 1,011,712 instead of 1,437,696; the frame layout
 * 159,744 + 425,984 + 53,248 = 638,976 instead of 1,064,960 (40 % fewer).
 * The ordering rule is the label format's: called right after davo_create; once any call has taken inputs (or a staging set, a
 * frame buffer or the snapshot ring exists) it returns DAVO_ERR_INVALID, and so does any other value of fmt.  It is independent
 * of davo_set_label_format, davo_set_posenn_se and davo_set_pairs, in any order.  davo_get_flow_format reads it back. */
enum { DAVO_FLOW_F32 = 0, DAVO_FLOW_F16 = 1 };
int davo_set_flow_format(davo_ctx* ctx, int fmt);
int davo_get_flow_format(const davo_ctx* ctx);

/* Depth format.  The depth planes are a monocular network's estimate (monodepth2), good to a few percent; the reference's dump
 * stores them as float32 [B,3,H,W,1], which is what every entry point that takes depth takes by default (DAVO_DEPTH_F32).
 * davo_set_depth_format(ctx, DAVO_DEPTH_F16) makes the context take IEEE binary16 instead, in the same layout: a rounding error of
 * at most 2^-12 relative; at the depth-split attention's 15 m default threshold a half is 2^-7 m wide.  davo_amd.depth_to_f16 is
 * the one rule by which float32 depth becomes halves, and it is the flow's: round to nearest even, finite values beyond +-65504
 * go to +-65504, NaN, infinities and signed zeros are kept.  The kernels read the halves natively: a 4-pixel unit is one aligned
 * 8-byte load, widened value by value (exact for every binary16 value, subnormals, signed zeros and infinities included; NaN
 * stays NaN - and a NaN depth is far, as in the float32 format), and every float32 expression, comparison and summation order
 * behind the widening is the float32 format's.  So for any binary16 array h, a DAVO_DEPTH_F16 context on h and a DAVO_DEPTH_F32
 * context on (float)h give the same bits in every tensor, in both precisions.
 * On a DAVO_DEPTH_F16 context the `depth' / `d_depth' argument of EVERY entry point below points at halves (a C caller casts
 * the pointer): davo_forward_depth, davo_forward_device_depth, davo_submit_depth, davo_calibrate_depth, the three `_frames' forms
 * ([N+2,H,W,1]), davo_forward_features and davo_forward_heat; and everything the context sizes by a depth plane follows - the
 * host entry points' copies and their sub-batching, the staging sets and frame buffers of the streaming slots, the frame
 * layout's gather, the mirror of davo_set_flip, the range guard's input snapshots and its re-issues.  Device depth buffers are
 * 16-byte aligned, as in the float32 format.  A context whose variant reads no depth accepts the call and still ignores every
 * depth pointer.
 * Bytes across the link per window at 128x416, att_source 11, both pairs, byte labels, binary16 flow: the window form sends
 * 1,011,712 (strip, flow, label maps: above) + 319,488 (three binary16 depth planes; 638,976 as float32) = 1,331,200 instead of
 * 1,650,688; the frame layout, long batch, 638,976 + 106,496 = 745,472 instead of 851,968.
 * The ordering rule is the flow format's: called right after davo_create; once any call has taken inputs (or a staging set, a
 * frame buffer or the snapshot ring exists) it returns DAVO_ERR_INVALID, and so does any other value of fmt.  It is independent
 * of davo_set_label_format, davo_set_flow_format, davo_set_pairs and davo_set_flip, in any order.  davo_get_depth_format reads
 * it back. */
enum { DAVO_DEPTH_F32 = 0, DAVO_DEPTH_F16 = 1 };
int davo_set_depth_format(davo_ctx* ctx, int fmt);
int davo_get_depth_format(const davo_ctx* ctx);

/* Replaces tf.train.Saver(tf.trainable_variables()).restore(sess, ckpt)
 * (test_kitti_pose.py:129-131), one tensor at a time, keyed by the TF variable name
 * (e.g. "pose_exp_net/cnv1/weights", "pose_exp_net/pose/rotation/cnv6/biases",
 * "pose_exp_net/se_flow/bottleneck_fc/kernel", "pose_exp_net/se_segflow/recover_fc/bias").  `data` is a host pointer; the context keeps
 * its own (re-laid-out) device copy.  ndim = 0 (shape may be NULL) is a scalar variable: att_source 13's
 * "pose_exp_net/se_flow/depth_threshold", whose value the context keeps on the host and hands to its kernels as an argument. */
int davo_load_weight(davo_ctx* ctx, const char* tf_name, const float* data,
                     const int64_t* shape, int ndim);

/* Number of weight tensors the variant still needs (0 = ready); names of the missing ones are
 * left in davo_last_error(). */
int davo_weights_missing(davo_ctx* ctx);

/* Replaces DAVO.inference(sess, mode='pose') (davo.py:1553-1569 -> sess.run({'pose': pred_poses})).
 * Host pointers, shapes as the reference's test driver sets them (test_kitti_pose.py:110-114):
 *   img  uint8 [B,H,3W,3]  (strip src0|tgt|src1, data_loader.py:537-557)
 *   flow f32   [B,4,H,W,2] (planes 0,1 used, davo.py:978-982); binary16 [B,4,H,W,2] behind the same pointer type on a
 *              DAVO_FLOW_F16 context (davo_set_flow_format) - here and for every `flow' / `d_flow' / `flow2' argument below
 *   seg  f32   [B,3,H,W,1] (file order src0,tgt,src1, davo.py:998-1004); uint8 [B,3,H,W,1] behind the same pointer type on a
 *              DAVO_LABELS_U8 context (davo_set_label_format) - here and for every `seg' / `d_seg' argument below
 *   pose_out f32 [B,2,6]   rows = (tgt->src0, tgt->src1), each [rz,ry,rx,tx,ty,tz]
 * Synchronous: returns after pose_out is written.  1 <= B <= max_batch. */
int davo_forward(davo_ctx* ctx, int B, const uint8_t* img, const float* flow, const float* seg,
                 float* pose_out);

/* The depth sources (att_source 11, 12) and the depth-split flow attention (13) read a fourth input (davo.py:960, 991-996; test_kitti_pose.py:48, 91):
 *   depth f32  [B,3,H,W,1] (file order src0,tgt,src1 like the label maps; <dump>/SS/FFFFFF-monodepth2_depth.npy); binary16
 *              [B,3,H,W,1] behind the same pointer type on a DAVO_DEPTH_F16 context (davo_set_depth_format) - here and for
 *              every `depth' / `d_depth' argument below,
 * 16-byte aligned where it is a device pointer.  Each entry point that takes inputs has a `_depth' form with that argument
 * behind `seg'; everything said about the three-input form holds for it, the depth planes included: davo_forward_depth copies
 * them with each sub-batch, davo_submit_depth stages all three planes per slot (13 never reads the target's plane), the f16x3 range recovery keeps and re-issues them
 * with the batch.  On a context whose variant reads depth the three-input forms return DAVO_ERR_INVALID (the message names the
 * `_depth' form); on any other variant the `_depth' forms accept a depth pointer or NULL and ignore it.
 *   davo_forward_depth          davo_forward           + depth (host pointer)     DAVO.inference, davo.py:1553-1569
 *   davo_forward_device_depth   davo_forward_device    + d_depth (device pointer)
 *   davo_submit_depth           davo_submit            + depth (host pointer)     test_kitti_pose.py:133-145
 *   davo_calibrate_depth        davo_calibrate         + d_depth (device pointer) */
int davo_forward_depth(davo_ctx* ctx, int B, const uint8_t* img, const float* flow, const float* seg,
                       const float* depth, float* pose_out);
int davo_forward_device_depth(davo_ctx* ctx, int B, const void* d_img, const void* d_flow, const void* d_seg,
                              const void* d_depth, void* d_pose, float* elapsed_ms);
int davo_submit_depth(davo_ctx* ctx, int B, const uint8_t* img, const float* flow, const float* seg,
                      const float* depth, float* pose_out, int hold);
int davo_calibrate_depth(davo_ctx* ctx, int batch, const void* d_img, const void* d_flow, const void* d_seg,
                         const void* d_depth, int* shifts_out);

/* Same computation on device-resident buffers (the path bench.py times; multi-GPU shards keep
 * their windows in HBM).  Asynchronous on the context's stream unless elapsed_ms != NULL, in
 * which case it is bracketed by HIP events, synchronised, and the device time is returned.
 * With davo_set_inflight(ctx, n > 1) the timed form still waits for its own batch only and the
 * batches of all slots are judged together at davo_synchronize().
 * f16x3 range guard: the asynchronous form cannot know its own result, so every batch gets a slot of a ring of range
 * records (running maxima: "clamped" is exact per batch, "too small" covers what the slot has stored since its record was last
 * zeroed - at a failed verdict, a change of scales, and for every 256th batch) and is judged later: when its slot of a ring of 8 is needed again (eight batches on), at davo_synchronize(), or before
 * anything that changes the storage scales.  A failed verdict RE-ISSUES that batch (see "auto_range" below) and
 * rewrites its pose buffer, so:
 *   - the OUTPUT buffer of a batch must stay alive until davo_synchronize() has returned, and its poses are final only
 *     then (davo_range_stats / davo_range_report say whether anything was re-issued).  A pose buffer may be handed to a
 *     later batch before that (two alternating buffers; one buffer overwritten every step): the newest batch issued into a
 *     range of memory always wins - a re-issue writes into a buffer of the context first and is copied to the batch's own
 *     pose buffer only if no batch issued after it targets an overlapping range.  What such a caller cannot have is FINAL
 *     poses per batch before it synchronises (a D2H copy ordered on the stream behind batch n reads batch n's first issue):
 *     streaming callers use davo_submit / davo_wait below, where the library owns the pose buffers and delivers final poses;
 *   - the INPUT buffers (16-byte aligned) may be overwritten or recycled as soon as work ordered behind the call on
 *     the context's stream may run (e.g. the next H2D on that stream, or anything behind an event recorded there):
 *     the batch's last kernel sees the finished range record and, if the batch will have to be re-issued, copies
 *     the inputs it was issued on into buffers of the context (1.97 MB per 128x416 window, eight batches deep,
 *     allocated at the first such call); the re-issue reads that copy.  A batch in range - every batch of a
 *     well-ranged checkpoint - copies nothing.  A caller that keeps its inputs unchanged until davo_synchronize()
 *     anyway can save the buffers with davo_set_option(ctx, "stable_inputs", 1); re-issues then read the caller's.
 * The timed, synchronous form judges (and re-issues) its own batch; elapsed_ms is then the first issue's time. */
int davo_forward_device(davo_ctx* ctx, int B, const void* d_img, const void* d_flow,
                        const void* d_seg, void* d_pose, float* elapsed_ms);

/* The sequence loop as a stream.  The reference's driver pulls batches through tf.data's prefetch(8*B) while the session runs
 * (test_kitti_pose.py:133-145, data_loader.py:321-324), so input transfer, compute and result delivery of neighbouring batches
 * overlap; davo_forward returns poses and cannot.  davo_submit takes host pointers shaped as davo_forward's (seg: bytes on a
 * DAVO_LABELS_U8 context) and rotates through the
 * in-flight slots (davo_set_inflight) like davo_forward_device: on the slot's own stream it queues the H2D copies of the planes the
 * path reads into the slot's staging set, the forward, and the D2H of the poses into a page-locked ring entry of the context.  With
 * two or more slots the copies of batch n+1 run under the kernels of batch n (one slot: copy and kernels alternate, still without
 * the host waiting for either).  It returns once the input buffers of the batch submitted `hold` calls earlier have been copied:
 * hold = 0 - on return THIS batch's img / flow / seg may be overwritten (a loader that recycles a batch when the next one is
 * asked for); hold = k - the caller keeps a batch's inputs unchanged for k more submits and the call waits for a copy that is
 * probably done already (k >= 8 never waits for a copy and records no event).  Page-locked inputs (davo_host_alloc /
 * davo_host_register) copy as DMA; pageable ones work, synchronously.
 * pose_out [B,2,6] is written BY THE HOST when the batch is delivered: after its f16x3 range ticket has been judged and, if it
 * failed, the batch re-issued (re-calibrated / float32 kernels, from the context's own copy of its inputs into the context's own
 * pose buffer).  Delivery happens in submission order inside later davo_submit calls (whatever has finished by then; the oldest
 * is waited for once eight batches are undelivered), davo_wait and davo_synchronize.  pose_out must stay valid until then; it may
 * be pageable.  davo_wait(ctx, n) returns once at most n submitted batches are undelivered (n = 0: all delivered; the streams may
 * still be busy with range bookkeeping, davo_synchronize also idles them).  davo_pending = undelivered batches (>= 0).
 * davo_forward, davo_set_stream and davo_set_inflight deliver everything first. */
int davo_submit(davo_ctx* ctx, int B, const uint8_t* img, const float* flow, const float* seg, float* pose_out, int hold);
int davo_wait(davo_ctx* ctx, int leave_pending);
int davo_pending(davo_ctx* ctx);

/* Pair selection.  A window's two poses come from two independent evaluations of the shared PoseNN (davo.py:1456-1457): pair 0
 * reads (tgt, src0), pair 1 reads (tgt, src1), and nothing of one enters the other.  The reference's trajectory driver
 * (test_kitti_pose.py:143-145) uses T(tgt->src0) of a sequence's first window only and inv(T(tgt->src1)) of every window, so for
 * every window but the first, half of the arithmetic and 45 % of the input bytes serve a pose its caller drops.
 * davo_set_pairs chooses which pairs the batches issued AFTER the call run: DAVO_PAIRS_BOTH (the default: every launch, copied
 * byte and pose bit as without this entry point), DAVO_PAIRS_SRC0 or DAVO_PAIRS_SRC1; any other value returns DAVO_ERR_INVALID
 * with a message.  It may be called between batches at any time (no re-creation, no weight reload) and covers davo_forward,
 * davo_forward_device, davo_submit and their `_depth' forms.  Batches already in flight keep the selection they were issued with,
 * and so does every range-recovery re-issue of an earlier batch (as issued, re-calibrated, or on the float32 kernels).
 * The pose layout does not change: pose_out stays [B,2,6].  The selected pair's row is its pose - the same float32 chains per
 * pixel as in a both-pairs batch; the row of the pair that was not selected is written as exactly +0.0 ("zero motion").
 * With one pair selected a batch of B windows runs B pair images instead of 2 B, and no kernel reads a byte of the unselected source
 * frame - its third of the image strip, its flow plane, its label map, its depth plane - so device-path callers need not fill them;
 * the host entry points copy only what the selection reads (958,464 instead of 1,757,184 bytes per 128x416 window of the flagship).
 * davo_calibrate[_depth] keeps running both pairs of the batch it is handed.  davo_debug_read sizes the per-pair-image tensors
 * (cnv1..cnv7, packed, cnv5_se, cnv5_se_scale) by the pair images of the last forward: B of them with one pair, image n being
 * window n's selected pair.  davo_last_plan / davo_last_split report what ran.  davo_get_pairs returns the current selection. */
enum { DAVO_PAIRS_SRC0 = 1, DAVO_PAIRS_SRC1 = 2, DAVO_PAIRS_BOTH = 3 };
int davo_set_pairs(davo_ctx* ctx, int pairs);
int davo_get_pairs(const davo_ctx* ctx);

/* Frame sequences.  The entry points above take the reference's per-window dump format, in which consecutive windows of a
 * sequence repeat two of their three frames: a caller that holds a video (a camera, a decoder, a simulator) would build every
 * frame into three strips and send it across the link three times.  The `_frames' forms take every frame once.  N windows
 * (1 <= N <= max_batch) come as N + 2 frames; window n is (src0, tgt, src1) = frames (n, n + 1, n + 2):
 *   frames   uint8 [N+2,H,W,3]
 *   flow2    f32   [N,2,H,W,2]   (binary16 on a DAVO_FLOW_F16 context) planes (tgt->src0, tgt->src1) of window n: planes 0, 1 of davo_forward's [B,4,H,W,2], the two the
 *                                path reads
 *   seg            [N+2,H,W,1]   float32, or bytes on a DAVO_LABELS_U8 context (davo_set_label_format)
 *   depth    f32   [N+2,H,W,1]   (binary16 on a DAVO_DEPTH_F16 context) in the signature: NULL (or anything, ignored) where the variant reads no depth; where it does
 *                                (att_source 11, 12, 13) a NULL pointer returns DAVO_ERR_INVALID with a message
 *   pose_out f32   [N,2,6]       as davo_forward's
 * Device pointers are 16-byte aligned (DAVO_ERR_INVALID otherwise).
 * What is computed is the window form's, bit for bit: on the device one launch per batch (csrc/window_gather.h) expands the
 * frames into the window layout of a staging set of the context - the windows the caller would have built, byte for byte -
 * and the forward runs on that set like on any window batch.  So everything said above about davo_forward, davo_submit and
 * davo_forward_device holds for davo_forward_frames, davo_submit_frames and davo_forward_device_frames: synchronous or
 * streamed delivery and its order, `hold' (it counts the `_frames' and the window submits of a context alike), the f16x3 range
 * ticket and the re-issue from the library's own copy of the batch, davo_wait, davo_pending, davo_set_inflight,
 * davo_set_stream, davo_set_pairs, and davo_debug_read on the batch issued last (it sees the gathered window batch).  Window
 * and frame calls may be mixed freely on one context.  Where the forms differ:
 *   - davo_forward_frames sub-batches like davo_forward ("host_chunk"): windows [b0, b0 + nb) take frames [b0, b0 + nb + 2), and
 *     the two frames a sub-batch shares with the one before it are not sent again.  Its poses are the bits of davo_forward on
 *     the same windows.
 *   - davo_forward_device_frames gathers into the staging set of its in-flight slot (built by the slot's first such call) and
 *     runs that set: the caller's four buffers are free as soon as work ordered behind the call on the context's stream may
 *     run, with or without "stable_inputs" (the range guard snapshots the staging set, which is the library's).  The timed form
 *     brackets the gather too.
 *   - each in-flight slot of the host entry points gets a frame buffer of max_batch + 2 frames per plane kind at its first
 *     `_frames' call; a context that never makes one allocates nothing for the layout and issues no launch for it.
 * Pair selection (davo_set_pairs) narrows what is copied and gathered to the frames some selected window reads; the skipped
 * frames and flow planes may hold anything (device path: need not be filled).  Frames [lo, hi) of the caller's arrays:
 *   selection   frames (pixels)   flow plane   label maps, target not attended / attended   depth, sources 11, 12 / 13
 *   both        [0, N+2)          0, 1         [0, N+2)                                     [0, N+2)
 *   src0        [0, N+1)          0            [0, N)   / [0, N+1)                          [0, N+1) / [0, N)
 *   src1        [1, N+2)          1            [2, N+2) / [1, N+2)                          [1, N+2) / [2, N+2)
 * Bytes across the link per window of a long batch at 128x416, both pairs, no depth: 159,744 (one frame) + 851,968 (two flow
 * planes) + 212,992 (one float32 label map; 53,248 as bytes) = 1,224,704 (1,064,960 with byte labels) against the window
 * form's 1,757,184 (1,437,696); each batch sends its two extra frames once more.
 * davo_frames_plan is that table as a function (no context, no device): ranges[8] receives the [lo, hi) pairs of the frames,
 * the label maps, the depth planes (0, 0 where att_source reads none) and the flow planes of a batch of N windows, *link_bytes
 * the bytes the host entry points copy for it; either pointer may be NULL.  DAVO_ERR_INVALID for an argument out of range.
 * davo_frames_plan_fmt is the same with the flow format as an argument (DAVO_FLOW_F32 or DAVO_FLOW_F16: 8 or 4 bytes per
 * pixel and flow plane in *link_bytes; 638,976 per window for the line above with byte labels and binary16 flow);
 * davo_frames_plan means flow_fmt = DAVO_FLOW_F32 and takes att_source 0..13, the range it was published with; the pooled
 * flow-attention sources (14..17), which read what att_source 1 reads, are planned by davo_frames_plan_fmt.
 * davo_frames_plan_fmt2 is davo_frames_plan_fmt with the depth format as an argument too (DAVO_DEPTH_F32 or DAVO_DEPTH_F16: 4 or
 * 2 bytes per pixel and depth plane in *link_bytes); davo_frames_plan_fmt means depth_fmt = DAVO_DEPTH_F32.
 * There are no `_frames' forms of davo_calibrate, davo_forward_features and davo_forward_heat. */
int davo_forward_frames(davo_ctx* ctx, int N, const uint8_t* frames, const float* flow2, const float* seg,
                        const float* depth, float* pose_out);
int davo_submit_frames(davo_ctx* ctx, int N, const uint8_t* frames, const float* flow2, const float* seg,
                       const float* depth, float* pose_out, int hold);
int davo_forward_device_frames(davo_ctx* ctx, int N, const void* d_frames, const void* d_flow2, const void* d_seg,
                               const void* d_depth, void* d_pose, float* elapsed_ms);
int davo_frames_plan(int H, int W, int N, int pairs, int att_source, int label_fmt, int* ranges, long long* link_bytes);
int davo_frames_plan_fmt(int H, int W, int N, int pairs, int att_source, int label_fmt, int flow_fmt, int* ranges, long long* link_bytes);
int davo_frames_plan_fmt2(int H, int W, int N, int pairs, int att_source, int label_fmt, int flow_fmt, int depth_fmt, int* ranges,
                          long long* link_bytes);

/* Mirrored inputs.  The reference treats left-right mirrored sequences as data of their own: it trains with --data_flip
 * (data_loader.py:77-84, 142-169), its feature-map driver writes `featuremaps-flip', and it ships mirrored ground truth
 * (kitti_benchmark/data/odometry/poses-flip/NN-flip.txt).  davo_set_flip(ctx, 1) makes the context mirror every batch issued AFTER
 * the call on the device, by the training loader's rule - flip(X):
 *   - each frame is mirrored left-right inside its own third of the strip;
 *   - each flow plane, label map and depth plane is mirrored left-right on its own;
 *   - no value changes: in particular the horizontal flow component is NOT negated (npy_flip does not negate it, and that is
 *     what a flip-trained network saw);
 *   - plane order and frame order stay.
 * The whole contract: a context with flip on, given X, computes bit for bit what the same context with flip off computes on
 * flip(X) - for every entry point, format, pair selection, topology and precision, every tensor davo_debug_read returns and
 * both exports.  (davo_amd.flip_windows / flip_frames are flip() in numpy.)
 * NOT built: the reference's own test-time switch (generate_feature_map.py:118-129).  It hands the [B,H,3W,3] strip to img_flip,
 * which sees three channels and treats the strip as ONE image: the strip is mirrored as a whole, src0 and src1 trade places while
 * their flows and label maps do not.  That is an accident of img_flip's channel count, not a rule.
 * Any value but 0 or 1 returns DAVO_ERR_INVALID with a message.  It may be called between batches at any time, like
 * davo_set_pairs; batches in flight keep the setting they were issued with, and so does every range-recovery re-issue (the
 * library's copy of a batch is taken after the mirror, so a re-issue never mirrors again).  The default is off: every launch,
 * copied byte and pose bit is then what it is without this entry point, and a context that never switches it on allocates
 * nothing and launches nothing for it.  davo_get_flip reads it back.  Where the mirror happens (csrc/window_mirror.h), always
 * once, where a batch becomes the staging set its forward reads; only what the pair selection and the variant read is touched:
 *   frame layout (every `_frames' call)                    inside the gather launch (mirrored stores): no launch more
 *   window layout from the host (davo_forward, davo_submit, their `_depth' forms, davo_forward_features, davo_forward_heat)
 *                                                          one `window_mirror' launch per sub-batch on the staging set, in place
 *   window layout on the device (davo_forward_device[_depth], davo_calibrate[_depth])
 *                                                          one `window_mirror' launch from the caller's buffers - never written -
 *                                                          into the slot's staging set, which the batch then runs from like a
 *                                                          device frame batch: it is the library's own copy, with or without
 *                                                          "stable_inputs".  The four pointers must be 16-byte aligned. */
int davo_set_flip(davo_ctx* ctx, int on);
int davo_get_flip(const davo_ctx* ctx);

/* Online tracking.  The `_frames' forms still take a finished piece of a video.  A live caller (one camera, or S simulators in
 * lockstep) gets one new frame per stream at a time: it would have to keep the last two frames itself, rebuild a three-frame
 * array for every step and send two of its three frames across the link again.  A tracking session does that on the device:
 * the caller pushes ONE new frame per lane, the context keeps the frames before it in a ring of its own, and the push yields the
 * poses of the window the frame completes - window (src0, tgt, src1) = the lane's frames (t - 2, t - 1, t) for push t = 0, 1, ...
 *   davo_track_begin(ctx, lanes, policy)   opens the session: 1 <= lanes <= max_batch video streams S, the ring (lanes x
 *            (in-flight slots + 2) frames, label maps and - depth variants - depth planes, in the context's label and depth
 *            formats) and its events.  Batches pending delivery are delivered first.  A second begin without an end, lanes out
 *            of range, an unknown policy and a context with an export switched on return DAVO_ERR_INVALID with a message.
 *   davo_track_push(ctx, frames, flow2, seg, depth, pose_out, hold)   host pointers, one push:
 *              frames   uint8 [S,H,W,3]      the new frame of every lane
 *              flow2          [S,2,H,W,2]    the flow planes (tgt->src0, tgt->src1) of the window this frame completes, tgt the
 *                                            frame pushed before it; the context's flow format
 *              seg            [S,H,W,1]      the new frame's label map; the context's label format
 *              depth          [S,H,W,1]      its depth plane, the context's depth format; NULL (or anything) where the variant
 *                                            reads none, DAVO_ERR_INVALID with a message for NULL where it does
 *              pose_out f32   [S,2,6]        written at delivery, as davo_submit's
 *            It is davo_submit_frames on the S windows (lane s, frames t - 2 .. t): streamed like it on the next in-flight slot,
 *            same bits as davo_forward_frames / davo_forward on those windows under the same selection and batch size, `hold'
 *            as there (pushes, `_frames' and window submits count alike), range ticket and re-issue (from the library's copy
 *            of the gathered windows: a re-issue never touches the ring), davo_wait, davo_pending, davo_synchronize.  Returns
 *            the number of windows issued - S, or 0 for the first two pushes of a session, which only store their frames
 *            (flow2 and pose_out are not read and may be NULL; the arrays are free on return) - or a negative davo_status.
 *            What a push copies: a frame, a label map and a depth plane per lane and the flow planes of its selection - at
 *            128x416, float32, tgt->src1: 159,744 + 425,984 + 212,992 = 798,720 bytes per lane (425,984 with byte labels and
 *            binary16 flow) against davo_submit_frames' 958,464 (585,728) at N = 1.  Planes the selection does not read may
 *            hold anything.
 *   davo_track_push_device(ctx, d_frames, d_flow2, d_seg, d_depth, d_pose, elapsed_ms)   the same from device buffers, 16-byte
 *            aligned (DAVO_ERR_INVALID otherwise), as davo_forward_device_frames: the frames are copied into the ring and the
 *            windows gathered on the slot's stream, so the caller's buffers are free once work ordered behind the call on the
 *            context's stream may run; they are never written.  d_pose [S,2,6] receives the poses in stream order.
 *   davo_track_frames(ctx)   frames pushed per lane so far (DAVO_ERR_INVALID outside a session).
 *   davo_track_end(ctx)      delivers what is pending, waits for the ring's last reader and frees the ring and its events
 *            (davo_destroy does the same for a session left open).  A context that never begins a session allocates nothing
 *            and launches nothing for it.
 * Policy - which pairs a push runs (davo_set_pairs explains the selections; an unselected row of pose_out is +0.0):
 *   DAVO_TRACK_TRAJECTORY   the session's first window runs both pairs, every later push DAVO_PAIRS_SRC1: what a trajectory needs
 *                           (run_kitti_pose --pairs trajectory).  davo_set_pairs is not read.
 *   DAVO_TRACK_AS_SET       every push runs the selection davo_set_pairs holds when it is issued.
 * A three-frame context (davo_set_posenn_topology) runs whole windows under either.
 * The ring holds frames as pushed, never mirrored: davo_set_flip mirrors inside the gather launch as in the frame layout, no
 * launch more, and toggling it between pushes applies to the pushes issued after the call.  Nothing of a ring place that no
 * selected pair reads is read.  (csrc/window_gather.h: the gather kernel takes a frame base per window third; DESIGN.md
 * section 2 "Online tracking": how uploads and gathers of different slots are ordered, by events and never through the host.)
 * Between pushes every window and `_frames' call, davo_set_flip, davo_set_pairs, davo_set_stream, davo_wait and
 * davo_synchronize are legal and leave the ring alone.  REFUSED during a session, with DAVO_ERR_INVALID and a message:
 * davo_set_inflight (the ring is sized by the slots the session began with), davo_set_feature_export, davo_set_heat_export
 * (there are no exports under tracking), davo_calibrate[_depth] and the three input format setters.
 * davo_track_plan is a pure function like davo_frames_plan_fmt2 (no context, no device): *link_bytes receives the bytes one
 * push of `lanes' lanes copies under selection `pairs' - davo_frames_plan_fmt2's figure for N = 1 per lane less the frames,
 * label maps and depth planes it sends again.  davo_track_ring is the ring's index rule as a pure function: for push t of a
 * session begun with `inflight' slots it returns the ring's places R = inflight + 2 (or DAVO_ERR_INVALID); places[4] receives
 * the place the push uploads into (t mod R) and the three its window reads ((t - 2 + k) mod R; -1 for t < 2); after[5] the pushes
 * whose gather the upload is ordered behind (t - R, t - R + 1, t - R + 2: the readers of that place; -1 where that push gathered
 * nothing) and the two whose upload the gather is ordered behind (t - 2, t - 1).  Either pointer may be NULL.
 * Not built: lanes that start at different times, more than one new frame per lane and push (the `_frames' forms catch up),
 * exports, multi-rank sessions, and the pose chain itself, which stays with the caller (davo_amd.Tracker does it the reference's
 * way). */
enum { DAVO_TRACK_TRAJECTORY = 0, DAVO_TRACK_AS_SET = 1 };
int davo_track_begin(davo_ctx* ctx, int lanes, int policy);
int davo_track_push(davo_ctx* ctx, const uint8_t* frames, const float* flow2, const float* seg, const float* depth,
                    float* pose_out, int hold);
int davo_track_push_device(davo_ctx* ctx, const void* d_frames, const void* d_flow2, const void* d_seg, const void* d_depth,
                           void* d_pose, float* elapsed_ms);
int davo_track_frames(const davo_ctx* ctx);
int davo_track_end(davo_ctx* ctx);
int davo_track_plan(int H, int W, int lanes, int pairs, int att_source, int label_fmt, int flow_fmt, int depth_fmt,
                    long long* link_bytes);
int davo_track_ring(int inflight, long long t, int* places, long long* after);
/* Test hook: fills ring place `place' (0 .. R - 1) of the open session - its frames, label maps and depth planes - with `byte',
 * after waiting for everything in flight that touches the ring.  No forward calls it. */
int davo_track_debug_fill(davo_ctx* ctx, int place, int byte);

/* The pooled flow-attention variants' window geometry (att_source 14..17) as a function (no context, no device): the cells of the
 * SE descriptor of an H x W frame, in descriptor order (entries 2 i, 2 i + 1 are the x and y means of cell i).  *n_cells receives
 * their number (D / 2; 0 for a source that does not pool); rects, where not NULL, [n][4] = rows [y0, y1) and columns [x0, x1) of
 * each cell cut to the real image (0, 0, 0, 0 for a cell that lies wholly in tf.pad's zeros); inv_div, where not NULL, [n] the
 * reciprocal of the cell's divisor: its own pixel count for gp2x2, for SPP the window height times its columns inside the
 * tf.pad-ded map - tf.pad's zeros count, SAME padding does not (nets/attention_module.py:68-77, 137-167).  Call it once with NULL
 * arrays for the count (at most 116).  DAVO_ERR_INVALID for an argument out of range. */
int davo_pool_plan(int H, int W, int att_source, int* n_cells, int* rects, float* inv_div);

/* Feature export.  Replaces DAVO.inference(sess, mode='feature') (davo.py:1553-1569), the call generate_feature_map.py:183-260
 * makes to draw the class-attention table and the cnv6 feature maps: the poses of davo_forward and, from the same forward, the
 * tensors of the reference's `masks', `features' and `images' fetches.  Frames are in the order tgt, src0, src1 throughout.
 *   att_19        [3][B][19]       att_19[f][b][c] is the value frame f's attention map takes on a pixel of class c
 *                                  (generate_feature_map.py:187-192 reads rows 1 and 2; davo.py:1493 has the fetch commented out).
 *                                  Where the forward looked a class table up for the frame - the source frames of every table source,
 *                                  the target where the variant attends it - the row is that table; where the reference overrides the
 *                                  map with tf.ones_like (the target under -se_flow, `_wo_tgt' and -static, every frame under
 *                                  -no_segmask: davo.py:1387,1394,1218) it is 19 ones.  (The reference's att_19s holds an se() output
 *                                  nobody multiplies in there; this entry point reports what was applied.)
 *   attention     [3][B][H][W]     the maps multiplied in, after those overrides (davo.py:1405-1414,1468): the gather of att_19 through
 *                                  int(seg), 0 on labels outside [0,19) (one_hot of an out-of-range id, davo.py:1115), 1 everywhere on
 *                                  an overridden frame
 *   masked_image  [3][B][H][W][3]  input_images[k][..., :3] after masking (davo.py:1419-1421,1447-1449,1471-1475): the float32
 *                                  expression the PoseNN input is packed with; the plain rgb where the version does not mask rgb
 *   image         [3][B][H][W][3]  the preprocessed frames u8 * (1/255) * 2 - 1, unmasked (davo.py:967-971,1519-1522)
 *   feat_rot,     [B][H][W][cnv6_out] each: tf.image.resize_bilinear(cnv6, (H, W)) of the rotation / translation head of the
 *   feat_trans                     tgt->src1 PoseNN call (davo.py:1457,1463-1465).  TF 1.13's resize: align_corners=False, no half-pixel
 *                                  centres, so in = out / 4 exactly (cnv6 is [H/4, W/4] for every shape davo_create accepts),
 *                                  lo = out >> 2, lerp = (out & 3) / 4, hi = min(lo + 1, last); per value in float32, in TF's order
 *                                  top = tl + (tr - tl) xl, bot = bl + (br - bl) xl, out = top + (bot - top) yl.  The corners are the
 *                                  stored cnv6 as davo_debug_read("cnv6") decodes it, so out[4i][4j] equals it to the bit.
 * att_source 13 (the depth-split flow attention): `attention' is the per-pixel select of the near and the far table by the frame's own
 * depth plane, `masked_image' the packer's expression with it; no single 19-row table was applied and the reference sets no att_19s
 * for the branch (davo.py:1470), so a non-NULL att_19 member returns DAVO_ERR_INVALID before anything runs.
 * `flows' and `segs' of the reference's dict are colourings of the caller's own inputs (flow_to_image, label_to_color_image) and
 * are not built; `seg_19' is the one-hot of the caller's label maps and needs nothing from the device (davo_amd.DAVO builds it).
 *
 * davo_set_feature_export(ctx, 1) allocates the export workspace (room for one davo_forward sub-batch of every tensor above),
 * davo_set_feature_export(ctx, 0) and davo_destroy free it; it is off by default, and a context that never switches it on
 * allocates and launches nothing for it.
 * davo_forward_features takes host pointers like davo_forward (seg: bytes on a DAVO_LABELS_U8 context; depth: the planes of a depth source as davo_forward_depth takes
 * them, NULL or ignored for any other variant) and is synchronous.  pose_out receives bit for bit what davo_forward returns on
 * the same inputs and context state.  Every member of *out that is not NULL receives its tensor for all B windows, whatever
 * "host_chunk" is; a NULL member is neither computed nor copied, and out == NULL or all members NULL is a plain davo_forward.
 * The exports come from the forward that produced the returned poses: a batch whose f16x3 range record fails its verdict is
 * re-issued first (re-calibrated, or on the float32 kernels) and exported from the re-issue, in the precision it ran.
 * Errors: DAVO_ERR_NOT_READY while the export is off; DAVO_ERR_INVALID unless the pair selection is DAVO_PAIRS_BOTH (the
 * reference's semantics: features are those of the second pair, maps of all three frames); otherwise davo_forward_depth's.
 * Works in both precisions, with davo_set_posenn_se (the features are still the stored cnv6, rotation | translation) and with
 * davo_set_impl(ctx, 1).  There is no streaming (davo_submit) form: this is the visualisation path. */
int davo_set_feature_export(davo_ctx* ctx, int on);
typedef struct {
    float* att_19;
    float* attention;
    float* masked_image;
    float* image;
    float* feat_rot;
    float* feat_trans;
} davo_feature_out;
int davo_forward_features(davo_ctx* ctx, int B, const uint8_t* img, const float* flow, const float* seg,
                          const float* depth, float* pose_out, const davo_feature_out* out);

/* Heat export.  The reference's only reader of feat_rot / feat_trans is generate_feature_map.py:204-265, which reduces each map at
 * once to np.sum(axis=-1), np.mean(axis=-1) and the scalar max() that normalises the mean image, and draws those: two [H,W] planes
 * and two scalars per window (426 KB at 128x416) where the full maps are 54.5 MB.  davo_forward_heat delivers exactly that, reduced on
 * the device where cnv6 lies, at [H/4, W/4], reading it once; the full maps exist on neither side of the bus.  Two identities:
 *   - sum o resize = resize o sum: the resize is linear with weights that do not depend on the channel, so the channel sum of
 *     resize_bilinear(cnv6) is resize_bilinear of the channel sum;
 *   - max of the resized map = max of the stored map: at the library's one scale (lo = out >> 2, lerp (out & 3) / 4) every stored
 *     value reappears unchanged at out[4i][4j], and every other output is an interpolation between corners that does not leave
 *     their range - in float32 and TF's order too.
 *   rot_sum, trans_sum  [B][H][W]  resize_bilinear (feat_rot's rule and float32 order: top = tl + (tr - tl) xl, bot likewise,
 *                                  out = top + (bot - top) yl) of the float32 sum over the head's cnv6_out channels of the stored cnv6
 *                                  of the tgt->src1 call, each value decoded as davo_debug_read("cnv6") decodes it.  The sum is one
 *                                  fixed tree, (c0 + c1) + (c2 + c3) per four channels and then pairwise, at most 8 roundings deep:
 *                                  bitwise reproducible.  out[4i][4j] is that sum to the bit.  The mean is sum * (1 / cnv6_out), exact
 *                                  (the width is a power of two); the caller multiplies.
 *   rot_max, trans_max  [B]        the largest value of the head's [H/4][W/4][cnv6_out] block, equal to feat_*.max() of the same
 *                                  forward to the bit (cnv6 is post-ReLU: at least +0).
 * davo_set_heat_export(ctx, 1) allocates a workspace of its own - per window of one davo_forward sub-batch 2 (H/4 W/4 + H W + 1)
 * floats - independent of davo_set_feature_export; (ctx, 0) and davo_destroy free it; off by default, and a context that never
 * switches it on allocates and launches nothing for it.
 * davo_forward_heat is davo_forward_features plus the heat members: the same inputs (seg: bytes on a DAVO_LABELS_U8 context), synchronous, the same sub-batching under
 * "host_chunk", the same pair-selection rule (DAVO_PAIRS_BOTH, else DAVO_ERR_INVALID), both precisions, davo_set_posenn_se and
 * davo_set_impl(ctx, 1); pose_out is bit for bit davo_forward's; a batch that fails its f16x3 range verdict is re-issued first and
 * exported from the re-issue, in the precision it ran.  A NULL member is neither computed nor copied; `out' or `heat' may be NULL.
 * Non-NULL members of `out' need davo_set_feature_export on, non-NULL members of `heat' need davo_set_heat_export on: otherwise
 * DAVO_ERR_NOT_READY with a message naming the switch. */
typedef struct {
    float* rot_sum;
    float* trans_sum;
    float* rot_max;
    float* trans_max;
} davo_heat_out;
int davo_set_heat_export(davo_ctx* ctx, int on);
int davo_forward_heat(davo_ctx* ctx, int B, const uint8_t* img, const float* flow, const float* seg,
                      const float* depth, float* pose_out,
                      const davo_feature_out* out, const davo_heat_out* heat);

const char* davo_last_error(const davo_ctx* ctx);
void davo_destroy(davo_ctx* ctx);

/* ---- device memory / stream plumbing for hosts without a HIP binding (ctypes) ---------- */
int davo_device_malloc(davo_ctx* ctx, size_t bytes, void** out);
int davo_device_free(davo_ctx* ctx, void* p);
/* Page-locked host memory for the buffers handed to davo_forward (what tf.data's prefetch-to-pinned
 * staging does under sess.run, data_loader.py:319-325): H2D then runs as DMA at the PCIe rate and
 * overlaps the kernels of the previous sub-batch.  Pageable buffers work too, just slower. */
int davo_host_alloc(int device, size_t bytes, void** out);
int davo_host_free(void* p);
/* Page-lock memory the caller already owns (hipHostRegister), e.g. the shared-memory batch buffers that the input
 * pipeline's worker processes decode into (davo_amd/loader.py: ProcessWindowLoader); undo with davo_host_unregister
 * before the memory is unmapped. */
int davo_host_register(int device, void* p, size_t bytes);
int davo_host_unregister(void* p);
int davo_memcpy_h2d(davo_ctx* ctx, void* dst, const void* src, size_t bytes);
int davo_memcpy_d2h(davo_ctx* ctx, void* dst, const void* src, size_t bytes);
/* Gives every f16x3 batch issued through davo_forward_device and not judged yet its range verdict (each on its own
 * record), then waits for every stream of the context.  A batch that left the fp16-pair storage range is re-issued
 * before the call returns (re-calibrated, or on the float32 kernels: "auto_range"), so on DAVO_OK every pose buffer
 * holds float32-grade results.  With "auto_range" 0 the first failed verdict is returned as DAVO_ERR_RANGE instead
 * (the poses of that batch are not float32-grade; all batches have been judged, nothing stays pending). */
int davo_synchronize(davo_ctx* ctx);
/* Run on a caller-owned hipStream_t (NULL restores the context's own stream).  Batches issued on the stream the context leaves
 * are judged (and, if need be, re-issued) inside this call, i.e. it waits for them: the old stream may be destroyed afterwards. */
int davo_set_stream(davo_ctx* ctx, void* hip_stream);
/* Number of batches davo_forward_device keeps in flight (1..4, default 1).  With n > 1 the context
 * owns n streams and n activation workspaces and successive calls rotate through them, so the small
 * kernels of one batch overlap the large convolutions of another (the counterpart of the
 * reference's tf.data prefetch, data_loader.py:321-324; +3...7 % throughput at n = 2, B = 32).  The
 * caller must give concurrent calls distinct input/output buffers and call davo_synchronize()
 * before reading results.  davo_forward (host buffers) stays synchronous. */
int davo_set_inflight(davo_ctx* ctx, int n);

/* ---- measurement ---------------------------------------------------------
 * With profiling on, every kernel launch of davo_forward[_device] is bracketed by HIP events
 * on the launch stream.  davo_profile_entry(i) returns the kernel's label, number of timed
 * launches and total device milliseconds since the last davo_profile_reset(); it returns
 * DAVO_ERR_INVALID once i is past the last entry.  Reading synchronises the stream. */
int davo_profile_enable(davo_ctx* ctx, int on);   /* 0 off | 1 every kernel | 2 only the dominant kernel (main cnv6 launch) */
int davo_profile_reset(davo_ctx* ctx);
int davo_profile_entry(davo_ctx* ctx, int i, char* name, int name_len, int* launches,
                       double* total_ms);
/* Per-launch record of one label since the last reset, in issue order: which = 0 the launches' own durations (ms),
 * which = 1 the time from the previous bracketed launch's START to this one's (with every batch bracketed, one step's
 * period on the stream; -1 for the first sample).  Copies up to cap floats, returns the number recorded (>= 0) or a
 * negative davo_status.  bench.py reports the clock ramp of its timed region from it. */
int davo_profile_samples(davo_ctx* ctx, const char* name, int which, float* out, int cap);

/* How the LAST forward issued conv layer `layer` (0..6 = cnv1..cnv7): launch 0 is the main launch,
 * launch 1 the remainder launch with a narrower N tile (mtiles = 0 if there was none).  A launch
 * covers `mtiles` 128-row M tiles x all output channels, in N tiles of `bn`.  bench.py uses it to
 * price the FLOPs of the launch it puts on the roofline. */
int davo_last_plan(davo_ctx* ctx, int layer, int launch, int* mtiles, int* bn);
/* Split-K parts of that layer's launch in the LAST forward: 1 where every output is one chain over K (and 0 before the
 * first forward), else the number of partial sums a fix-up added (f16x3 cnv5 / cnv6 on a launch of few tiles, "split_k").
 * davo_last_plan reports the same tiles either way; the tests use this to show which branch ran. */
int davo_last_split(davo_ctx* ctx, int layer, int* parts);

/* Arithmetic of the convolution stack:
 *   1 (default) "f16x3": every float32 operand is split into two fp16 halves (22 significant
 *      bits) and each product is three fp16 MFMA products accumulated in float32 — float32-grade
 *      results (measured ~1e-7 relative on the 6-DoF outputs) at 5.3x less matrix-pipe time;
 *      a layer's activations must stay within the fp16-pair range (see davo_calibrate below).
 *   0 "f32": v_mfma_f32_32x32x2_f32, bit-for-bit float32 fmaf chains, no range restriction. */
int davo_set_precision(davo_ctx* ctx, int precision);

/* f16x3 range management.  Activations between layers are stored as fp16 (hi, lo) pairs; a layer's values must
 * stay below 65504 (they are clamped there) and its largest value at or above 2^-6 for the pairs to carry float32-grade
 * precision.  Each storing kernel records the largest value it wrote (running maxima: a clamped value is caught in the very call
 * that stores it, "too small" on what has been stored since the record was last zeroed - by a recovery, a change of scales, and for
 * every 256th call / batch); davo_forward judges the record at the end of its call.
 * The reference's float32 graph never fails on a finite network (davo.py:1553-1569), so by default neither does this
 * library: a batch that left the range is re-issued with the scales re-calibrated ON THAT BATCH, and if it still
 * leaves the range (no per-layer power of two covers it) on the float32 kernels — mode 0 below, for that batch only;
 * later batches run f16x3 with the new scales.  davo_range_stats counts what happened.  davo_set_option(ctx,
 * "auto_range", 0) turns the recovery off: the entry points then return DAVO_ERR_RANGE (poses are still written, not
 * float32-grade) and the caller calibrates or changes mode itself.  davo_calibrate runs the path on
 * a sample batch (device buffers, as davo_forward_device: d_seg points at bytes on a DAVO_LABELS_U8 context) and gives every layer an exact power-of-two storage
 * scale that puts its largest value in [512, 1024); results inside the safe range do not depend on the scales
 * beyond rounding noise (~1e-8).  The reference's float32 graph needs none of this (TF conv2d, nets/posenn.py:205-215);
 * mode 0 (f32) ignores the scales.
 *   davo_activation_range: max_abs[6] = largest |activation| written by cnv1..cnv6 since the last reset (true
 *     magnitudes), shifts[6] = log2 of the storage scales; either may be NULL.  Synchronises.
 *   davo_set_activation_shifts: install scales from an earlier calibration (NULL = all zero). */
int davo_calibrate(davo_ctx* ctx, int batch, const void* d_img, const void* d_flow, const void* d_seg, int* shifts_out);
int davo_activation_range(davo_ctx* ctx, float* max_abs, int* shifts, int reset);
int davo_set_activation_shifts(davo_ctx* ctx, const int* shifts);
/* Back to the range state davo_create left: batches issued so far are judged (and recovered) first, then the storage scales
 * are all zero again, every range record is zeroed, the maxima of davo_activation_range start over, the every-256th-batch
 * counters and the record ring's cursor are where a new context has them, and davo_range_report is "".  What the context does
 * next - a davo_calibrate, its batches, their verdicts - is then what a new context with the same weights would do: a driver
 * that runs several independent jobs (sequences) on one context calls this between them, and a job's results do not depend on
 * the jobs before it.  The counts of davo_range_stats are not reset (they are "since davo_create"; take differences).
 * Synchronises; launches nothing and changes nothing for a caller that never calls it. */
int davo_reset_range_state(davo_ctx* ctx);
/* Range recoveries since davo_create: re-calibrations triggered by a failed verdict, batches that ran on the float32
 * kernels because no scale covered them, batches re-issued in total.  Any pointer may be NULL. */
int davo_range_stats(davo_ctx* ctx, long long* recalibrations, long long* f32_batches, long long* reissued);
/* What the range management last did, in words ("" if nothing yet): which layer's verdict triggered a re-calibration or
 * a float32 batch, or which weight tensor's per-input-channel spread keeps the network on the float32 kernels.  The
 * string lives until the next call on the context. */
const char* davo_range_report(const davo_ctx* ctx);

/* Options.
 *   "auto_range" (default 1): f16x3 batches that leave the fp16-pair storage range are re-issued (see above); 0 = the
 *       failed verdict is returned as DAVO_ERR_RANGE.
 *   "stable_inputs" (default 0): 1 = the caller keeps the input buffers of every davo_forward_device batch unchanged
 *       until davo_synchronize(); the library then takes no copies of them (see davo_forward_device).
 * Kernel-fusion switches of the f16x3 path (both modes give the same poses to ~1e-7):
 *   "fuse_pose" (default 1): pred 1x1 + spatial mean + 0.01 (nets/posenn.py:240-250) run in cnv7's
 *       epilogue; the cnv7 activation is never written to HBM.  0 = cnv7 stored, separate pose-head kernels.
 *   "fold_tails" (default -1 = auto): 1 = the 2->8->19 excitation MLP runs in the workgroup of the squeeze launch that
 *       delivers a triplet's last partial sum, and the pose head's sum over cnv7's tiles in the workgroup of the cnv7
 *       launch that finishes last (csrc/pose_tail.h: ticket counters, agent-scope loads and stores, fixed summation order):
 *       two launches fewer per batch; 2 = the excitation only; 0 = se_excite / pose_from_tiles as launches of their own.
 *       The memory-side round trips cost more than the launches they save except at the smallest batches (B = 32: squeeze
 *       +18 us, cnv7 +3 us against 13 us of launches), so auto folds the excitation at batch <= 2 only.  Bit-identical.
 *   "deep_ring" (default 1): launches of at most one workgroup per CU (batch 1..4) run the same tiles on LDS rings of 3..6
 *       slots instead of 2 (more chunks of LDS-DMA in flight behind a counted wait).  Bit-identical results.
 *   "split_k" (default 1): cnv5 / cnv6 launches of at most half a workgroup per CU (batch 1 at 128x416) run the two halves
 *       of their input channels as two groups of the same kernel into float32 partial sums; a fix-up kernel adds them,
 *       applies ReLU and writes the stored form (cnv6 at batch 1: 52 -> 39 us).  Two partial sums instead of one chain: the
 *       layer's outputs - and so the poses - agree with the single chain to float32 rounding (~1e-7 relative), not to the
 *       bit; 0 = one K chain at every batch size (poses then do not depend on how windows are batched, with "fuse_pose" 0
 *       to the bit).
 *   "fold_fixup" (default 0): with "split_k", the part of a tile that finishes last adds the tile's partial sums and writes the stored
 *       form itself, so the two fix-up launches of a batch-1 forward (7 us each) go: the parts of a tile are the workgroups (x, 0..S-1)
 *       of a grid whose x extent is a multiple of 8, workgroup ids go round-robin over the XCDs (checked on the device once per
 *       context), so the partial sums meet in one XCD's L2.  Same additions in the same order: bit-identical to 0.  Measured SLOWER
 *       (batch 1: 0.141 against 0.132 ms per forward, profiles/r05k_fold_fixup_ab.md): one workgroup per tile adds what the fix-up
 *       launch spreads over the whole chip, behind a ticket's memory-side round trip; kept for experiments.
 *   "f32_n16" (default 1; float32 mode): cnv1 (16 output channels) on a 128x16 tile with v_mfma_f32_16x16x4_f32 instead of the
 *       128x32 tile whose matrix instructions were half padding.  Another order of the same float32 fma chain per output.
 *   "f32_n256" (default 0; float32 mode): cnv5 / cnv6 on a 128 x 256 tile of eight waves, one workgroup per CU (csrc/conv_igemm.h,
 *       conv_igemm_f32_n256): a pixel tile is staged once for all 256 output channels.  Bit-identical; measured 4 % slower per step
 *       than the 128-column tiles (eight waves behind one barrier stay in step: MEASURED_AND_REJECTED.md); kept for experiments.
 *   "merge_rem_f32" (default 1; float32 mode): where cnv4 / cnv5 / cnv6 are planned as a main launch of whole rounds of 128-column tiles
 *       plus a remainder launch of narrower ones, both run as ONE grid (csrc/conv_igemm.h, conv_igemm_f32_mainrem): workgroups are
 *       handed out in id order, so the remainder's tiles start on the CUs that finish their last main tile first (float32 step
 *       -1.8 % at B = 32; cnv7 measured slower merged and keeps two launches).  Bit-identical to 0.
 *   "patch_f32" (default 1; float32 mode): cnv1, cnv2 and cnv3 from an LDS-staged input patch on v_mfma_f32_16x16x4_f32
 *       (csrc/conv_patch_f32.h: the f16x3 patch kernels' recipe in float32) instead of the implicit GEMM: 0.153 / 0.070 / 0.091
 *       -> 0.108 / 0.049 / 0.069 ms at B = 32.  Another fixed order of the same float32 fma chain per output.
 *   "tile_208x128" (default 0): 1 = cnv4 may run on a 208-pixel x 128-channel tile of four waves (csrc/conv_igemm_h3s.h): whole
 *       rounds of the 256 CUs at every batch that is a multiple of 8, bit-identical results, measured 8 % slower than the
 *       128x128 tile at B = 32 and level at B = 16; kept for experiments.
 *   "merge_order" (default -1 = 2 where the launch has a tile order, see "skip_order", else 0): how the merged grid interleaves
 *       its two tile shapes: 0 = offset inside every XCD (half of each XCD's CUs run their short tile first), 1 = per XCD (even
 *       XCDs first, odd XCDs last: an XCD's CUs stay in step, a fifth fewer L2 misses, 0.5 % slower), 2 = all main tiles, long
 *       ones first, then the remainder tiles.  Bit-identical results.
 *   "skip_order" (default 1): the 3x3 kernels do not walk the chunks of a filter row that is zero padding for every pixel of
 *       a tile (davo_tile_filter_rows), so the tiles of a launch differ in length; every XCD's run of tiles can be handed out
 *       long tiles first (a device table per launch shape): 0 = never, 1 = in the float32 launches (cnv5 850 -> 793 us),
 *       2 = in the f16x3 merged grids too (cnv5 259.9 -> 256.8 us, a third more HBM reads, same step time under the power cap).
 *       Bit-identical results.
 *   "pad_classes" (default 1; float32 mode): cnv5 and cnv6 run on GEMM rows sorted by padding class - the pixels of a tile
 *       share the set of filter taps that land inside the image, and the tile walks only those (davo_pad_class_tables): the
 *       column taps of the left and right `rate` map columns are dropped too, which no flat run of pixels can do.  The dropped
 *       terms are exact zeros: bit-identical to 0 = the natural order.  8 + mask (8..15): exactly the layers of the mask (1 cnv4,
 *       2 cnv5, 4 cnv6); cnv4 has the kernels too but measured level at B = 32 and is not in the default.  Other values are
 *       refused.  Float32 step at B = 32: 3.553 -> 3.493 ms (cnv5 798 -> 761 us, cnv6 1770 -> 1745 us).
 *   "merge_cnv4" (default 0): cnv4 as whole rounds of 256x128 tiles + 128x128 remainder tiles in one grid like cnv5 / cnv6
 *       ("merge_rem"); measured level with the single launch of 128x128 tiles.  Bit-identical results.
 *   "fuse_pack" (default -1 = auto, which is off: measured level at every batch): 1 = cnv1 builds its input patch from
 *       the raw inputs (mask + pack fused in).
 *   "patch_cnv2", "patch_cnv3" (default 1): cnv2 (5x5 stride 2) / cnv3 (3x3 dilation 2) read their taps from an LDS-staged
 *       input patch (csrc/conv_patch_h3.h); 0 = the implicit-GEMM kernel.  The two sum a pixel's taps in different orders:
 *       poses agree to float32 rounding.
 *   "patch_cnv1_t" (default 1; three-frame PoseNN, davo_set_posenn_topology, f16x3 only): cnv1 at 16 packed channels reads its
 *       taps from an LDS-staged patch, two 8-channel passes per tile (csrc/conv_patch_h3.h, conv_patch_cnv1t_h3); 0 = the
 *       implicit-GEMM kernel at cin = 16.  Measured in one process, arms interleaved, 128x416: 54.8 against 112.6 us at B = 32,
 *       12.1 against 23.3 us at B = 1 (profiles/three_frame_measure.log).  The two sum a pixel's products in different orders:
 *       poses agree to float32 rounding.  No effect on a pairs context or in float32 mode (conv_igemm_f32 at cin = 16 there).
 *   "merge_rem" (default 1): where cnv5 / cnv6 are planned as a main launch of 256x256 tiles plus a remainder launch of
 *       128x128 tiles (B = 32), both run as ONE grid in which half of the CUs take their remainder tile first and the other
 *       half last (csrc/conv_igemm_h3.h, conv_igemm_h3_mainrem): the halves' store bursts no longer coincide.  0 = two
 *       launches.  Same tiles, same kernels' arithmetic: bit-identical results.
 *   "share_taps" (default 1): cnv3..cnv6 on the 256-row tiles stage ONE pixel patch per filter row for its three kx taps
 *       (csrc/conv_igemm_h3.h, RATE > 0); 0 = a staged chunk per tap.  Bit-identical results.
 *   "wave128" (default 2, round 5): 1 = cnv5 / cnv6's launches of whole 256x256 tiles run on FOUR waves of 128x128 outputs each
 *       (csrc/conv_igemm_h3w.h: 0.167 LDS fragment reads per matrix instruction instead of 0.25, which is what the power-capped
 *       matrix pipe's rate depends on; one wave per SIMD, every other instruction of the loop in a slot behind one MFMA); the
 *       layer's remainder rows then run as a launch of their own ("merge_rem" does not apply).  Same products in the same order:
 *       bit-identical to 0 = conv_igemm_h3's eight waves of 64x128.  -4.6 % per step at B = 32 (profiles/r05bd_w128_ab.log).
 *       2 = the remainder rows too leave conv_igemm_h3's 128x128 tiles: 256x64 tiles on four waves of 64x64 outputs, the shared pixel
 *       patch and deep DMA rings (conv_igemm_h3w64: 19 KB staged per chunk instead of 32; cnv5 / cnv6 remainder 34 / 59 -> 31 / 50 us,
 *       profiles/r05bh_w64_ab.log).  Bit-identical as well.
 *       With 2, cnv4 too runs on four-wave tiles (conv_igemm_h3w128: 256x128, shared patch, five-slot weight ring) where its 256-row
 *       tiles fill whole rounds of the CUs to within 12 % (B = 128: 0.385 -> 0.318 ms; B = 32: level, so not taken); 3 forces that kernel
 *       wherever it fits (test hook).  Bit-identical.
 *   "cu_partition" (default 0; with davo_set_inflight(ctx, n > 1)): slot i's stream is CU-masked to its own 1/n of every
 *       XCD's compute units (hipExtStreamCreateWithCUMask) and its launches are planned for that many CUs.  Measured
 *       without gain (HISTORY.md round 2); kept for experiments.  Results do not change.
 *   "force_tile" (test hook, default -1 = the launch planner decides): tile id of csrc/plan.h (0 128x32, 1 256x64,
 *       2 256x128, 3 128x256, 4 128x128, 5 256x256, 6 208x256); every f16x3 layer the tile fits is issued as one
 *       launch of that shape.  Poses do not depend on it beyond float32 rounding of the fused pose head's sums.
 *   "profile_stride" (default 1): with davo_profile_enable(ctx, 2) (only the dominant kernel bracketed by HIP events) the
 *       events go around every n-th batch's launch only: a pair costs two ~6 us pipeline bubbles around the launch it times.
 * Host-buffer entry point (davo_forward):
 *   "host_chunk" (default 8): windows per sub-batch; the H2D copy of sub-batch i+1 overlaps the kernels of
 *       sub-batch i when B >= 2*host_chunk.  0 = copy the whole batch, then compute.  Results do not change. */
int davo_set_option(davo_ctx* ctx, const char* key, int value);
/* Reading the options back.  The launch options - every key above but "auto_range", "stable_inputs", "cu_partition", "force_tile",
 * "profile_stride" and "host_chunk" - are one table (csrc/options.h): a row names the option, holds its default and the rule that
 * turns davo_set_option's value into the one the context stores (switches: value != 0; ranges clamp, with "merge_order" > 2 -> 0,
 * "fold_tails" > 2 -> 1, "fuse_pack" > 0 -> 1 and every negative auto value -> -1; "pad_classes": 0 -> 0, 1 -> 6, 8 + mask -> mask).
 *   davo_get_option: *value = the stored value of a launch option, or the current value of "auto_range", "stable_inputs",
 *     "cu_partition", "profile_stride" or "host_chunk".  "force_tile" is kept per layer and is refused, like an unknown key.
 *   davo_option_info (no context, no GPU): row i of the table - its name and its default in stored form; DAVO_ERR_INVALID
 *     for i < 0 and past the last row, which is how a caller finds the end.  Either pointer may be NULL.
 *   davo_option_store (no context, no GPU): *stored = what davo_set_option(ctx, key, value) would store for a launch option;
 *     DAVO_ERR_INVALID where it would refuse the value, and for every key that is no launch option. */
int davo_get_option(const davo_ctx* ctx, const char* key, int* value);
int davo_option_info(int i, const char** name, int* stored_default);
int davo_option_store(const char* key, int value, int* stored);

/* ---- multi-GPU: the pose gather of the window-sharded sequence driver, on RCCL ---------------
 * The reference runs one process on one GPU (test_kitti_pose.py:133-149: window loop, then the
 * sequential 4x4 chain).  Here one process per GPU takes a contiguous window range; the only
 * exchange is one all-gather of [n,2,6] float32 before the chain.  librccl is loaded on the first
 * call of this group.  Protocol: rank 0 calls davo_comm_unique_id and ships the DAVO_COMM_ID_BYTES
 * to the other ranks by any side channel (davo_amd/comm.py: a file), then every rank calls
 * davo_comm_init with its own context (one GPU per rank: RCCL refuses two ranks on one device).
 *   davo_allgather_poses: local [n_local,2,6] host floats (n_local <= n_per_rank; the rest of the
 *     rank's slot is zero-filled) -> all [nranks*n_per_rank,2,6] host floats on every rank, rank r's
 *     windows at [r*n_per_rank, ...).  elapsed_ms (may be NULL) = device time of the collective alone.
 *   davo_allgather_poses_device: the same on device buffers (n_per_rank windows in, nranks*n_per_rank
 *     out), after the context's own streams have drained.
 *   davo_comm_allreduce: one double, in place; op 0 sum | 1 max | 2 min (bench.py: max-over-ranks).
 *   davo_comm_barrier: every stream of this context idle, then a rendezvous of all ranks.
 *   davo_comm_preload: only loads librccl (573 MB to map, its code objects to register: most of a second); needs no context and
 *     may run on any thread, e.g. at process start behind the host's own imports.
 * Threads: davo_comm_preload, davo_comm_unique_id and davo_comm_init may run on a second host thread while the context's owner
 * thread issues forwards (a communicator takes seconds to build and is not needed before the gather); davo_comm_init publishes
 * the communicator into the context as its last step.  Every other call of this group belongs to the owner thread.
 * Errors: DAVO_ERR_COMM (message names the RCCL call); there is no fallback transport. */
#define DAVO_COMM_ID_BYTES 128
int davo_comm_preload(char* err, int err_len);
int davo_comm_unique_id(void* id_out, char* err, int err_len);
int davo_comm_init(davo_ctx* ctx, int nranks, int rank, const void* id);
int davo_comm_size(davo_ctx* ctx, int* nranks, int* rank);
int davo_allgather_poses(davo_ctx* ctx, const float* local, int n_local, int n_per_rank, float* all,
                         float* elapsed_ms);
int davo_allgather_poses_device(davo_ctx* ctx, const void* d_local, int n_per_rank, void* d_all,
                                float* elapsed_ms);
int davo_comm_allreduce(davo_ctx* ctx, double* value, int op);
int davo_comm_barrier(davo_ctx* ctx);
int davo_comm_destroy(davo_ctx* ctx);

/* ---- test hooks -------------------------------------------------------------------------
 * impl 0 = MFMA implicit-GEMM kernels (default, the product path);
 * impl 1 = one-thread-per-output direct convolution in HIP on the reference's own tensor
 *          layouts (10-channel input, HWIO weights) — an on-device cross-check, never timed
 *          (the feature-attention block runs on it too: the float32 forms of its three kernels). */
int davo_set_impl(davo_ctx* ctx, int impl);

/* Copy an intermediate of the LAST forward to host (float32, NHWC, pair-image major = 2B images):
 * "att_table" [B,3,19] (att_source 13: the near MLP's tables; "att_table_far" [B,3,19] holds the far MLP's and returns
 * DAVO_ERR_INVALID on every other variant), "se_desc" [B,2,D] (att_source 14..17 only: the pooled SE descriptors of src0, src1 as the
 * dense layer reads them; a frame no selected pair reads keeps what it held), "packed" [2B,H,W,8|10], "cnv1".."cnv5", "cnv6" [.., 2*cnv6_out]
 * (rotation | translation), "cnv7" [.., 512].  With davo_set_posenn_se(ctx, 1) also "cnv5_se_scale" [2B,2,256] (row 0 = s_r,
 * row 1 = s_r * s_t) and "cnv5_se" [2B,H/4,W/4,512] (cnv6's rotation input | its translation input).  After a davo_forward_heat
 * with the heat export on also "heat_sum" [2,n,H/4,W/4]: the channel sums (rotation | translation) the planes of the piece exported
 * last were resized from, n = that piece's windows (all B where the workspace holds the batch).
 * n_floats must equal the tensor size. */
int davo_debug_read(davo_ctx* ctx, const char* tensor, float* host_out, size_t n_floats);

/* Stand-alone slim.conv2d(padding='SAME') (nets/posenn.py:205-215) through the same MFMA
 * kernels, host pointers: x [N,H,W,Cin] float32 (Cin a power of two >= 4; >= 8 for f16x3),
 * w HWIO [k,k,Cin,Cout], y [N,ceil(H/stride),ceil(W/stride),Cout] float32.
 * k in {1,3,5,7}, stride in {1,2}; precision as davo_set_precision. */
int davo_conv2d_same(int device, const float* x, int N, int H, int W, int Cin,
                     const float* w, int k, int Cout, const float* bias,
                     int stride, int rate, int relu, int precision, float* y, char* err, int err_len);

/* The launch planner on its own (no GPU needed): how an f16x3 layer of M output rows x npad output
 * channels (x groups) is issued.  Up to two launches: rows[i] output rows in tiles of tile_bm[i] x
 * tile_bn[i]; returns the number of launches (1 or 2) or a negative davo_status. */
int davo_plan_layer(int M, int npad, int groups, int* rows, int* tile_bm, int* tile_bn);

/* The per-tile rule of the 3x3 kernels on its own (no GPU needed): a tile that covers the flattened output pixels [m0, m1]
 * of a [*, Hout, Wout] map walks only the filter rows [*ky0, *ky0 + *nky) that reach inside the Hin-row input for at
 * least one of its pixels (slim.conv2d pads with zeros: nets/posenn.py:205-215); the chunks of the other rows multiply
 * padding only and are skipped.  chunk_map[v], v < 3 * nky * nblocks (optional, may be NULL): index, in the layer's
 * weight rows, of the v-th chunk the f16x3 kernels walk for such a tile.  Returns DAVO_OK or a negative davo_status. */
int davo_tile_filter_rows(int m0, int m1, int Hout, int Wout, int Hin, int stride, int pad_t, int rate,
                          int* ky0, int* nky, int nblocks, int* chunk_map);

/* Class-sorted GEMM rows of the float32 dilated 3x3 layers on their own (no GPU needed; "pad_classes", csrc/pad_classes.h).
 * For NB images of a [Hout, Wout] output map read from a [Hin, Win] input with pad_t / pad_l zero rows / columns in front and
 * dilation `rate` (stride 1):
 *   row_pixel[ceil(M / 128) * 128], M = NB * Hout * Wout: GEMM row -> flattened output pixel n * Hout * Wout + oy * Wout + ox,
 *     -1 behind the last pixel.  Images are taken in blocks of ceil(NB / 8); inside a block the pixels are sorted by the set
 *     of filter taps that land inside the input (descending tap count, ties by ascending mask), in (image, oy, ox) order inside
 *     a class.  Where tiles that straddle classes would make that order walk no fewer taps than the natural one (few images
 *     per block), row_pixel is the natural order, row m = pixel m, the masks are that order's, and the layer runs the kernel
 *     without tables at this shape.  Returns 1 (class-sorted) or 0 (natural order), or a negative davo_status.
 *   tile_taps[ceil(M / 128)]: bit ky * 3 + kx is set when tap (ky, kx) is real for at least one row of that 128-row tile; the
 *     kernel walks exactly these taps for the tile.
 * davo_pad_class_tile_order: order[i], i < mtiles * ntiles_n = the tile (M tile t / ntiles_n of the launch, first M tile mtile0)
 *   that the i-th workgroup of a launch takes; the eight XCDs run the contiguous eighths of the table (the first (mtiles * ntiles_n)
 *   % 8 of them one entry longer), each with its long tiles first and all with the same work to within a tile.
 * davo_plan_layer_f32: the float32 path's launches for a layer of mtiles 128-row tiles x npad output channels on ncu compute
 *   units: launch i covers M tiles [mtile0[i], mtile0[i] + launch_mtiles[i]) at tile_bn[i] columns; returns 1 or 2.
 * The latter two return DAVO_OK (the plan: its launch count) or a negative davo_status. */
int davo_pad_class_tables(int NB, int Hout, int Wout, int Hin, int Win, int pad_t, int pad_l, int rate,
                          int* row_pixel, unsigned short* tile_taps);
int davo_pad_class_tile_order(const unsigned short* tile_taps, int mtile0, int mtiles, int ntiles_n, int* order);
int davo_plan_layer_f32(int mtiles, int npad, int groups, int ncu, int* mtile0, int* launch_mtiles, int* tile_bn);

/* Every launch decision of one conv layer on its own (no GPU needed): what a forward of NB pair images of an H x W frame issues for
 * layer 0..6 = cnv1..cnv7 through the implicit-GEMM kernels (csrc/plan.h: decide_layer_h3 for precision 1, decide_layer_f32 for 0),
 * with cnv6_out channels per head.  fuse_pose: the pose head runs in this launch's epilogue (layer 6 where the forward fuses it).
 * options[i], i < n_options <= DAVO_DECIDE_OPTIONS, in this order; the ones left out keep a new context's values.  Positions 0..13
 * are davo_option_info's rows 0..13, in stored form (what davo_option_store returns; "pad_classes" is the mask 1 cnv4 | 2 cnv5 | 4 cnv6):
 *    0 wave128          1 skip_order    2 merge_order   3 pad_classes   4 merge_rem_f32
 *    5 share_taps       6 merge_rem     7 merge_cnv4    8 tile_208x128   9 deep_ring   10 split_k   11 fold_fixup
 *   12 f32_n16         13 f32_n256     14 compute units a launch may use (256)   15 compute units of the device (256)
 *   16 cu_partition    17 a caller's stream is set     18 max_batch (1)
 *   19, 20 storage shifts of the layer's input and output (0)   21 force_tile (-1)
 *   22 the launch's last workgroup writes the poses ("fold_tails" 1; 0)   23 feature attention: cnv6 as one group per head (0)
 *   24 the three-frame PoseNN: NB windows, cnv1 at 16 packed channels (0)   25 the coupled heads: one-group cnv6 and cnv7 (0)
 * The layer's input and output (channels, map, storage) are the record davo_decide_forward reports for that layer.
 * out[0] = steps (1 or 2), then DAVO_DECIDE_STEP_INTS per step:
 *   family (0 h3 | 1 h3s | 2 h3w | 3 h3w64 | 4 h3w128 | 5 h3 merged grid | 6 h3 split-K | 7 f32 | 8 f32 n256 | 9 f32 merged grid),
 *   tile (f16x3: the planner's tile id; float32: the N tile's columns, of the remainder for a merged grid), first output row, one past the
 *   last output row, mtile0, ntiles_n, grid x, grid y, n_main, n_rem, merge order (-1: 2 where a tile-order table exists, else 0), deep,
 *   1 = profile entry "<layer>.rem", the merged grid's remainder mtile0 and ntiles_n, tile order wanted (0 none | 1 long tiles first),
 *   1 = the family's own predicate holds for the step's block, chunks of K the step walks
 * then DAVO_DECIDE_TAIL_INTS: the two davo_last_plan codes (M tiles * 1000 + tile | columns), davo_last_split, 1 = fold the split-K
 *   fix-up where the device's dispatch order allows, 1 = float32 class-sorted rows where the shape has tables, the fused pose head's tile
 *   height, M tiles and N tiles, pose-tile and split-K scratch floats per in-flight slot, the layer's f16x3 chunks of K and chunks per
 *   channel block.
 * Returns the number of ints the record holds (written up to out_cap), or a negative davo_status (DAVO_ERR_INVALID also where no tile
 * fits the fused pose head). */
#define DAVO_DECIDE_OPTIONS 26
#define DAVO_DECIDE_STEP_INTS 18
#define DAVO_DECIDE_TAIL_INTS 12
int davo_decide_layer(int precision, int layer, int H, int W, int NB, int cnv6_out, int fuse_pose, const int* options, int n_options,
                      int* out, int out_cap);

/* The launch sequence of one forward on its own (no GPU needed; csrc/plan.h: decide_forward): what a forward of B windows of an
 * H x W frame issues, in order, and what each conv layer reads and writes.
 * call[DAVO_FORWARD_CALL_INTS]: H, W, B, pair selection (1 src0 | 2 src1 | 3 both), the kernels that run (0 f16x3 | 1 float32 |
 *   2 impl 1), the variant's att_source, cnv6_out and cin_per_frame, davo_set_posenn_topology's, davo_set_posenn_heads' and
 *   davo_set_posenn_se's values.
 * options[i], i < n_options <= DAVO_FORWARD_OPTIONS, in this order; the ones left out keep a new context's values.  Positions 0..6
 * are davo_option_info's rows 14..20, in stored form:
 *    0 fold_tails   1 fuse_pack   2 fuse_pose   3 patch_cnv1_t   4 patch_cnv2   5 patch_cnv3   6 patch_f32
 *    7 force_tile (-1)   8 the batch's first kernel zeroes its range record's per-batch word (a ticketed batch; 0)
 *    9 the batch's last kernel mirrors the range record and keeps the inputs where it fails (every f16x3 batch of an entry point; 0)
 * out: DAVO_FORWARD_HEAD_INTS - images through cnv1..cnv7; the attention front: kind (0 flow | 1 flow, depth-split | 2 class table |
 *   3 depth | 4 pooled), 1 = a squeeze launch, 1 = the excitation folded into it, 1 = se_excite follows, 1 = se_excite_far follows, the
 *   label of the launch that zeroes the record (-1 none); the packer: 0 none (fused into cnv1) | 1 pair | 2 three-frame, its ld (16 | 8 |
 *   10), the packed tensor's channels as davo_debug_read sizes it, 1 = it is in memory; 1 = se5_squeeze / se5_excite / se5_scale sit
 *   between cnv5 and cnv6; the head: 0 written by cnv7's launch | 1 pose_from_tiles | 2 two passes, its pred columns and heads, 1 = the
 *   range guard's snapshot is a launch of its own, 1 = cnv7 is stored -
 * then DAVO_FORWARD_LAYER_INTS per layer cnv1..cnv7: runner (0 patch | 1 patch with mask + pack fused in | 2 three-frame cnv1 patch |
 *   3 f16x3 implicit GEMM | 4 float32 implicit GEMM | 5 direct), label, input buffer (-1 packed | -2 the SE-scaled cnv5 | i = layer i's
 *   output), its channels, rows and columns, the output's channels per pixel, rows and columns, 1 = float32 output, fuse_pose, pose_tail,
 *   pose_six, davo_last_plan's code (patch runners; 0 = davo_decide_layer has it), impl 1's groups, input and output channels per group
 *   and the two groups' input and output channel offsets -
 * then the number of launches and their labels in issue order, as indices into DAVO_FORWARD_LABELS (a conv layer once, whatever
 * davo_decide_layer splits it into; the last label has no profile entry).
 * Returns the number of ints the record holds (written up to out_cap), or a negative davo_status: DAVO_ERR_INVALID for bad arguments
 * and for every combination the forward itself refuses. */
#define DAVO_FORWARD_LABELS {"se_pool_squeeze", "se_pool_excite", "se_depth_squeeze", "se_class_squeeze", "se_squeeze_partial", "se_excite", \
                             "se_excite_far", "mask_pack", "cnv1", "cnv2", "cnv3", "cnv4", "cnv5", "se5_squeeze", "se5_excite", "se5_scale", \
                             "cnv6", "cnv7", "pose_head", "range_guard_snapshot"}
#define DAVO_FORWARD_CALL_INTS 11
#define DAVO_FORWARD_OPTIONS 10
#define DAVO_FORWARD_HEAD_INTS 17
#define DAVO_FORWARD_LAYER_INTS 21
int davo_decide_forward(const int* call, const int* options, int n_options, int* out, int out_cap);

#ifdef __cplusplus
}
#endif
#endif /* DAVO_HIP_H */

// launch.h — the kernel launch functions, one translation unit per kernel family so the device
// code compiles in parallel.  Each launcher sets the dynamic-LDS attribute of its kernel once per
// (device, kernel) and returns the launch's error.
#pragma once
#include <hip/hip_runtime.h>

#include "params.h"
#include "plan.h"

namespace davo {

// hipFuncAttributeMaxDynamicSharedMemorySize for `kernel` on the CURRENT device, set once per (device, kernel):
// a function attribute belongs to the device's code object, so a second context on another GPU of the same
// process needs its own call (launch_misc.hip).
hipError_t ensure_dynamic_lds(const void* kernel, int bytes);

// ---- launch_f32.hip: conv_igemm_f32 (FP32 MFMA, bit-exact fmaf chains) ---------------------------
// generic shapes (davo_conv2d_same and non-default cnv6 widths)
hipError_t launch_conv(int KS, int stride, int BN, const ConvParams& p, dim3 grid, hipStream_t s);
// the seven PoseNN layers (layer 0..6 = cnv1..cnv7), each under its own kernel name; BN is chosen per launch
hipError_t launch_layer(int layer, int BN, const ConvParams& p, dim3 grid, hipStream_t s);
hipError_t launch_layer_n256(int layer, const ConvParams& p, dim3 grid, hipStream_t s);
hipError_t launch_layer_mainrem(int layer, int rbn, const ConvParams& pm, const ConvParams& pr, int n_main, int n_rem, int groups, hipStream_t s);

// ---- launch_h3.hip: conv_igemm_h3 (f16x3) -----------------------------------------------------------
hipError_t launch_layer_h3(int layer, int tile, const ConvParamsH& p, dim3 grid, hipStream_t s);
// main launch (256x256 tiles, shared-tap staging) + remainder launch (128x128 tiles) of cnv5 / cnv6 (layer 4 / 5) as one grid
// (conv_igemm_h3_mainrem), or 256x128 + 128x128 of cnv4 (layer 3).  Not supported where the two launches do not have that shape
// or the layer's padded Cout is narrower than the instantiation's main tile (a -cnv6_64 cnv6 has 128 columns): such a layer keeps its two launches
bool layer_h3_mainrem_supported(int layer, const ConvParamsH& pm, int n_main, int n_rem);
// order: 0 = the short tiles' offset inside every XCD (round 2), 1 = per XCD (even XCDs short tiles first, odd XCDs last)
hipError_t launch_layer_h3_mainrem(int layer, const ConvParamsH& pm, int n_main, const ConvParamsH& pr, int n_rem, int order, hipStream_t s);
// launch_h3s.hip: conv_igemm_h3s (TILE_208x256) for layer 4..6 = cnv5, cnv6, cnv7
hipError_t launch_layer_h3s(int layer, const ConvParamsH& p, dim3 grid, hipStream_t s);
// conv_igemm_h3w.h: 256x256 tiles on four waves of 128x128 (cnv5, cnv6; option "wave128")
// the *_supported predicates read geometry fields only: decide_layer_h3 (plan.hip) asks them, so no launch is ever tried; a launcher's
// own hipErrorNotSupported is an assertion of last resort (forward.hip reports it as an internal error)
bool layer_h3w_supported(int layer, const ConvParamsH& p);
hipError_t launch_layer_h3w(int layer, const ConvParamsH& p, dim3 grid, hipStream_t s);
bool layer_h3w128_supported(const ConvParamsH& p);
hipError_t launch_layer_h3w128(const ConvParamsH& p, hipStream_t s);      // cnv4: 256x128 tiles, p.mtile0 in 256-row tiles
bool layer_h3w64_supported(int layer, const ConvParamsH& p);
hipError_t launch_layer_h3w64(int layer, const ConvParamsH& p, hipStream_t s);      // remainder rows: 256x64 tiles, p.ntiles_n = 4, p.mtile0 in 256-row tiles
hipError_t launch_h3_generic(int KS, int stride, int tile, const ConvParamsH& p, dim3 grid, hipStream_t s);

// ---- launch_misc.hip: prologue, pose head, cnv1 patch kernel, direct convolution ---------------------
// fmt (here and below): the context's input format (params.h) - what d_flow, d_seg and d_depth point at.  A launcher picks its kernel's
// element types from it through input_types.h; a value that names no element type of a plane kind the kernel reads is an error
// the four dense tensors of an SE block in the reference's [in,out] layout: bottleneck kernel and bias, recover kernel and bias
struct SeDense {
    const float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
    explicit operator bool() const { return w1 && b1 && w2 && b2; }
};
hipError_t launch_se_squeeze(const void* d_flow, const InputFormat& fmt, int B, int HW, const Variant& v, float* d_partial, int sel, hipStream_t s);
hipError_t launch_se_excite(const float* d_partial, int B, int HW, const Variant& v, const SeDense& w, const float* wstatic, float* d_tab,
                            unsigned* d_range_reset, int sel, hipStream_t s);
// squeeze + excitation in one launch: the last workgroup of each triplet evaluates its tables (prologue.h, pose_tail.h);
// -> 1 if the parts (x, 0..3) of a 64 x 4 grid ran on one XCD each for every x (what the folded split-K fix-up relies on), 0 if not
hipError_t xcd_round_robin_probe(hipStream_t s, int* ok);
// d_counters: one zeroed unsigned per triplet, left at zero
hipError_t launch_se_squeeze_excite(const void* d_flow, const InputFormat& fmt, int B, int HW, const Variant& v, float* d_partial, unsigned* d_counters,
                                    const SeDense& w, const float* wstatic, float* d_tab, unsigned* d_range_reset, int sel, hipStream_t s);
// att_source 13: the same launch with both excitations in the last workgroup - near / far = the dense tensors of se_flow_near /
// se_flow_far, d_tab the near tables, d_tab_far the far ones
hipError_t launch_se_squeeze_excite_split(const void* d_flow, const InputFormat& fmt, int B, int HW, const Variant& v, float* d_partial, unsigned* d_counters,
                                          const SeDense& near, const SeDense& far, float* d_tab, float* d_tab_far,
                                          unsigned* d_range_reset, int sel, hipStream_t s);
// segmentation / rgb / seg+flow class-table sources (att_source 4..10): per-frame descriptor records into d_partial (max_batch x 3 x SQ_CHUNKS x SQ_REC words);
// fold: the triplet's last workgroup evaluates its tables too (d_counters as above), otherwise launch_se_excite follows.
hipError_t launch_se_class_squeeze(bool fold, const uint8_t* d_img, const void* d_flow, const void* d_seg, const InputFormat& fmt, int B, int H, int W,
                                  const Variant& v, unsigned* d_partial, unsigned* d_counters, const SeDense& w, float* d_tab,
                                  unsigned* d_range_reset, int sel, hipStream_t s);
// depth sources (att_source 11, 12): one float32 sum per (triplet, frame, chunk) into word 0 of the same records; d_depth is
// [B][3][H][W] in file order (src0, tgt, src1), 16-byte aligned, in the format's depth element; fold as above
hipError_t launch_se_depth_squeeze(bool fold, const void* d_depth, const InputFormat& fmt, int B, int HW, const Variant& v, unsigned* d_partial,
                                   unsigned* d_counters, const SeDense& w, float* d_tab, unsigned* d_range_reset, int sel, hipStream_t s);
// pooled flow-attention variants (att_source 14..17; se_pool.h): window sums into d_partial [B][2][pd.n_items][2], then the excitation
// (one launch each; "fold_tails" does not apply) -> d_tab [B][3][19] and the descriptor d_desc [B][2][2 pd.n_cells]
hipError_t launch_se_pool_squeeze(const void* d_flow, const InputFormat& fmt, int B, int H, int W, const Variant& v, const PoolDev& pd, float* d_partial,
                                  int sel, hipStream_t s);
hipError_t launch_se_pool_excite(const float* d_partial, int B, const Variant& v, const PoolDev& pd, const SeDense& w, float* d_tab, float* d_desc,
                                 unsigned* d_range_reset, int sel, hipStream_t s);
// ld: 16 = split-fp16 8-channel layout (f16x3), 8 = float32 8-channel, 10 = the reference's 10-channel layout
// att_source 13 (the depth-split flow attention) runs the depth-split form: d_depth (16-byte aligned, in the format's depth element), the
// far tables and the threshold are required there and ignored everywhere else (a caller with none passes nullptr, nullptr, 0.f)
hipError_t launch_mask_pack(int ld, const uint8_t* d_img, const void* d_flow, const void* d_seg, const InputFormat& fmt, const float* d_tab,
                            const Variant& v, int B, int H, int W, float* d_packed, int sel, hipStream_t s,
                            const void* d_depth, const float* d_tab_far, float depth_thr);
// the three-frame PoseNN's packer (prologue.h, mask_pack3): B windows -> [B][H][W][16], float32 or (h3) split-fp16 [16 hi | 16 lo]
hipError_t launch_mask_pack3(bool h3, const uint8_t* d_img, const void* d_flow, const void* d_seg, const InputFormat& fmt, const float* d_tab,
                             const Variant& v, int B, int H, int W, float* d_packed, hipStream_t s);
// window_gather.h: N windows of a frame-layout batch into the window-major planes every kernel above reads; every pointer 16-byte
// aligned; a.f_flow null = the flow planes are in place already (the host entry points copy them there)
struct GatherArgs;
hipError_t launch_window_gather(const GatherArgs& a, int N, const InputFormat& fmt, hipStream_t s);
// window_mirror.h: N windows mirrored left-right (davo_set_flip).  frames: the gather above with mirrored stores, a's meaning
// unchanged; else a.f_* are window-major like a.w_* - the same pointers (in place) or a caller's buffers - and a.f_flow is required.
// a.seg_tgt: the target's label map is read at all.  Every pointer 16-byte aligned
hipError_t launch_window_mirror(const GatherArgs& a, int N, bool frames, const InputFormat& fmt, hipStream_t s);
// cnv1 / cnv2 / cnv3 (layer 0..2) from an LDS-staged input patch: conv_patch_cnvN_h3, or conv_patch_cnvN_f32 in float32 mode (f32);
// fused: conv_patch_cnv1_h3<true, float | uint8_t, float | in_f16> by fmt's label and flow elements (f16x3 cnv1 only; p.seg and p.flow are in those formats);
// cnv1t (f16x3 cnv1 only): conv_patch_cnv1t_h3 of the three-frame PoseNN - p.x the 16-channel split-fp16 packed tensor, p.w cp1t::WBYTES of fragments
hipError_t launch_patch_layer(int layer, bool f32, bool fused, bool cnv1t, const ConvPatchParams& p, int nblk, hipStream_t s, const InputFormat& fmt);
// split-K fix-up: d_part [M][S][N] float32 partial sums -> the layer's stored activation (ReLU, fp16 hi/lo pairs, range monitor)
hipError_t launch_splitk_fixup(const float* d_part, long M, int N, int S, int relu, uint8_t* d_y, unsigned* d_range, hipStream_t s);
hipError_t launch_pose_from_tiles(const float* d_tiles, int NB, int P, int bm, int mtiles, int ntiles_n,
                                  const float* d_bpred, float* d_pose, const SnapArgs& snap, int sel, hipStream_t s);
// the range guard's conditional copy of the batch's inputs as a launch of its own (prologue.h)
hipError_t launch_range_guard_snapshot(const SnapArgs& snap, hipStream_t s);
// the two-pass pose head on a stored cnv7 (pose_head_partial + pose_finish), by pred columns and heads:
//   (3, 2) the pair network: d_c7 [NB][P][512], d_wpred [2][256][3] -> d_partial [NB][2][PH_SPLIT][3]
//   (6, 2) the three-frame PoseNN: NB = B windows, d_c7 [B][P][512], d_wpred [2][256][6], d_bpred [2][6], d_partial [B][2][PH_SPLIT][6]; sel is not read
//   (6, 1) the coupled network: d_c7 [NB][P][256], d_wpred [256][6], d_bpred [6], d_partial [NB][PH_SPLIT][6]
// -> d_pose [B][2][6]; any other (cols, heads) is an error
hipError_t launch_pose_head(int cols, int heads, const float* d_c7, int NB, int P, const float* d_wpred, const float* d_bpred,
                            float* d_partial, float* d_pose, int sel, hipStream_t s);
hipError_t launch_conv_direct(const float* x, int N, int Hin, int Win, int cin, int x_ld, int x_coff, const float* w, int KS,
                              int cout, const float* bias, int stride, int rate, int pt, int pl, int Ho, int Wo, int relu,
                              float* y, int y_ld, int y_coff, hipStream_t s);
// the feature-attention variant's SE block on cnv5 (posenn_se.h): squeeze, excite, scale.  h3: x and y are split-fp16 blocked
// (else float32 NHWC); P = pixels per pair image; d_partial [NB][SE5_CHUNKS][256], d_scale [NB][2][256] (s_r | s_r * s_t),
// d_y [NB][P][512]; rot, trans: the dense tensors of rotation's and translation's block; unscale = 2^-(cnv5's storage shift)
hipError_t launch_se5_squeeze(bool h3, const void* d_x, int NB, int P, float* d_partial, hipStream_t s);
hipError_t launch_se5_excite(const float* d_partial, int NB, int P, float unscale, const SeDense& rot, const SeDense& trans, float* d_scale, hipStream_t s);
hipError_t launch_se5_scale(bool h3, const void* d_x, const float* d_scale, int NB, int P, void* d_y, unsigned* d_range, hipStream_t s);

// ---- launch_feature.hip: the feature export (feature_export.h; davo_forward_features) -----------------------------
// one piece of nw windows: d_img / d_seg / d_tab point at the piece's first window; outputs [3][nw][19], [3][nw][H][W], [3][nw][H][W][3] x 2,
// frames in the order tgt, src0, src1; a null output is not written
hipError_t launch_feature_maps(const uint8_t* d_img, const void* d_seg, const InputFormat& fmt, const float* d_tab, const Variant& v, int nw, int H, int W,
                               float* d_att_19, float* d_attention, float* d_masked, float* d_image, hipStream_t s,
                               const void* d_depth, const float* d_tab_far, float depth_thr);      // att_source 13: as launch_mask_pack
// d_cnv6: the whole stored cnv6 of a both-pairs forward (h3: f16x3 blocked, scaled by 1 / unscale; else float32 NHWC); windows
// [w0, w0 + nw) of it -> d_rot / d_trans [nw][4 H2][4 W2][c6]; a null head is not computed
hipError_t launch_feature_resize_cnv6(bool h3, const void* d_cnv6, int w0, int nw, int H2, int W2, int c6, float unscale,
                                      float* d_rot, float* d_trans, hipStream_t s);
// the heat export (davo_forward_heat) of the same windows: per head the channel sum of the stored cnv6 -> d_sum_* [nw][H2][W2], the
// block's maximum -> d_max_* [nw] (zeroed here, then raised as bit patterns), and the resize of the sum -> d_plane_* [nw][4 H2][4 W2].
// A head is computed when its sum and max are given; its plane may be null (the maximum alone is wanted)
hipError_t launch_feature_heat(bool h3, const void* d_cnv6, int w0, int nw, int H2, int W2, int c6, float unscale,
                               float* d_sum_rot, float* d_sum_trans, float* d_max_rot, float* d_max_trans,
                               float* d_plane_rot, float* d_plane_trans, hipStream_t s);

}  // namespace davo

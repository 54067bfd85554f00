// plan.h — launch planning of the convolution layers: which tile shape, how a layer is split
// into a main launch of whole rounds plus a remainder launch, and which kernel family each launch
// runs on (LayerDecision, below), and the launch sequence of a whole forward (ForwardPlan, at the end).
// Pure host logic (plan.hip); the test hooks davo_plan_layer, davo_decide_layer and davo_decide_forward
// (include/davo_hip.h) expose it to the CPU test-suite.
#pragma once
#include <vector>

#include "options.h"
#include "params.h"

namespace davo {

// Tuning knobs (environment variables, the measurement-only `dbg` bits of the kernels) exist only in a
// -DDAVO_TUNING build (tools/build_variant.py); the product library reads no environment.
#ifdef DAVO_TUNING
const char* tuning_env(const char* name);
#else
inline const char* tuning_env(const char*) { return nullptr; }
#endif

// ---- FP32-MFMA path (conv_igemm.h): 128-row M tiles x BN ---------------------------------------
struct Launch { int mtile0, mtiles, BN; };
// ncu: compute units the launch may use (256 = the whole MI355X; fewer when the context's stream is CU-masked)
std::vector<Launch> plan_layer(int mtiles, int npad, int groups, int ncu = 256);

// ---- f16x3 path (conv_igemm_h3.h) -----------------------------------------------------------------
// tile id -> (WM, WN, TM, TN): BM = WM*TM*32, BN = WN*TN*32, threads = WM*WN*64
// TILE_208x256 is conv_igemm_h3s.h (waves split the channels; whole rounds for the PoseNN's 16x208-pixel feature maps)
// 7 is not a tile: davo_last_plan reports it for the merged main + remainder grid.  TILE_208x128 (round 4): the four-wave conv_igemm_h3s for cnv4
enum { TILE_128x32 = 0, TILE_256x64 = 1, TILE_256x128 = 2, TILE_128x256 = 3, TILE_128x128 = 4, TILE_256x256 = 5, TILE_208x256 = 6, TILE_MERGED_MARK = 7, TILE_208x128 = 8, NUM_TILES = 9 };
inline bool is_208(int t) { return t == TILE_208x256 || t == TILE_208x128; }
struct TileShape { int bm, bn, threads, lds; };
TileShape tile_shape(int t);
// rows of a layer's packed f16x3 weights and bias per group: Cout padded to the widest N tile a launch may use.
// The packers' allocation (weights.hip, L.npad_h) and the merged grid's bound on its main tile (launch_h3.hip, mainrem_ok) both
// call this: the bound holds only while the allocation comes from the same function.
inline int h3_npad(int cout) {
    const int gran = cout > 128 ? 256 : cout > 64 ? 128 : cout > 32 ? 64 : 32;
    return (cout + gran - 1) / gran * gran;
}

struct TileInfo { int id, per_cu; double eff; };
struct LaunchH { int row0, rows, tile; };
double h3_cost(const TileInfo& t, long ntiles, int ncu = 256);
const TileInfo* h3_tiles(int* n);
// main launch + optional remainder launch for an M x npad (x groups) layer; forced_tile >= 0: one launch of that tile
// allow_208: the layer has a conv_igemm_h3s instantiation for its width (3x3, Cin >= 32: cnv5, cnv6, cnv7 at 256 output channels
// per group -> TILE_208x256; cnv4 at 128 -> TILE_208x128)
// others_scale: the efficiencies of every tile but 256x256 are multiplied by it (cnv5 / cnv6 with "wave128": their 256x256 launches run
// on conv_igemm_h3w, 4.7 % faster than the kernel the table was fitted on)
std::vector<LaunchH> plan_layer_h3(int M, int npad, int groups, int forced_tile, bool allow_208 = false, int ncu = 256, double others_scale = 1.0);
// one launch, one tile shape no taller than max_bm rows (fused pose head: a tile touches <= 2 images); -1 if none fits
int plan_single_tile_h3(int M, int npad, int groups, int max_bm, int forced_tile, bool allow_208 = false, int ncu = 256);
// "force_tile" (davo_set_option) / DAVO_H3_TILE for a layer of cout output channels: the tile where it fits, else -1 = the planner picks
inline int forced_tile_h(int value, int cout) { return (value >= 0 && value < NUM_TILES && cout >= tile_shape(value).bn) ? value : -1; }

// ---- a layer's launches, decided before anything is issued ---------------------------------------------------------------------
// decide_layer_h3 / decide_layer_f32 are pure functions of a layer's host geometry, the call and a copy of the context's options: no
// device pointer goes in or comes out, no HIP call is made.  forward.hip issues what they return (one issuer per precision);
// davo_decide_layer (hooks.hip) shows it to the CPU test-suite.  DESIGN.md section 6 lists the rules in order with their measurements.

// TF `SAME` padding (SURVEY.md note P): out = ceil(in/stride), pad_before = total // 2
inline void same_pad(int in, int k, int stride, int rate, int* out, int* before) {
    const int o = (in + stride - 1) / stride;
    const int keff = (k - 1) * rate + 1;
    int total = (o - 1) * stride + keff - in;
    if (total < 0) total = 0;
    *out = o;
    *before = total / 2;
}
inline int ilog2_exact(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return (1 << l) == v ? l : -1;
}

constexpr int SK_TILE_COUNTERS = 256;            // tiles of a split-K launch whose fix-up is folded in: at most one per CU

// the host fields of a layer (ctx.h: ConvLayer adds the label and the device copies); init_layer (weights.hip) fills them
struct LayerGeom {
    int KS = 0, stride = 0, rate = 0;
    int cin = 0, cin_log2 = 0, cout = 0;       // packed input channels per tap (power of two), valid outputs
    int BN = 0, npad = 0, kpad = 0, nchunks = 0, groups = 0;
    // f16x3 path (conv_igemm_h3.h): channel-blocked k order, split-fp16 packed weights
    int cb_log2 = 0, tpc_log2 = 0, cpb = 0, nchunks_h = 0, npad_h = 0;
    int tile_h = 0;                            // -1: the planner picks per launch; a tile id: "force_tile" / DAVO_H3_TILE (forced_tile_h)
    float wscale = 1.f;                        // power of two the packed fp16 weights are multiplied by
};
// x_ch: channels of the input tensor (f16x3: of the whole blocked tensor; float32: floats per pixel); pose_tail: the launch's last
// workgroup adds the pose tiles and writes the poses (f16x3 with fuse_pose only)
// pose_six (f16x3 with fuse_pose, a one-group cnv7): the coupled network's six-column head - the NC = 6 epilogue of conv_igemm_h3.h, its
// partial sums in the two-head layout, no 208-pixel tile (conv_igemm_h3s.h has the three-column epilogue alone)
struct LayerCall { int li, x_ch, Hin, Win, y_ld; bool y_f32; int NB; bool fuse_pose, pose_tail; bool pose_six = false; };
// the context's settings these decisions read: its launch options (options.h), davo_ctx's ncu, dev_cus, cu_partition, user_stream and
// max_batch, and the storage shifts of the layer's input and output (act_shift[li - 1], 0 for cnv1; act_shift[li])
struct PlanOptions : LaunchOptions {
    int ncu = 256, dev_cus = 256;
    bool cu_partition = false, user_stream = false;
    int max_batch = 1, shift_in = 0, shift_out = 0;
};

// kernel families: which launcher of launch.h a step goes to
enum { FAM_H3 = 0, FAM_H3S = 1, FAM_H3W = 2, FAM_H3W64 = 3, FAM_H3W128 = 4, FAM_H3_MAINREM = 5, FAM_H3_SPLITK = 6,
       FAM_F32 = 7, FAM_F32_N256 = 8, FAM_F32_MAINREM = 9, NUM_FAMILIES = 10 };
const char* family_name(int family);
// the tile-order table a parameter block wants (forward.hip builds, uploads and caches it): none, long tiles first under the cache
// key `key' (tile_order_for), or - float32 layers on class-sorted rows - the padding classes' order where the shape has class tables
// and long-first otherwise
enum { ORDER_NONE = 0, ORDER_LONG_FIRST = 1 };
struct OrderRequest { int kind = ORDER_NONE, key = 0, bm = 0, mtile0 = 0, mtiles = 0, ntiles_n = 0; };
// One launch.  p[0] is its parameter block, every pointer null; merged grids carry the remainder's block in p[1].
// tile: the planner's tile id (f16x3; FAM_H3W64 runs those rows on 256x64 tiles) or the N tile's columns (float32; merged grid: the remainder's).  row0: first output row of the step
// (its last is p[nblocks - 1].M - 1, for float32 m_end - 1).  order (f16x3 merged grid): the merge order, -1 = 2 where p[0] gets a
// tile-order table, else 0.
template <class P>
struct LaunchStep {
    int family = FAM_H3, tile = 0, nblocks = 1;
    P p[2] = {};
    OrderRequest ord[2];
    unsigned gx = 0, gy = 1;
    int row0 = 0, m_end = 0, n_main = 0, n_rem = 0, order = 0;
    bool rem_label = false;                    // profile entry "<layer>.rem" instead of "<layer>"
};
template <class P>
struct LayerDecision {
    int err = 0;                               // DAVO_OK, or a davo_status with msg
    const char* msg = nullptr;
    int nsteps = 0;
    LaunchStep<P> steps[2];
    int plan_code[2] = {0, 0}, split = 1;      // davo_last_plan (M tiles of 128 rows * 1000 + tile | columns), davo_last_split
    // split-K (steps[0] is FAM_H3_SPLITK): split parts write float32 partial sums [sk_M][split][sk_cout]; fold_if_xcd: the fix-up runs
    // in the launch's last part per tile where the device deals a grid's parts out per XCD (xcd_round_robin_probe), on the tile
    // counters from sk_counter0
    long sk_M = 0;
    int sk_cout = 0, sk_counter0 = 0;
    bool fold_if_xcd = false;
    bool pad_classes = false;                  // float32: the layer runs on class-sorted rows where the shape has tables (pad_classes.h)
    // per-slot scratch (floats): the fused pose head's tile sums (+ bytes behind every slot's, DAVO_POSE_DEBUG), split-K partial sums
    size_t pose_floats = 0, pose_debug_bytes = 0, splitk_floats = 0;
    int pose_bm = 0, pose_mt = 0, pose_ntn = 0;      // fused pose head: tile height, M tiles, N tiles of the launch
};
// the parameter blocks of a whole layer as one launch at mtile0 = 0, every pointer null (davo_conv2d_same fills its own from them)
ConvParamsH fill_params_h3(const LayerGeom& L, const LayerCall& call, bool share_taps, int shift_in, int shift_out);
ConvParams fill_params_f32(const LayerGeom& L, const LayerCall& call);
LayerDecision<ConvParamsH> decide_layer_h3(const LayerGeom& L, const LayerCall& call, const PlanOptions& o);
LayerDecision<ConvParams> decide_layer_f32(const LayerGeom& L, const LayerCall& call, const PlanOptions& o);

// ---- a forward's launches, decided before anything is issued -------------------------------------------------------------------
// decide_forward is to the whole forward what decide_layer_* are to a layer: a pure function of plain values - no context, no
// device pointer, no HIP call, no allocation - that returns the launch sequence as one fixed-size record.  forward.hip walks it
// (run_front, run_layers, run_head: issuing only); davo_decide_forward (hooks.hip) shows it to the CPU test-suite, and
// davo_decide_layer takes its LayerCall from the same records.  The map ladder H, H/2, H/4, ..., H/8 and the channel ladder
// 8|16, 16, 32, 64, 128, 256|512, cnv6's width, 256|512 are written down in decide_forward and nowhere else.
enum { MODE_H3 = 0, MODE_F32 = 1, MODE_DIRECT = 2 };      // the kernels that really run: f16x3, float32 MFMA, impl 1's direct convolution
struct ForwardCall {
    int H = 0, W = 0, B = 0, pairs = PAIRS_BOTH, mode = MODE_H3;
    Variant v{};
    bool triplet = false, coupled = false;     // davo_set_posenn_topology, davo_set_posenn_heads
    int posenn_se = 0;                         // davo_set_posenn_se
    int groups6 = 1, groups7 = 2, cin7 = 0;    // cnv6's and cnv7's groups and cnv7's input channels per group, as the layers were initialised
};
// the settings the sequence reads (the context's launch options, L[i].tile_h, the float32 patch weights, L[6].npad), the batch's two
// range-guard wishes (Run::zero_record, Run::snap.record) and the tuning build's DAVO_FUSE_PACK / DAVO_CNV{1,2,3}_PATCH (-1: not set)
struct ForwardOptions : LaunchOptions {
    bool forced_tile[7] = {false, false, false, false, false, false, false};
    bool have_patch_f32[3] = {true, true, true};
    int npad7 = 256;
    bool zero_record = false, want_snapshot = false;
    int env_fuse_pack = -1, env_patch[3] = {-1, -1, -1};
};
// the profile labels of a forward's launches, as indices into DAVO_FORWARD_LABELS (include/davo_hip.h; plan.hip holds the two to one length)
enum { LB_SE_POOL_SQUEEZE = 0, LB_SE_POOL_EXCITE, LB_SE_DEPTH_SQUEEZE, LB_SE_CLASS_SQUEEZE, LB_SE_SQUEEZE_PARTIAL, LB_SE_EXCITE, LB_SE_EXCITE_FAR,
       LB_MASK_PACK, LB_CNV1, LB_CNV2, LB_CNV3, LB_CNV4, LB_CNV5, LB_SE5_SQUEEZE, LB_SE5_EXCITE, LB_SE5_SCALE, LB_CNV6, LB_CNV7, LB_POSE_HEAD,
       LB_SNAPSHOT, NUM_LABELS };
enum { FRONT_FLOW = 0, FRONT_FLOW_SPLIT = 1, FRONT_CLASS = 2, FRONT_DEPTH = 3, FRONT_POOLED = 4 };
enum { PACK_NONE = 0, PACK_PAIR = 1, PACK_TRIPLET = 2 };      // none: mask + pack run inside cnv1's patch fill
enum { RUN_PATCH = 0, RUN_PATCH_FUSED = 1, RUN_PATCH_CNV1T = 2, RUN_IGEMM_H3 = 3, RUN_IGEMM_F32 = 4, RUN_DIRECT = 5 };
enum { BUF_PACKED = -1, BUF_SE = -2 };                        // a layer's input: the packed tensor, the SE-scaled cnv5, else act[i]
enum { HEAD_TAIL = 0, HEAD_TILES = 1, HEAD_TWO_PASS = 2 };    // the poses come out of cnv7's launch | pose_from_tiles | pose_head_partial + pose_finish
struct LayerPlan {
    int runner = RUN_IGEMM_H3, label = LB_CNV1;
    int x_buf = BUF_PACKED, x_ch = 0, Hin = 0, Win = 0;       // x_ch as LayerCall's: channels of the whole input tensor
    int y_ld = 0, Hout = 0, Wout = 0;                         // the output is act[layer], y_ld channels per pixel
    bool y_f32 = false, fuse_pose = false, pose_tail = false, pose_six = false;
    int plan_code = 0;                                        // patch runners: davo_last_plan's code (the igemm layers' come from decide_layer_*)
    // impl 1: the layer runs once per group g < ngroups, cin channels from offset x_coff[g] of the input to cout at y_coff[g] of the output
    int ngroups = 1, cin = 0, cout = 0, x_coff[2] = {0, 0}, y_coff[2] = {0, 0};
};
struct ForwardPlan {
    int err = 0;                               // DAVO_OK, or a davo_status with msg: an internal refusal, nothing is issued
    char msg[160] = {0};
    int mode = MODE_H3, NB = 0;                // the call's mode; images through cnv1..cnv7
    struct { int kind = FRONT_FLOW; bool squeeze = false, fold_excite = false, excite = false, excite_far = false; int reset_at = -1; } front;
    struct { int kind = PACK_PAIR, ld = 16, packed_ld = 8; bool packed_valid = true; } pack;
    LayerPlan layer[7];
    bool se5 = false;                          // feature attention: se5_squeeze, se5_excite, se5_scale between cnv5 and cnv6
    struct { int kind = HEAD_TWO_PASS, cols = 3, heads = 2; bool snapshot_launch = false, cnv7_valid = true; } head;
    int nlaunch = 0, launch[24] = {0};         // the launches in issue order (LB_*; a conv layer once, whatever decide_layer_* splits it into)
};
ForwardPlan decide_forward(const ForwardCall& call, const ForwardOptions& o);
const char* forward_label(int label);          // the profile entry of an LB_*
inline LayerCall layer_call(const ForwardPlan& p, int li) {
    const LayerPlan& r = p.layer[li];
    return LayerCall{li, r.x_ch, r.Hin, r.Win, r.y_ld, r.y_f32, p.NB, r.fuse_pose, r.pose_tail, r.pose_six};
}

}  // namespace davo

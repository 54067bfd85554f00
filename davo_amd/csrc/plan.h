// plan.h — launch planning of the convolution layers: which tile shape, how a layer is split
// into a main launch of whole rounds plus a remainder launch, and which kernel family each launch
// runs on (LayerDecision, below).  Pure host logic (plan.hip); the test hooks davo_plan_layer and
// davo_decide_layer (include/davo_hip.h) expose it to the CPU test-suite.
#pragma once
#include <vector>

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
// the context's settings these decisions read (davo_ctx: opt_*, ncu, dev_cus, cu_partition, user_stream, max_batch) and the storage
// shifts of the layer's input and output (act_shift[li - 1], 0 for cnv1; act_shift[li])
struct PlanOptions {
    int wave128 = 2, skip_order = 1, merge_order = -1, pad_classes = 7, merge_rem_f32 = 1;
    bool share_taps = true, merge_rem = true, merge_cnv4 = false, tile_208x128 = false, deep_ring = true, split_k = true, fold_fixup = false;
    bool f32_n16 = true, f32_n256 = false;
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

}  // namespace davo

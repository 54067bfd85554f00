// options.h — the launch options of a context (include/davo_hip.h: davo_set_option): every option once, with its default, and one
// table row per option that names it, points at its field and says how a caller's value becomes the stored one.  davo_ctx holds one
// LaunchOptions; PlanOptions and ForwardOptions (plan.h) carry a copy; davo_set_option, davo_get_option, davo_option_info,
// davo_option_store and the option slots of davo_decide_layer / davo_decide_forward all walk the table.  Host code only.
#pragma once
#include <cstring>

namespace davo {

constexpr int PAD_CLASS_LAYERS = 6;              // "pad_classes" 1: cnv5 | cnv6 (bits: 1 cnv4, 2 cnv5, 4 cnv6).  cnv4 measured level (245.2 -> 243.4 us, inside its run-to-run spread) and stays on the natural order

// The stored values.  Switches are 0 | 1.
struct LaunchOptions {
    int wave128 = 2;                           // f16x3: cnv5 / cnv6 256x256 tiles on four waves of 128x128 outputs (conv_igemm_h3w.h: -3..5 % per step, bit-identical); 2: their remainder rows on 256x64 tiles too (-1.2 %); 3: cnv4 on conv_igemm_h3w128 whatever the round count (test hook)
    int skip_order = 1;                        // launches whose tiles skip different numbers of padding rows of the filter hand out the long tiles first (tile_order_for, forward.hip): 0 = never, 1 = float32 launches, 2 = the f16x3 merged grids too
    int merge_order = -1;                      // merged grids: 0 = short tiles offset inside every XCD, 1 = per XCD, 2 = main tiles (long first) then the remainder; -1 = 2 where a tile order exists, else 0
    int pad_classes = PAD_CLASS_LAYERS;        // float32: the layers of the mask (1 cnv4, 2 cnv5, 4 cnv6) run on rows sorted by padding class, every tile walks only the taps that are real for its own pixels (pad_classes.h)
    int merge_rem_f32 = 1;                     // f32 mode: cnv4..cnv7 main + remainder launches as one grid (conv_igemm_f32_mainrem)
    int share_taps = 1;                        // f16x3: cnv3..cnv6 stage one pixel patch per filter row for its three taps
    int merge_rem = 1;                         // f16x3: cnv5 / cnv6 main + remainder launches as one grid (conv_igemm_h3_mainrem)
    int merge_cnv4 = 0;                        // f16x3: cnv4 as whole rounds of 256x128 tiles + 128x128 remainder tiles in one grid where the batch allows
    int tile_208x128 = 0;                      // f16x3: cnv4 may run on the four-wave 208x128 tile (conv_igemm_h3s.h; measured 8 % behind the 128x128 tile at B = 32: off)
    int deep_ring = 1;                         // f16x3: launches of at most one workgroup per CU (batch 1..4) run on LDS rings of 3..6 slots
    int split_k = 1;                           // f16x3: cnv5 / cnv6 launches of at most half a workgroup per CU split their K loop in two (plan.hip)
    int fold_fixup = 0;                        // f16x3 split-K: the part that finishes a tile last adds its partial sums (no splitk_fixup launch); needs xcd_rr > 0.  Measured slower (batch 1: 0.141 against 0.132 ms): off
    int f32_n16 = 1;                           // f32 mode: cnv1 (16 output channels) on the 128x16 tile / v_mfma_f32_16x16x4_f32 instead of the padded 128x32 one
    int f32_n256 = 0;                          // f32 mode experiment: cnv5 / cnv6 on the 128 x 256 tile (eight waves, one workgroup per CU)
    int fold_tails = -1;                       // the excitation MLP and the pose head's tile sum run in the last workgroup of the squeeze / cnv7 launch: 0 off | 1 both tails | 2 the excitation only | -1 auto: the excitation at small batches (pose_tail.h: what it costs)
    int fuse_pack = -1;                        // f16x3: mask+pack fused into cnv1's patch fill: 0 off | 1 on | -1 where it pays (small batches: one launch fewer)
    int fuse_pose = 1;                         // f16x3: pose head fused into cnv7's epilogue
    int patch_cnv1_t = 1;                      // three-frame PoseNN, f16x3: cnv1 from an LDS-staged 16-channel patch (conv_patch_cnv1t_h3) instead of the implicit GEMM at cin = 16
    int patch_cnv2 = 1;                        // f16x3: cnv2 from an LDS-staged input patch (conv_patch_cnv2_h3) instead of the implicit GEMM
    int patch_cnv3 = 1;                        // f16x3: cnv3 likewise (conv_patch_cnv3_h3)
    int patch_f32 = 1;                         // float32 mode: cnv1 / cnv2 / cnv3 from an LDS-staged input patch (conv_patch_f32.h) instead of the implicit GEMM
};

// How davo_set_option stores a caller's v.  SWITCH: v != 0.  RANGE: lo below lo, `over' above hi, else v (a clamp where over = hi).
// PAD_MASK: 0 -> 0, 1 -> PAD_CLASS_LAYERS, 8 + mask (8..15) -> the mask; every other value is refused.
enum { RULE_SWITCH = 0, RULE_RANGE = 1, RULE_PAD_MASK = 2 };
struct OptionRow {
    const char* name;
    int LaunchOptions::*field;
    int rule, lo, hi, over;
};
// The rows' order is public: rows 0..13 are davo_decide_layer's options 0..13, rows 14..20 davo_decide_forward's options 0..6
// (hooks.hip holds the table's length to the header's DAVO_DECIDE_OPTIONS and DAVO_FORWARD_OPTIONS).
constexpr OptionRow OPTION_TABLE[] = {
    {"wave128", &LaunchOptions::wave128, RULE_RANGE, 0, 3, 3},
    {"skip_order", &LaunchOptions::skip_order, RULE_RANGE, 0, 2, 2},
    {"merge_order", &LaunchOptions::merge_order, RULE_RANGE, -1, 2, 0},
    {"pad_classes", &LaunchOptions::pad_classes, RULE_PAD_MASK, 0, 0, 0},
    {"merge_rem_f32", &LaunchOptions::merge_rem_f32, RULE_RANGE, 0, 2, 2},
    {"share_taps", &LaunchOptions::share_taps, RULE_SWITCH, 0, 0, 0},
    {"merge_rem", &LaunchOptions::merge_rem, RULE_SWITCH, 0, 0, 0},
    {"merge_cnv4", &LaunchOptions::merge_cnv4, RULE_SWITCH, 0, 0, 0},
    {"tile_208x128", &LaunchOptions::tile_208x128, RULE_SWITCH, 0, 0, 0},
    {"deep_ring", &LaunchOptions::deep_ring, RULE_SWITCH, 0, 0, 0},
    {"split_k", &LaunchOptions::split_k, RULE_SWITCH, 0, 0, 0},
    {"fold_fixup", &LaunchOptions::fold_fixup, RULE_SWITCH, 0, 0, 0},
    {"f32_n16", &LaunchOptions::f32_n16, RULE_SWITCH, 0, 0, 0},
    {"f32_n256", &LaunchOptions::f32_n256, RULE_SWITCH, 0, 0, 0},
    {"fold_tails", &LaunchOptions::fold_tails, RULE_RANGE, -1, 2, 1},
    {"fuse_pack", &LaunchOptions::fuse_pack, RULE_RANGE, -1, 1, 1},
    {"fuse_pose", &LaunchOptions::fuse_pose, RULE_SWITCH, 0, 0, 0},
    {"patch_cnv1_t", &LaunchOptions::patch_cnv1_t, RULE_SWITCH, 0, 0, 0},
    {"patch_cnv2", &LaunchOptions::patch_cnv2, RULE_SWITCH, 0, 0, 0},
    {"patch_cnv3", &LaunchOptions::patch_cnv3, RULE_SWITCH, 0, 0, 0},
    {"patch_f32", &LaunchOptions::patch_f32, RULE_SWITCH, 0, 0, 0},
};
constexpr int NUM_OPTIONS = sizeof OPTION_TABLE / sizeof OPTION_TABLE[0];

inline const OptionRow* find_option(const char* key) {
    for (const OptionRow& r : OPTION_TABLE)
        if (strcmp(r.name, key) == 0) return &r;
    return nullptr;
}
// v as row r stores it -> *stored; false where the row's rule refuses v
inline bool option_store(const OptionRow& r, int v, int* stored) {
    if (r.rule == RULE_PAD_MASK) {
        if (v != 0 && v != 1 && (v < 8 || v > 15)) return false;
        *stored = v == 1 ? PAD_CLASS_LAYERS : v & 7;
    } else {
        *stored = r.rule == RULE_SWITCH ? v != 0 : v < r.lo ? r.lo : v > r.hi ? r.over : v;
    }
    return true;
}

}  // namespace davo

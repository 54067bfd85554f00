// plan.hip — launch planning (see plan.h).  Host logic only.
#include "plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/davo_hip.h"
#include "launch.h"

namespace davo {

#ifdef DAVO_TUNING
const char* tuning_env(const char* name) { return getenv(name); }
#endif

// ---- FP32-MFMA path -------------------------------------------------------------------------------
// Workgroups of one launch all take the same time, and the dispatcher refills both slots of a
// CU together, so a grid that is not a whole number of rounds (256 CUs x resident workgroups)
// pays for a full last round: at B = 32 the 3,328 tiles of cnv5/cnv6 are 6.5 rounds of 512 and
// ran in the time of 7.  A layer is therefore issued as a main launch of whole rounds at the
// widest N tile plus, when it pays, a remainder launch with a narrower N tile (more, shorter
// workgroups) that again fills whole rounds.  Costs are in units of one round of 128x128 tiles.
static int slots_for(int BN, int ncu) { return ncu * (BN == 32 ? 3 : 2); }         // LDS 46 / 55 / 74 KB per workgroup
// time of one round (every CU full) relative to a round of 128x128 tiles: resident workgroups
// per CU x tile area / measured relative efficiency of the narrower tiles
static double tile_cost(int BN) { return BN == 128 ? 1.0 : BN == 64 ? 0.5 / 0.92 : 0.375 / 0.75; }

static double rounds_cost(long tiles, int BN, int ncu) {
    const long s = slots_for(BN, ncu);
    return (double)((tiles + s - 1) / s) * tile_cost(BN);
}

std::vector<Launch> plan_layer(int mtiles, int npad, int groups, int ncu) {
    int bmax = npad % 128 == 0 ? 128 : npad % 64 == 0 ? 64 : 32;
    // tuning build only: DAVO_FORCE_BN=32|64|128 -> one launch at that N tile, DAVO_PLAN=single -> one launch
    // at the widest N tile
    if (const char* e = tuning_env("DAVO_FORCE_BN")) {
        const int bn = atoi(e);
        if ((bn == 32 || bn == 64 || bn == 128) && npad % bn == 0) return {{0, mtiles, bn}};
    }
    if (const char* e = tuning_env("DAVO_PLAN"))
        if (!strcmp(e, "single")) return {{0, mtiles, bmax}};
    std::vector<Launch> best;
    double best_cost = 1e30;
    for (int bn = bmax; bn >= 32; bn >>= 1) {                          // one launch
        const double c = rounds_cost((long)mtiles * (npad / bn) * groups, bn, ncu);
        if (c < best_cost - 1e-9) { best_cost = c; best = {{0, mtiles, bn}}; }
    }
    const long per_m = (long)(npad / bmax) * groups;                   // tiles per M tile at bmax
    const long s = slots_for(bmax, ncu);
    const int main_m = (int)(((long)mtiles * per_m / s) * s / per_m);  // whole rounds only
    if (main_m > 0 && main_m < mtiles && (main_m * per_m) % s == 0) {
        const double cm = rounds_cost(main_m * per_m, bmax, ncu);
        for (int bn = bmax; bn >= 32; bn >>= 1) {
            const double c = cm + rounds_cost((long)(mtiles - main_m) * (npad / bn) * groups, bn, ncu) + 0.02;
            if (c < best_cost - 1e-9) { best_cost = c; best = {{0, main_m, bmax}, {main_m, mtiles - main_m, bn}}; }
        }
    }
    return best;
}

// ---- f16x3 path -----------------------------------------------------------------------------------
TileShape tile_shape(int t) {
    switch (t) {
        case TILE_128x32: return {128, 32, 256, TileH<4, 1, 1, 1>::LDS_BYTES_DMA};
        case TILE_256x64: return {256, 64, 512, TileH<4, 2, 2, 1>::LDS_BYTES_DMA};
        case TILE_256x128: return {256, 128, 512, TileH<4, 2, 2, 2>::LDS_BYTES_DMA};
        case TILE_128x256: return {128, 256, 512, TileH<2, 4, 2, 2>::LDS_BYTES_DMA};
        case TILE_256x256: return {256, 256, 512, TileH<4, 2, 2, 4>::LDS_BYTES_DMA};
        case TILE_208x256: return {TileS::BM, TileS::BN, TileS::THREADS, TileS::LDS_BYTES};
        case TILE_208x128: return {TileSW<4>::BM, TileSW<4>::BN, TileSW<4>::THREADS, TileSW<4>::lds_bytes(3)};
        default: return {128, 128, 512, TileH<4, 2, 1, 2>::LDS_BYTES_DMA};
    }
}

// Same idea as plan_layer: whole rounds of the most efficient tile, then a remainder launch with a
// smaller tile that again fills whole rounds.  Costs are in units of one round of 256x256 tiles;
// eff = measured throughput of the tile relative to 256x256 at full occupancy (B=128: cnv5, cnv6, cnv7 forced to
// one tile shape each, re-measured after the matrix loop was software-pipelined).  The two narrow tiles keep the
// figures fitted on the K < 600 layers that use them (cnv3, cnv4: A/B on one box, profiles/ r01f notes).
// The 208x256 tile (conv_igemm_h3s.h) is offered only to the layers it is instantiated for and only as a single launch;
// 0.93: cnv6 at B=128 (16 whole rounds) 1.995 ms against 1.869 ms on 13 rounds of 256x256, cnv5 1.071 against 0.997 (three pixel
// ring slots on the 208 tile, shared-tap staging on the 256 tile).
// Round 2: 256x256 and 256x128 stage one pixel patch per filter row for its three taps on cnv3..cnv6 (-3 % and -6 %:
// gpurun_out/ab_r02v.log, ab_r02w.log), which moves 256x128 past 128x128 where no round is left half empty (cnv4 at B=128).
static TileInfo kTiles[] = {{TILE_256x256, 1, 1.00}, {TILE_128x256, 1, 0.82}, {TILE_256x128, 1, 0.89},
                            {TILE_128x128, 2, 0.87}, {TILE_256x64, 2, 0.62}, {TILE_128x32, 4, 0.40}, {TILE_208x256, 1, 0.93},
                            {TILE_208x128, 1, 0.75}};      // 208x128: cnv4 only, offered with "tile_208x128" 1; fitted on cnv4 at B = 32 (profiles/r04_cnv4_208x128_ab.log)

// tuning build only: DAVO_H3_EFF="e0,e1,e2,e3,e4,e5[,p4]" (and DAVO_H3_EFF208=e) overrides the efficiencies (table order) and 256x64's per_cu
static void tiles_from_env() {
    static bool done = false;
    if (done) return;
    done = true;
    const char* e = tuning_env("DAVO_H3_EFF");
    if (!e) return;
    double v[7] = {0, 0, 0, 0, 0, 0, 0};
    const int n = sscanf(e, "%lf,%lf,%lf,%lf,%lf,%lf,%lf", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6);
    for (int i = 0; i < 6 && i < n; ++i) if (v[i] > 0) kTiles[i].eff = v[i];
    if (n >= 7 && v[6] >= 1) kTiles[4].per_cu = (int)v[6];
    if (const char* e2 = tuning_env("DAVO_H3_EFF208")) { const double x = atof(e2); if (x > 0) kTiles[6].eff = x; }
}

const TileInfo* h3_tiles(int* n) {
    tiles_from_env();
    if (n) *n = (int)(sizeof kTiles / sizeof kTiles[0]);
    return kTiles;
}

// whole rounds run per_cu workgroups per CU side by side; in the last, partial round a CU holds
// ceil(rest / 256) of them (the dispatcher spreads a short tail one per CU)
double h3_cost(const TileInfo& t, long ntiles, int ncu) {
    const TileShape ts = tile_shape(t.id);
    const long slots = (long)ncu * t.per_cu;
    const double one = (ts.bm * ts.bn / 65536.0) / t.eff;
    const long full = ntiles / slots, rest = ntiles % slots;
    return (double)full * t.per_cu * one + (double)((rest + ncu - 1) / ncu) * one;
}

std::vector<LaunchH> plan_layer_h3(int M, int npad, int groups, int forced_tile, bool allow_208, int ncu, double others_scale) {
    tiles_from_env();
    TileInfo tiles[sizeof kTiles / sizeof kTiles[0]];
    for (size_t i = 0; i < sizeof kTiles / sizeof kTiles[0]; ++i) {
        tiles[i] = kTiles[i];
        if (tiles[i].id != TILE_256x256) tiles[i].eff *= others_scale;
    }
    auto ntiles = [&](const TileInfo& t, int rows) {
        const TileShape ts = tile_shape(t.id);
        return (long)((rows + ts.bm - 1) / ts.bm) * (npad / ts.bn) * groups;
    };
    auto fits = [&](const TileInfo& t) {
        const int bn = tile_shape(t.id).bn;
        return bn <= npad && npad % bn == 0 && (!is_208(t.id) || (allow_208 && bn == npad));
    };
    if (forced_tile >= 0 && forced_tile != TILE_MERGED_MARK && (!is_208(forced_tile) || (allow_208 && tile_shape(forced_tile).bn == npad))) return {{0, M, forced_tile}};
    std::vector<LaunchH> best;
    double best_cost = 1e30;
    const char* rf = tuning_env("DAVO_H3_REM_TILE");
    const int rem_force = rf ? atoi(rf) : -1;
    for (const TileInfo& t1 : tiles) {
        if (!fits(t1)) continue;
        const double c1 = h3_cost(t1, ntiles(t1, M), ncu);
        if (c1 < best_cost - 1e-9) { best_cost = c1; best = {{0, M, t1.id}}; }
        if (is_208(t1.id)) continue;                                       // single launch only
        const TileShape s1 = tile_shape(t1.id);
        const long per_round = (long)ncu * t1.per_cu, per_m = (long)(npad / s1.bn) * groups;
        if (per_round % per_m) continue;
        const long m_per_round = per_round / per_m;                       // M tiles of t1 in one round
        const long rounds = ((long)M / s1.bm) / m_per_round;
        int rows1 = (int)(rounds * m_per_round * s1.bm);
        rows1 -= rows1 % 256;                                             // every tile height divides 256
        if (rows1 <= 0 || rows1 >= M) continue;
        const double cm = h3_cost(t1, ntiles(t1, rows1), ncu);
        for (const TileInfo& t2 : tiles) {
            if (!fits(t2) || is_208(t2.id)) continue;
            if (rem_force >= 0 && t2.id != rem_force) continue;
            const double c = cm + h3_cost(t2, ntiles(t2, M - rows1), ncu) + 0.08;      // a second launch: its fill/drain and the kernel boundary
            if (c < best_cost - 1e-9) { best_cost = c; best = {{0, rows1, t1.id}, {rows1, M - rows1, t2.id}}; }
        }
    }
    return best;
}

int plan_single_tile_h3(int M, int npad, int groups, int max_bm, int forced_tile, bool allow_208, int ncu) {
    tiles_from_env();
    for (int pass = 0; pass < 2; ++pass) {                               // a forced tile that does not fit is ignored
        int best = -1;
        double bc = 1e30;
        for (const TileInfo& t : kTiles) {
            const TileShape ts = tile_shape(t.id);
            if (ts.bn > npad || npad % ts.bn || ts.bm > max_bm || (is_208(t.id) && !(allow_208 && ts.bn == npad))) continue;
            if (pass == 0 && forced_tile >= 0 && t.id != forced_tile) continue;
            const double cst = h3_cost(t, (long)((M + ts.bm - 1) / ts.bm) * (npad / ts.bn) * groups, ncu);
            if (cst < bc) { bc = cst; best = t.id; }
        }
        if (best >= 0 || forced_tile < 0) return best;
    }
    return -1;
}

// ---- a layer's launches (plan.h: LayerDecision) ----------------------------------------------------------------------------------
const char* family_name(int family) {
    static const char* const names[NUM_FAMILIES] = {"h3", "h3s", "h3w", "h3w64", "h3w128", "h3_mainrem", "h3 split-K", "f32", "f32 n256", "f32 mainrem"};
    return family >= 0 && family < NUM_FAMILIES ? names[family] : "?";
}

ConvParamsH fill_params_h3(const LayerGeom& L, const LayerCall& call, bool share_taps, int shift_in, int shift_out) {
    ConvParamsH p{};
    same_pad(call.Hin, L.KS, L.stride, L.rate, &p.Hout, &p.pad_t);
    same_pad(call.Win, L.KS, L.stride, L.rate, &p.Wout, &p.pad_l);
    p.Hin = call.Hin; p.Win = call.Win;
    p.x_pix_bytes = (long)call.x_ch * 4; p.x_boff = 0; p.x_pix_log2 = ilog2_exact(call.x_ch * 4);
    p.cb_log2 = L.cb_log2; p.tpc_log2 = L.tpc_log2; p.cpb = L.cpb; p.nchunks = L.nchunks_h;
    p.w_row_bytes = (long)L.nchunks_h * 128;
    p.y_mode = call.y_f32 ? 0 : 1; p.y_ld = call.y_ld; p.y_coff = 0; p.Cout = L.cout;
    p.rate = L.rate;
    p.M = call.NB * p.Hout * p.Wout; p.ntaps = L.KS * L.KS; p.mtile0 = 0; p.relu = 1;
    p.Mtot = p.M; p.xs = share_taps ? 1 : 0;
    // stored activations carry 2^act_shift (exact)
    p.out_scale = ldexpf(1.0f / L.wscale, shift_out - shift_in);
    p.bias_scale = ldexpf(L.wscale, shift_in);
    if (L.groups == 2) {
        p.g_x_boff = L.cin * 4; p.g_y_coff = L.cout;
        p.g_w = (long)L.npad_h * p.w_row_bytes; p.g_bias = L.npad_h;
    }
    return p;
}

ConvParams fill_params_f32(const LayerGeom& L, const LayerCall& call) {
    ConvParams p{};
    same_pad(call.Hin, L.KS, L.stride, L.rate, &p.Hout, &p.pad_t);
    same_pad(call.Win, L.KS, L.stride, L.rate, &p.Wout, &p.pad_l);
    p.Hin = call.Hin; p.Win = call.Win;
    p.cin_log2 = L.cin_log2; p.x_ld = call.x_ch; p.x_coff = 0; p.y_ld = call.y_ld; p.y_coff = 0;
    p.Cout = L.cout; p.rate = L.rate;
    p.M = call.NB * p.Hout * p.Wout; p.nchunks = L.nchunks; p.Kpad = L.kpad; p.ntaps = L.KS * L.KS;
    p.ntiles_n = L.npad / L.BN; p.relu = 1;
    if (L.groups == 2) {
        p.g_x_coff = L.cin; p.g_y_coff = L.cout;
        p.g_w = (long)L.npad * L.kpad; p.g_bias = L.npad;
    }
    return p;
}

// The float32 rules, in order: the planner's launches (cnv1 on the 128x16 tile), then "f32_n256", then the merged
// main + remainder grid, else one launch per planned launch.
LayerDecision<ConvParams> decide_layer_f32(const LayerGeom& L, const LayerCall& call, const PlanOptions& o) {
    LayerDecision<ConvParams> d;
    const int li = call.li;
    ConvParams p = fill_params_f32(L, call);
    const int mtiles = (p.M + BM - 1) / BM;
    std::vector<Launch> plan = plan_layer(mtiles, L.npad, L.groups, o.ncu);
    if (li == 0 && L.cout <= 16 && o.f32_n16) plan = {{0, mtiles, 16}};      // cnv1 on the 128x16 tile at every batch size (conv_igemm.h, N16)
    if (call.fuse_pose) {      // the pose head runs in the epilogue (conv_igemm.h)
        d.pose_floats = (size_t)L.groups * mtiles * 8 * 6;
        p.pose_P = p.Hout * p.Wout; p.pose_mt = mtiles;
        d.pose_bm = BM; d.pose_mt = mtiles; d.pose_ntn = 8;
    }
    // cnv4, cnv5, cnv6: GEMM rows sorted by padding class, every tile walks the taps of its own pixels ("pad_classes")
    d.pad_classes = li >= 3 && li <= 5 && ((o.pad_classes >> (li - 3)) & 1) && L.KS == 3 && L.stride == 1 && L.cin_log2 >= 5 && L.groups == 1 &&
                    !call.fuse_pose && !o.f32_n256;
    const bool long_first = L.KS == 3 && L.cin_log2 >= 5;       // the tiles of a 3x3 layer skip different numbers of padding rows
    auto block = [&](LaunchStep<ConvParams>& s, int b, int key, int mtile0, int n_mtiles, int ntn) {
        s.p[b] = p;
        s.p[b].mtile0 = mtile0; s.p[b].ntiles_n = ntn;
        s.ord[b] = {long_first ? ORDER_LONG_FIRST : ORDER_NONE, key, BM, mtile0, n_mtiles, ntn};
        s.nblocks = b + 1;
        s.m_end = std::min((mtile0 + n_mtiles) * BM, p.M);
    };
    // experiment ("f32_n256"): cnv5 / cnv6 as whole rounds of 128 x 256 tiles (eight waves, one workgroup per CU) + a remainder launch of
    // 128 x 64 tiles
    if (o.f32_n256 && (li == 4 || li == 5) && L.npad == 256 && L.groups == 1 && !call.fuse_pose && mtiles >= o.ncu) {
        const int main_m = (mtiles / o.ncu) * o.ncu;
        LaunchStep<ConvParams>& sm = d.steps[d.nsteps++];
        sm.family = FAM_F32_N256; sm.tile = 256; sm.gx = main_m;
        block(sm, 0, 2, 0, main_m, 1);
        d.plan_code[0] = main_m * 1000 + 256;
        if (main_m < mtiles) {
            LaunchStep<ConvParams>& sr = d.steps[d.nsteps++];
            sr.family = FAM_F32; sr.tile = 64; sr.row0 = main_m * BM; sr.rem_label = true;
            block(sr, 0, 0, main_m, mtiles - main_m, L.npad / 64);
            sr.gx = (mtiles - main_m) * sr.p[0].ntiles_n;
            d.plan_code[1] = (mtiles - main_m) * 1000 + 64;
        }
        return d;
    }
    // main + remainder as one grid (conv_igemm.h, conv_igemm_f32_mainrem; "merge_rem_f32"): the remainder's tiles start on the CUs
    // that finish their last main tile first, instead of behind a launch boundary.  Same tiles, same arithmetic.
    // (cnv7 keeps its two launches: merged it measured 0.532 against 0.439 + 0.052 ms - its 32-column remainder tiles then run two per CU
    // on the main tile's LDS and register budget instead of three, and 0.545 with a 64-column remainder; cnv4 / cnv5 / cnv6: -5 / -4 / -1 %,
    // profiles/r05q_f32_mainrem_ab.md)
    if (o.merge_rem_f32 && li >= 3 && (li <= 5 || o.merge_rem_f32 > 1) && plan.size() == 2 && plan[0].BN == 128 && (plan[1].BN == 32 || plan[1].BN == 64)) {
        const int ntn_m = L.npad / 128, ntn_r = L.npad / plan[1].BN;
        const int n_main = plan[0].mtiles * ntn_m, n_rem = plan[1].mtiles * ntn_r;
        if (n_main % 8 == 0 && (L.groups == 1 || n_rem % 8 == 0)) {
            LaunchStep<ConvParams>& s = d.steps[d.nsteps++];
            s.family = FAM_F32_MAINREM; s.tile = plan[1].BN; s.n_main = n_main; s.n_rem = n_rem;
            s.gx = (n_main + n_rem) * L.groups;
            block(s, 0, 0, plan[0].mtile0, plan[0].mtiles, ntn_m);
            block(s, 1, 0, plan[1].mtile0, plan[1].mtiles, ntn_r);
            d.plan_code[0] = (plan[0].mtiles + plan[1].mtiles) * 1000 + 128;      // one launch covers the layer
            return d;
        }
    }
    for (size_t i = 0; i < plan.size() && i < 2; ++i) {
        LaunchStep<ConvParams>& s = d.steps[d.nsteps++];
        s.family = FAM_F32; s.tile = plan[i].BN; s.row0 = plan[i].mtile0 * BM; s.rem_label = i > 0;
        block(s, 0, 0, plan[i].mtile0, plan[i].mtiles, plan[i].BN == 16 ? 1 : L.npad / plan[i].BN);
        s.gx = plan[i].mtiles * s.p[0].ntiles_n; s.gy = L.groups;
        d.plan_code[i] = plan[i].mtiles * 1000 + plan[i].BN;
    }
    return d;
}

// The f16x3 rules, in order: the planner's launches; the fused pose head's single tile; cnv4 on conv_igemm_h3w128;
// "merge_cnv4"; the merged main + remainder grid; split-K; else one launch per planned launch, on conv_igemm_h3w / h3w64 where "wave128"
// has a kernel for it.
LayerDecision<ConvParamsH> decide_layer_h3(const LayerGeom& L, const LayerCall& call, const PlanOptions& o) {
    LayerDecision<ConvParamsH> d;
    const int li = call.li;
    const bool fuse_pose = call.fuse_pose;
    // cnv7 feeds the float32 pose head unscaled
    ConvParamsH p = fill_params_h3(L, call, o.share_taps, o.shift_in, li == 6 ? 0 : o.shift_out);
    if (const char* e = tuning_env("DAVO_DBG")) p.dbg = atoi(e);       // tuning build only
    // cnv5, cnv6, cnv7 (256 channels per group) and cnv4 (128): conv_igemm_h3s.h is instantiated for them
    const bool allow_208 = (li >= 4 && L.npad_h == 256) || (li == 3 && L.npad_h == 128 && o.tile_208x128);
    // cnv5 / cnv6 with "wave128": the 256x256 tile is conv_igemm_h3w's, 4.7 % faster than the one the planner's table was fitted on
    // (measured across 21 batch sizes with the table scaled: only B = 24 and 256x832 B = 6 change plan, -2.7 / -3.2 %: profiles/r05bn_planner_scale.log)
    const double others_scale = (o.wave128 && (li == 4 || li == 5) && L.npad_h == 256 && L.groups == 1 && !fuse_pose) ? 0.955 : 1.0;
    std::vector<LaunchH> plan = plan_layer_h3(p.M, L.npad_h, L.groups, L.tile_h, allow_208, o.ncu, others_scale);
    if (fuse_pose) {      // one launch, one tile shape no taller than an image, so a tile touches <= 2 images
        const int P = p.Hout * p.Wout;
        if (call.pose_six && (li != 6 || L.groups != 1)) { d.err = DAVO_ERR_INVALID; d.msg = "internal: the six-column fused pose head belongs to a one-group cnv7"; return d; }
        const int best = plan_single_tile_h3(p.M, L.npad_h, L.groups, P, L.tile_h, allow_208 && !call.pose_six, o.ncu);
        if (best < 0) { d.err = DAVO_ERR_INVALID; d.msg = "no tile fits the fused pose head"; return d; }
        plan = {{0, p.M, best}};
        const TileShape ts = tile_shape(best);
        const int mt = (p.M + ts.bm - 1) / ts.bm, ntn = L.npad_h / ts.bn;
#ifdef DAVO_POSE_DEBUG
        d.pose_debug_bytes = (size_t)L.groups * mt * ntn * 512 * 20 * sizeof(float);
#endif
        d.pose_floats = (size_t)(call.pose_six ? 2 : L.groups) * mt * ntn * 6;      // six columns: [2 column halves][mt][ntn][2][3]
        p.y_mode = 2; p.pose_P = P; p.pose_mt = mt; p.pose_nc = call.pose_six ? 6 : 0;
        if (call.pose_tail) {      // the launch's last workgroup adds the tiles and writes the poses (pose_tail.h)
            p.pose_NB = call.NB; p.pose_bm = ts.bm; p.pose_total = L.groups * mt * ntn;
        }
        d.pose_bm = ts.bm; d.pose_mt = mt; d.pose_ntn = ntn;
    }
    // cnv4 on conv_igemm_h3w128's 256 x 128 tiles, every row in one launch - where the 256-row tiles fill whole rounds of the CUs or
    // nearly so: a round of them takes 24.4 us against 29.2 for the same rows on conv_igemm_h3's tiles (B = 128: 0.385 -> 0.318 ms),
    // which a last round that is three quarters empty gives back (B = 32, 3.25 rounds: 0.0925 -> 0.0938 ms)
    const long t256 = (p.M + 255) / 256;
    const bool rounds_ok = t256 >= o.ncu && (double)((t256 + o.ncu - 1) / o.ncu) * o.ncu <= 1.12 * (double)t256;
    if ((o.wave128 >= 3 || (o.wave128 >= 2 && rounds_ok)) && li == 3 && !fuse_pose && L.groups == 1 && L.npad_h == 128 && L.tile_h < 0 &&
        p.M >= 256 * o.ncu) {
        ConvParamsH pw = p;
        pw.ntiles_n = 1; pw.mtile0 = 0;
        if (layer_h3w128_supported(pw)) {
            LaunchStep<ConvParamsH>& s = d.steps[d.nsteps++];
            s.family = FAM_H3W128; s.tile = TILE_256x128; s.p[0] = pw; s.gx = (unsigned)(pw.M / 256);
            d.plan_code[0] = ((p.M + 127) / 128) * 1000 + TILE_256x128;
            return d;
        }
    }
    if (o.merge_cnv4 && o.merge_rem && li == 3 && !fuse_pose && L.npad_h == 128 && L.groups == 1 && o.ncu == 256 && L.tile_h < 0 &&
        plan.size() == 1 && plan[0].tile == TILE_128x128) {
        // cnv4 (N = 128): whole rounds of 256x128 tiles (shared-tap staging, twice the matrix work per staged byte of the
        // 128x128 tile) + the remaining rows on 128x128 tiles, as one grid like cnv5 / cnv6 below
        const int rows1 = (p.M / 256 / o.ncu) * o.ncu * 256;
        const int rem = p.M - rows1, n_rem = (rem + 127) / 128;
        if (rows1 > 0 && rem > 0 && rem % 128 == 0 && n_rem % 64 == 0 && n_rem <= 256)
            plan = {{0, rows1, TILE_256x128}, {rows1, rem, TILE_128x128}};
    }
    const bool merge_256 = plan.size() == 2 && plan[0].tile == TILE_256x256 && plan[1].tile == TILE_128x128 && L.npad_h == 256;
    // the merged grid's 256x128 main tile is instantiated for cnv4 alone (launch_h3.hip): a cnv6 of 128 columns (-cnv6_64) with the same
    // plan keeps its two launches
    const bool merge_128 = li == 3 && plan.size() == 2 && plan[0].tile == TILE_256x128 && plan[1].tile == TILE_128x128 && L.npad_h == 128;
    if (o.merge_rem && !fuse_pose && (merge_256 || merge_128) && L.groups == 1 && o.ncu == 256 && !tuning_env("DAVO_NO_MERGE")) {
        // main + remainder as one grid (conv_igemm_h3_mainrem): same tiles, same arithmetic, de-phased store bursts
        ConvParamsH pm = p, pr = p;
        const int rem_ntn = L.npad_h / 128;                       // N tiles of a 128x128 remainder row block
        pm.ntiles_n = 1; pm.mtile0 = 0; pm.M = plan[0].rows;
        pr.ntiles_n = rem_ntn; pr.mtile0 = plan[1].row0 / 128; pr.M = plan[1].row0 + plan[1].rows;
        const int n_main = plan[0].rows / 256, n_rem = ((plan[1].rows + 127) / 128) * rem_ntn;
        // "wave128": the four-wave main tile (conv_igemm_h3w.h) runs as a launch of its own - merged with four-wave remainder tiles it
        // measured 0.262 / 0.497 ms for cnv5 / cnv6 against 0.258 / 0.487 as two launches (profiles/r05bc_w128_ab.log)
        const bool own_launch = o.wave128 && merge_256 && layer_h3w_supported(li, pm);
        if (!own_launch && layer_h3_mainrem_supported(li, pm, n_main, n_rem)) {
            LaunchStep<ConvParamsH>& s = d.steps[d.nsteps++];
            s.family = FAM_H3_MAINREM; s.tile = plan[0].tile; s.nblocks = 2; s.p[0] = pm; s.p[1] = pr;
            s.n_main = n_main; s.n_rem = n_rem; s.gx = n_main + n_rem;
            // f16x3: long-first measured 256.8 against 259.9 us on cnv5 with a third more HBM reads (205 -> 272 MB: neighbours no longer
            // run side by side) and no change of the power-capped step: natural order unless "skip_order" is 2
            if (o.skip_order >= 2) s.ord[0] = {ORDER_LONG_FIRST, 1, 256, 0, n_main, 1};
            s.order = o.merge_order;
            d.plan_code[0] = ((plan[0].rows + plan[1].rows + 127) / 128) * 1000 + TILE_MERGED_MARK;     // 256x256 + 128x128 in one grid
            return d;
        }
    }
    // Split-K.  A launch of at most half a workgroup per CU (cnv6 at batch 1: 104 tiles of 128x128, each a serial chain of 72
    // chunks at ~0.7 us) leaves half of the chip idle and is as long as its chain: the two halves of the input channels run
    // as two "groups" of the same kernel (the grouped-convolution path cnv7 uses: own channel offset, weight offset and
    // output slot; the second half starts from a zero bias) into float32 partial sums, and splitk_fixup adds the two,
    // applies ReLU and writes the stored form.  Two partial sums instead of one chain change the float32 rounding of the
    // layer's outputs (not their value: ~1e-7 relative), so batch sizes that split and batch sizes that do not agree to
    // rounding, not to the bit ("split_k" 0 restores the single chain).  (With S parts: S groups, S partial sums.)
    if (o.split_k && !fuse_pose && (li == 4 || li == 5) && L.groups == 1 && plan.size() == 1 && p.y_mode == 1 && L.cout % 32 == 0 &&
        !is_208(plan[0].tile)) {
        const TileShape ts = tile_shape(plan[0].tile);
        const int mtiles = (p.M + ts.bm - 1) / ts.bm, ntn = L.npad_h / ts.bn;
        const long tiles = (long)mtiles * ntn;
        // parts: whole channel blocks each, whole filter rows (shared-tap staging walks a row's three taps together).  Four parts
        // where the workgroups then still fit side by side (two per CU on the two-slot ring), else two (one per CU, deep ring)
        auto fits = [&](int S) { return L.nchunks_h % (S * L.cpb) == 0 && ((L.nchunks_h / S) % 3) == 0; };
        const int per_cu = ts.lds * 2 <= 160 * 1024 ? 2 : 1;
        const int S = (fits(4) && tiles * 4 <= (long)per_cu * o.ncu && tiles * 2 <= o.ncu) ? 4 : (fits(2) && tiles * 2 <= o.ncu ? 2 : 1);       // two parts at two per CU (B = 2) measured slower: 54 -> 57 us
        if (S > 1) {
            LaunchStep<ConvParamsH>& s = d.steps[d.nsteps++];
            ConvParamsH& ps = s.p[0];
            ps = p;
            ps.nchunks = L.nchunks_h / S;
            ps.g_x_boff = (L.cin / S) * 4; ps.g_w = (long)ps.nchunks * 128; ps.g_bias = L.npad_h; ps.g_y_coff = L.cout;
            ps.y_mode = 0; ps.y_ld = S * L.cout; ps.relu = 0;
            ps.ntiles_n = ntn; ps.mtile0 = 0;
            s.family = FAM_H3_SPLITK; s.tile = plan[0].tile; s.gx = mtiles * ntn; s.gy = S;
            ps.deep = o.deep_ring && tiles * S <= o.ncu;
            d.plan_code[0] = ((p.M + 127) / 128) * 1000 + plan[0].tile; d.split = S;
            d.splitk_floats = (size_t)p.M * S * L.cout; d.sk_M = p.M; d.sk_cout = L.cout;
            // The fix-up folded into the launch (pose_tail.h, splitk_tail): with an x extent that is a multiple of 8 the S parts of a
            // tile run on one XCD, so the part that finishes last finds the others' partial sums in its own L2 and writes the stored
            // form itself - no splitk_fixup launch (7 us each at batch 1, two per forward).  Checked once per context on the device.
            d.fold_if_xcd = o.fold_fixup && S <= 4 && s.gx % 8 == 0 && (int)s.gx <= SK_TILE_COUNTERS && o.ncu == o.dev_cus && !o.cu_partition &&
                            !o.user_stream;
            d.sk_counter0 = 1 + o.max_batch;
            return d;
        }
    }
    for (size_t i = 0; i < plan.size() && i < 2; ++i) {
        const TileShape ts = tile_shape(plan[i].tile);
        LaunchStep<ConvParamsH>& s = d.steps[d.nsteps++];
        ConvParamsH& q = s.p[0];
        q = p;
        q.ntiles_n = L.npad_h / ts.bn;
        q.mtile0 = plan[i].row0 / ts.bm;
        q.M = plan[i].row0 + plan[i].rows;                    // rows past this launch's range are not its job
        const int mtiles = (plan[i].rows + ts.bm - 1) / ts.bm;
        s.gx = mtiles * q.ntiles_n; s.gy = L.groups;
        q.deep = o.deep_ring && plan.size() == 1 && (long)s.gx * s.gy <= o.ncu;       // at most one workgroup per CU
        d.plan_code[i] = ((plan[i].rows + 127) / 128) * 1000 + plan[i].tile;
        // no tile order here: cnv4's single launch of 128x128 tiles (two per CU, 6.5 rounds) measured 94.4 us in natural order and
        // 97.4 long-first (profiles/r04e_skip_padding_rows.md); the merged grids above and the float32 launches take one
        s.family = is_208(plan[i].tile) ? FAM_H3S : FAM_H3; s.tile = plan[i].tile; s.row0 = plan[i].row0; s.rem_label = i > 0;
        if (o.wave128 && L.groups == 1 && !fuse_pose) {
            if (plan[i].tile == TILE_256x256 && layer_h3w_supported(li, q)) s.family = FAM_H3W;
            else if (o.wave128 >= 2 && i == 1 && plan.size() == 2 && plan[0].tile == TILE_256x256 && plan[1].tile == TILE_128x128 &&
                     L.npad_h == 256 && plan[1].row0 % 256 == 0 && plan[1].rows % 256 == 0) {
                // the remainder rows of a layer whose main launch ran on conv_igemm_h3w: 256 x 64 tiles (conv_igemm_h3w64)
                ConvParamsH pr = q;
                pr.ntiles_n = 4; pr.mtile0 = plan[1].row0 / 256;
                if (layer_h3w64_supported(li, pr)) {
                    q = pr;
                    s.family = FAM_H3W64; s.gx = (unsigned)(plan[1].rows / 256 * 4); s.gy = 1;
                }
            }
        }
    }
    return d;
}

// ---- the whole forward ------------------------------------------------------------------------------------------------------------
namespace {
constexpr int FOLD_EXCITE_MAX_BATCH = 2;       // auto modes: largest batch that folds the excitation / fuses mask + pack into cnv1
constexpr int FUSE_PACK_MAX_BATCH = 0;         // measured level at every batch (cnv1 +5 us for mask_pack's 6.7): nowhere by default
constexpr const char* const FORWARD_LABELS[] = DAVO_FORWARD_LABELS;
static_assert(sizeof FORWARD_LABELS / sizeof *FORWARD_LABELS == NUM_LABELS, "plan.h's LB_* index DAVO_FORWARD_LABELS");
constexpr int PATCH_PLAN_ID[3] = {99, 98, 97}, PATCH_CNV1T_PLAN_ID = 96;       // davo_last_plan's tile ids of the patch kernels

ForwardPlan refuse(ForwardPlan p, int err, const char* fmt, int a = 0, int b = 0) {
    p.err = err;
    snprintf(p.msg, sizeof p.msg, fmt, a, b);
    return p;
}
}  // namespace

const char* forward_label(int label) { return label >= 0 && label < NUM_LABELS ? FORWARD_LABELS[label] : "?"; }

// Launches are ~6 us each whatever they do; at batch 1 the path is 11 of them around 0.1 ms of work.  Where a launch can be folded
// into its neighbour at less than that, small batches do it (measured per batch: profiles/): the excitation MLP
// in the squeeze launch's last workgroup (costs two memory-side round trips per workgroup: +2 us at B = 1, +18 us at B = 32), mask +
// pack inside cnv1's patch fill (level at B = 32).
ForwardPlan decide_forward(const ForwardCall& call, const ForwardOptions& o) {
    ForwardPlan p;
    p.mode = call.mode;
    const int sel = call.pairs, B = call.B, a = call.v.att_source, c6 = call.v.cnv6_out;
    const bool tri = call.triplet, cpl = call.coupled, se = call.posenn_se != 0;
    const bool h3 = call.mode == MODE_H3, direct = call.mode == MODE_DIRECT;
    if (sel != PAIRS_SRC0 && sel != PAIRS_SRC1 && sel != PAIRS_BOTH) return refuse(p, DAVO_ERR_INVALID, "internal: pair selection %d", sel);
    if (cpl && (tri || se || call.groups6 != 1 || call.groups7 != 1 || call.cin7 != c6))
        return refuse(p, DAVO_ERR_INVALID, "internal: the coupled PoseNN runs on the pair topology with one-group cnv6 and cnv7");
    if (tri && (sel != PAIRS_BOTH || direct))
        return refuse(p, DAVO_ERR_INVALID, "internal: the three-frame PoseNN runs both pairs on the MFMA kernels (pairs %d, impl %d)", sel, direct ? 1 : 0);
    if (direct && call.v.cin_per_frame != 5) return refuse(p, DAVO_ERR_INVALID, "impl 1 supports the 10-channel (v1) input only");
    p.NB = tri ? B : pairs_per_window(sel) * B;        // the three-frame PoseNN: one image per window, both poses from one pass
    auto launch = [&](int label) { p.launch[p.nlaunch++] = label; };

    // the attention front: squeeze, then (or, folded, in the squeeze launch's last workgroup) the excitation
    const bool split = a == ATT_DEPTH_SPLIT, pooled = att_pooled(a);
    const bool fold = (att_flow_squeeze(a) || att_class_table(a)) && (o.fold_tails >= 1 || (o.fold_tails < 0 && B <= FOLD_EXCITE_MAX_BATCH));
    const bool fold_pose = o.fold_tails == 1;
    p.front.kind = pooled ? FRONT_POOLED : att_desc_depth(a) ? FRONT_DEPTH : att_class_table(a) ? FRONT_CLASS : split ? FRONT_FLOW_SPLIT : FRONT_FLOW;
    p.front.squeeze = p.front.kind != FRONT_FLOW || att_flow_squeeze(a);      // (no attention, static tables: the excitation launch alone)
    p.front.fold_excite = fold;
    p.front.excite = !fold && !pooled;                 // pooled: se_pool_excite, always a launch of its own ("fold_tails" does not apply)
    p.front.excite_far = !fold && split;               // the same launch again on the far MLP, under a profile entry of its own
    const int squeeze_label = pooled ? LB_SE_POOL_SQUEEZE : p.front.kind == FRONT_DEPTH ? LB_SE_DEPTH_SQUEEZE
                              : p.front.kind == FRONT_CLASS ? LB_SE_CLASS_SQUEEZE : LB_SE_SQUEEZE_PARTIAL;
    if (p.front.squeeze) launch(squeeze_label);
    if (pooled) launch(LB_SE_POOL_EXCITE);
    if (p.front.excite) launch(LB_SE_EXCITE);
    if (p.front.excite_far) launch(LB_SE_EXCITE_FAR);
    // the record's per-batch word is zeroed by the launch that evaluates the tables
    if (h3 && o.zero_record) p.front.reset_at = pooled ? LB_SE_POOL_EXCITE : fold ? squeeze_label : LB_SE_EXCITE;

    // f16x3, fuse_pack: cnv1 builds its input patch straight from the raw inputs (mask + pack fused in, the packed tensor never
    // touches HBM).  Measured equal in time to mask_pack + cnv1 (the fused fill is bound by its byte loads), so the two-kernel form
    // stays the default.  The depth-split attention and the three-frame PoseNN have no fused fill, whatever "fuse_pack" says.
    const bool fuse_wanted = o.env_fuse_pack == 1 || o.fuse_pack == 1 || (o.fuse_pack < 0 && B <= FUSE_PACK_MAX_BATCH);
    const bool patch1 = o.env_patch[0] != 0;
    const bool fused = h3 && patch1 && fuse_wanted && !split && !tri;
    p.pack.kind = tri ? PACK_TRIPLET : fused ? PACK_NONE : PACK_PAIR;
    p.pack.ld = h3 ? 16 : direct ? 10 : 8;
    p.pack.packed_ld = tri ? 16 : direct ? 10 : 8;
    p.pack.packed_valid = !fused;
    if (p.pack.kind != PACK_NONE) launch(LB_MASK_PACK);

    // the ladders: cnv1 and cnv2 halve the map, cnv3..cnv6 keep it, cnv7 halves it again; channels per pixel of each stored tensor
    const int H1 = (call.H + 1) / 2, W1 = (call.W + 1) / 2, H2 = (H1 + 1) / 2, W2 = (W1 + 1) / 2, H3 = (H2 + 1) / 2, W3 = (W2 + 1) / 2;
    const int Hs[8] = {call.H, H1, H2, H2, H2, H2, H2, H3}, Ws[8] = {call.W, W1, W2, W2, W2, W2, W2, W3};
    const int ch6 = cpl ? c6 : 2 * c6, ch7 = cpl ? 256 : 512;
    const int packed_ch = direct ? 10 : tri ? 16 : 8;
    const int ch[8] = {packed_ch, 16, 32, 64, 128, 256, ch6, ch7};
    const bool big_map = H3 * W3 >= 128;               // the fused head's tiles of 128 rows must not span more than two images
    // the three-frame PoseNN stores cnv7 (the fused epilogue has three columns per head); the coupled one fuses its six columns in
    // f16x3 (NC = 6), float32 needs the full 256-column tile
    const bool pose_fused = !direct && o.fuse_pose && big_map && !tri && (h3 || (o.npad7 == 256 && !cpl));
    const bool patch_ok[3] = {h3 ? (tri ? o.patch_cnv1_t && !o.forced_tile[0] : patch1) : o.patch_f32 && o.have_patch_f32[0] && p.pack.packed_ld == 8,
                              h3 ? o.patch_cnv2 && !o.forced_tile[1] && o.env_patch[1] != 0 : o.patch_f32 && o.have_patch_f32[1],
                              h3 ? o.patch_cnv3 && !o.forced_tile[2] && o.env_patch[2] != 0 : o.patch_f32 && o.have_patch_f32[2]};
    p.se5 = se;
    for (int li = 0; li < 7; ++li) {
        LayerPlan& r = p.layer[li];
        r.label = li < 5 ? LB_CNV1 + li : li == 5 ? LB_CNV6 : LB_CNV7;
        r.x_buf = li == 0 ? BUF_PACKED : (li == 5 && se) ? BUF_SE : li - 1;      // feature attention: cnv6 reads [cnv5 s_r | cnv5 s_r s_t]
        r.x_ch = (li == 5 && se) ? 512 : ch[li];
        r.Hin = Hs[li]; r.Win = Ws[li]; r.Hout = Hs[li + 1]; r.Wout = Ws[li + 1];
        r.y_ld = ch[li + 1];
        r.y_f32 = !h3 || li == 6;
        if (direct) {
            // impl 1: cnv6 and cnv7 once per head; with feature attention head g reads its half of the scaled tensor
            r.runner = RUN_DIRECT;
            const int heads = (li >= 5 && !cpl) ? 2 : 1;
            r.ngroups = heads;
            r.cin = li == 5 ? 256 : li == 6 ? c6 : ch[li];
            r.cout = li == 5 ? c6 : li == 6 ? 256 : ch[li + 1];
            for (int g = 0; g < heads; ++g) { r.x_coff[g] = (li == 5 && !se) ? 0 : g * r.cin; r.y_coff[g] = g * r.cout; }
            continue;
        }
        r.runner = h3 ? RUN_IGEMM_H3 : RUN_IGEMM_F32;
        if (li < 3 && patch_ok[li]) {
            r.runner = (li == 0 && tri) ? RUN_PATCH_CNV1T : (li == 0 && fused) ? RUN_PATCH_FUSED : RUN_PATCH;
            r.plan_code = ((p.NB * r.Hout * r.Wout + 127) / 128) * 1000 + (r.runner == RUN_PATCH_CNV1T ? PATCH_CNV1T_PLAN_ID : PATCH_PLAN_ID[li]);
        }
        if (li == 6) {
            r.fuse_pose = pose_fused;
            r.pose_tail = h3 && fold_pose;             // the launch's last workgroup adds the tiles and writes the poses (pose_tail.h)
            r.pose_six = h3 && pose_fused && cpl;
        }
    }
    for (int li = 0; li < 5; ++li) launch(p.layer[li].label);
    if (se) { launch(LB_SE5_SQUEEZE); launch(LB_SE5_EXCITE); launch(LB_SE5_SCALE); }
    for (int g = 0; g < p.layer[5].ngroups; ++g) { launch(LB_CNV6); launch(LB_CNV7); }

    // the head.  "fold_tails" 1 drops the pose_head launch wherever the head is fused - in float32 too, which has no pose tail in
    // cnv7 ("Which launches a forward gets": kept as it was found)
    p.head.kind = (pose_fused && fold_pose) ? HEAD_TAIL : pose_fused ? HEAD_TILES : HEAD_TWO_PASS;
    p.head.cols = (cpl || tri) ? 6 : 3;
    p.head.heads = cpl ? 1 : 2;
    p.head.cnv7_valid = !pose_fused;
    if (p.head.kind != HEAD_TAIL) launch(LB_POSE_HEAD);
    // the range guard's conditional copy of the batch's inputs rides in pose_from_tiles; every other head leaves it a launch
    p.head.snapshot_launch = h3 && o.want_snapshot && p.head.kind != HEAD_TILES;
    if (p.head.snapshot_launch) launch(LB_SNAPSHOT);
    return p;
}

}  // namespace davo

// forward.hip — the forward plan of the pose path on one context:
//
//   se_squeeze_partial (se_class_squeeze for the class-table sources) -> se_excite -> mask_pack -> cnv1..cnv5 -> cnv6 (rotation|translation
//   fused into one N = 2*cnv6_out GEMM, both read cnv5: nets/posenn.py:222-238)
//   -> cnv7 (grouped x2) -> pose head.
//   Feature attention (`-se_insert', davo_set_posenn_se): cnv5 -> se5_squeeze -> se5_excite -> se5_scale -> [cnv5 s_r | cnv5 s_r s_t]
//   -> cnv6 as a two-group layer (group g reads channels [256 g, 256 g + 256)) -> cnv7 as before (posenn_se.h).
//
// The two PoseNN calls of a triplet (davo.py:1456-1457, shared weights) run as one batch of
// 2B pair images - or, with one pair selected (davo_set_pairs; params.h), as B pair images: the prologue and the pose kernels map
// a pair image to its (window, source frame), every layer in between takes the count.  Host code only: kernels are reached
// through launch.h.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "ctx.h"
#include "launch.h"
#include "pad_classes.h"
#include "plan.h"

namespace davo {

// ---- profiling ------------------------------------------------------------------------------------
ProfScope::ProfScope(davo_ctx* ctx, hipStream_t stream, const char* name) : c(ctx), s(stream) {
    if (!c->prof) return;
    if (c->prof_dominant_only) {
        if (strcmp(name, "cnv6") != 0) return;
        if (c->prof_tick++ % c->prof_stride != 0) return;
    }
    for (auto& pe : c->prof_entries)
        if (pe.name == name) { e = &pe; break; }
    if (!e) {
        c->prof_entries.emplace_back();
        e = &c->prof_entries.back();
        e->name = name;
    }
    auto get = [&]() {
        EventOwner ev;
        if (!c->event_pool.empty()) { ev = std::move(c->event_pool.back()); c->event_pool.pop_back(); }
        else (void)event_create(&ev);
        return ev;
    };
    a = get(); b = get();
    if (a) (void)hipEventRecord(a.get(), s);
}

ProfScope::~ProfScope() {
    if (!e) return;
    if (b) (void)hipEventRecord(b.get(), s);
    if (a && b) e->pending.emplace_back(std::move(a), std::move(b));
    else {                                    // half a pair is of no use: back to the pool
        if (a) c->event_pool.push_back(std::move(a));
        if (b) c->event_pool.push_back(std::move(b));
    }
}

int sync_all_slots(davo_ctx* c) {
    for (auto& s : c->slots) HIP_TRY(c, hipStreamSynchronize(s.stream.get()));
    if (c->user_stream) HIP_TRY(c, hipStreamSynchronize(c->user_stream));
    return DAVO_OK;
}

int prof_collect(davo_ctx* c) {
    { int rc = sync_all_slots(c); if (rc) return rc; }
    for (auto& pe : c->prof_entries) {
        EventOwner prev_start;
        for (auto& ab : pe.pending) {
            float ms = 0.f, gap = -1.f;
            if (hipEventElapsedTime(&ms, ab.first.get(), ab.second.get()) == hipSuccess) {
                pe.total_ms += ms;
                pe.launches += 1;
                if (prev_start && hipEventElapsedTime(&gap, prev_start.get(), ab.first.get()) != hipSuccess) gap = -1.f;
                if (pe.dur_ms.size() < PROF_SAMPLES_CAP) { pe.dur_ms.push_back(ms); pe.period_ms.push_back(gap); }
            }
            if (prev_start) c->event_pool.push_back(std::move(prev_start));
            prev_start = std::move(ab.first);
            c->event_pool.push_back(std::move(ab.second));
        }
        if (prev_start) c->event_pool.push_back(std::move(prev_start));
        pe.pending.clear();
    }
    return DAVO_OK;
}

namespace {

constexpr int MAX_WEIGHT_CHANNEL_SPREAD_LOG2 = 14;     // f16x3 per-channel guard (weights.hip)
constexpr int FOLD_EXCITE_MAX_BATCH = 2;       // auto modes: largest batch that folds the excitation / fuses mask + pack into cnv1
constexpr int FUSE_PACK_MAX_BATCH = 0;        // measured level at every batch (cnv1 +5 us for mask_pack's 6.7): nowhere by default

// ---- tile orders ------------------------------------------------------------------------------------
// One cache for every launch's table (davo_ctx::tile_orders): `build' is asked once per key for the order, an empty one meaning
// that no table is needed, and the table is uploaded.  A table that cannot be put on the device is not fatal: natural order.
template <class Build>
const int* cached_tile_order(davo_ctx* c, const std::vector<int>& key, Build build) {
    if (!c->opt_skip_order) return nullptr;
    auto it = c->tile_orders.find(key);
    if (it != c->tile_orders.end()) return it->second.get();
    const std::vector<int> order = build();
    DevMem<int> dev;
    if (!order.empty() && !(dev = upload_table(order))) (void)hipGetLastError();
    return (c->tile_orders[key] = std::move(dev)).get();
}

// ---- long tiles first ------------------------------------------------------------------------------
// The 3x3 kernels skip the chunks of filter rows that are all padding for a tile (params.h, valid_filter_rows), so the tiles
// of one launch differ in length (dilation 8 on a 32-row map: 6 of an image's 13 tiles of 256 pixels walk two thirds of the
// chunks).  Workgroups are handed out strictly in id order, an XCD's to its four shader engines round-robin
// (tools/exp/dispatch_probe.hip), and a launch is three to six rounds of tiles: in natural order some CUs draw long tiles
// every round and the launch is as long as before.  The table puts, inside every XCD's contiguous run of tiles (xcd_remap),
// the long tiles first (stable, so neighbours stay neighbours): every engine then sees the same long-first sequence and
// the short tiles pack the end.  Returns nullptr when all tiles of the launch cost the same.
const int* tile_order_for(davo_ctx* c, int li, int kind, int bm, int mtile0, int mtiles, int ntiles_n, int M,
                          int Hout, int Wout, int Hin, int stride, int pad_t, int rate) {
    return cached_tile_order(c, {li, kind, bm, mtile0, mtiles, ntiles_n, M, Hout, Wout}, [&]() {
        const int nt = mtiles * ntiles_n;
        std::vector<int> cost(nt), order(nt);
        bool uniform = true;
        for (int t = 0; t < nt; ++t) {
            const int m0 = (mtile0 + t / ntiles_n) * bm, m1 = std::min(m0 + bm, M) - 1;
            cost[t] = valid_filter_rows(m0, m1, Hout, Wout, Hin, stride, pad_t, rate).nky;
            uniform = uniform && cost[t] == cost[0];
        }
        if (uniform) return std::vector<int>();
        const int q = nt >> 3, r = nt & 7;
        for (int x = 0; x < 8; ++x) {                       // xcd_remap: XCD x runs tiles [start, start + len)
            const int start = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q, len = q + (x < r ? 1 : 0);
            int w = start;
            for (int want = 3; want >= 1; --want)
                for (int t = start; t < start + len; ++t)
                    if (cost[t] == want) order[w++] = t;
        }
        return order;
    });
}

// ---- class-sorted rows (pad_classes.h; "pad_classes") -------------------------------------------------
// The device tables of one layer at one shape: built at the first batch of that shape, kept until the context goes.
// nullptr with *rc set: the tables could not be put on the device - an error, never the natural order in silence.  nullptr with
// *rc DAVO_OK: at this shape the sorted rows walk no fewer taps than the natural order (pad_classes.h), the layer runs without tables.
const PadTables* pad_tables_for(davo_ctx* c, int li, int NB, int Hout, int Wout, int Hin, int Win, int pad_t, int pad_l, int rate, int* rc) {
    *rc = DAVO_OK;
    const std::vector<int> key = {li, NB, Hout, Wout, Hin, Win, pad_t, pad_l, rate};
    auto it = c->pad_tables.find(key);
    if (it != c->pad_tables.end()) return it->second.row_pixel ? &it->second : nullptr;
    PadTables t;
    std::vector<int32_t> rows;
    if (!pad_class_tables(NB, Hout, Wout, Hin, Win, pad_t, pad_l, rate, BM, &rows, &t.host_taps)) {
        c->pad_tables[key] = PadTables();                       // remembered: nothing to build at this shape
        return nullptr;
    }
    if (!(t.row_pixel = upload_table(rows)) || !(t.tile_taps = upload_table(t.host_taps))) {
        *rc = fail(c, DAVO_ERR_HIP, "pad-class tables of layer %d: %s", li, hipGetErrorString(hipGetLastError()));
        return nullptr;
    }
    return &(c->pad_tables[key] = std::move(t));
}

// tile_order_for where the tiles walk their own taps: a tile costs the tap count of its mask, the XCDs' runs are dealt out level
// (pad_classes.h, pad_class_tile_order)
const int* tile_order_pc(davo_ctx* c, int li, int mtile0, int mtiles, int ntiles_n, int M, int Hout, int Wout, const PadTables& t) {
    return cached_tile_order(c, {li, 100, BM, mtile0, mtiles, ntiles_n, M, Hout, Wout}, [&]() {
        std::vector<int> order;
        bool uniform = true;
        for (int m = 1; m < mtiles; ++m) uniform = uniform && tap_count(t.host_taps[mtile0 + m]) == tap_count(t.host_taps[mtile0]);
        if (!uniform) pad_class_tile_order(t.host_taps.data(), mtile0, mtiles, ntiles_n, &order);
        return order;
    });
}

// ---- per-slot scratch -------------------------------------------------------------------------------
// A scratch buffer of the context with one region of *floats floats per in-flight slot: grown (behind every stream) if this launch
// needs more per slot than it has, then -> the region of this batch's slot.  extra_bytes: room behind the regions.
int slot_scratch(davo_ctx* c, const Run& run, GrowBuf* buf, size_t* floats, size_t need, float** region, size_t extra_bytes = 0) {
    if (need > *floats) {
        const size_t bytes = need * sizeof(float) * MAX_INFLIGHT + extra_bytes;         // one region per in-flight slot
        if (buf->get() && bytes > buf->bytes()) { int rs = sync_all_slots(c); if (rs) return rs; }      // only ahead of a free
        *floats = 0;
        HIP_TRY(c, buf->reserve(bytes));
        *floats = need;
    }
    *region = static_cast<float*>(buf->get()) + (size_t)run.slot * *floats;
    return DAVO_OK;
}

// ---- one conv layer, FP32-MFMA path ---------------------------------------------------------------
// fuse_pose (cnv7): the pose head runs in the epilogue (conv_igemm.h); *pose_mt receives the layer's M tiles
int run_conv_layer(davo_ctx* c, const Run& run, int li, const float* x, int x_ld, int Hin, int Win, float* y, int y_ld, int NB, bool fuse_pose = false, int* pose_mt = nullptr) {
    const ConvLayer& L = c->L[li];
    ConvParams p{};
    int Ho, Wo, pt, pl;
    same_pad(Hin, L.KS, L.stride, L.rate, &Ho, &pt);
    same_pad(Win, L.KS, L.stride, L.rate, &Wo, &pl);
    p.x = x; p.w = L.d_w.get(); p.bias = L.d_b.get(); p.y = y; p.zeros = c->d_zeros.get();
    p.Hin = Hin; p.Win = Win; p.Hout = Ho; p.Wout = Wo;
    p.cin_log2 = L.cin_log2; p.x_ld = x_ld; p.x_coff = 0; p.y_ld = y_ld; p.y_coff = 0;
    p.Cout = L.cout; p.pad_t = pt; p.pad_l = pl; p.rate = L.rate;
    p.M = NB * Ho * Wo; p.nchunks = L.nchunks; p.Kpad = L.kpad; p.ntaps = L.KS * L.KS;
    p.ntiles_n = L.npad / L.BN; p.relu = 1;
    if (L.groups == 2) {
        p.g_x_coff = L.cin; p.g_y_coff = L.cout;
        p.g_w = (long)L.npad * L.kpad; p.g_bias = L.npad;
    }
    const int mtiles = (p.M + BM - 1) / BM;
    std::vector<Launch> plan = plan_layer(mtiles, L.npad, L.groups, c->ncu);
    if (li == 0 && L.cout <= 16 && c->opt_f32_n16) plan = {{0, mtiles, 16}};      // cnv1 on the 128x16 tile at every batch size (conv_igemm.h, N16)
    if (fuse_pose) {
        { int rs = slot_scratch(c, run, &c->d_pose_tiles, &c->pose_tiles_floats, (size_t)L.groups * mtiles * 8 * 6, &p.pose_partial); if (rs) return rs; }
        p.pose_w = c->d_wpred.get();
        p.pose_P = Ho * Wo; p.pose_mt = mtiles;
        if (pose_mt) *pose_mt = mtiles;
    }
    c->last_plan[li][0] = c->last_plan[li][1] = 0; c->last_split[li] = 1;
    // cnv4, cnv5, cnv6: GEMM rows sorted by padding class, every tile walks the taps of its own pixels ("pad_classes")
    const PadTables* pc = nullptr;
    if (li >= 3 && li <= 5 && ((c->opt_pad_classes >> (li - 3)) & 1) && L.KS == 3 && L.stride == 1 && L.cin_log2 >= 5 && L.groups == 1 && !fuse_pose && !c->opt_f32_n256) {
        int rc = DAVO_OK;
        pc = pad_tables_for(c, li, NB, Ho, Wo, Hin, Win, pt, pl, L.rate, &rc);
        if (rc) return rc;
        if (pc) { p.row_pixel = pc->row_pixel.get(); p.tile_taps = pc->tile_taps.get(); }
    }
    auto order_for = [&](const Launch& l, int ntn) {
        if (pc) return tile_order_pc(c, li, l.mtile0, l.mtiles, ntn, p.M, Ho, Wo, *pc);
        return (L.KS == 3 && L.cin_log2 >= 5) ? tile_order_for(c, li, 0, BM, l.mtile0, l.mtiles, ntn, p.M, Ho, Wo, Hin, L.stride, pt, L.rate) : nullptr;
    };
    // experiment ("f32_n256"): cnv5 / cnv6 as whole rounds of 128 x 256 tiles (eight waves, one workgroup per CU) + a remainder launch of
    // 128 x 64 tiles
    if (c->opt_f32_n256 && (li == 4 || li == 5) && L.npad == 256 && L.groups == 1 && !fuse_pose && mtiles >= c->ncu) {
        const int main_m = (mtiles / c->ncu) * c->ncu;
        ConvParams pm = p;
        pm.mtile0 = 0; pm.ntiles_n = 1;
        pm.tile_order = tile_order_for(c, li, 2, BM, 0, main_m, 1, p.M, Ho, Wo, Hin, L.stride, pt, L.rate);
        {
            ProfScope ps(c, run.stream, L.label);
            HIP_TRY(c, launch_layer_n256(li, pm, dim3(main_m, 1), run.stream));
        }
        c->last_plan[li][0] = main_m * 1000 + 256;
        if (main_m < mtiles) {
            ConvParams pr = p;
            pr.mtile0 = main_m; pr.ntiles_n = L.npad / 64;
            pr.tile_order = tile_order_for(c, li, 0, BM, main_m, mtiles - main_m, pr.ntiles_n, p.M, Ho, Wo, Hin, L.stride, pt, L.rate);
            const std::string label = std::string(L.label) + ".rem";
            ProfScope ps(c, run.stream, label.c_str());
            HIP_TRY(c, launch_layer(li, 64, pr, dim3((mtiles - main_m) * pr.ntiles_n, 1), run.stream));
            c->last_plan[li][1] = (mtiles - main_m) * 1000 + 64;
        }
        return DAVO_OK;
    }
    // main + remainder as one grid (conv_igemm.h, conv_igemm_f32_mainrem; "merge_rem_f32"): the remainder's tiles start on the CUs
    // that finish their last main tile first, instead of behind a launch boundary.  Same tiles, same arithmetic.
    // (cnv7 keeps its two launches: merged it measured 0.532 against 0.439 + 0.052 ms - its 32-column remainder tiles then run two per CU
    // on the main tile's LDS and register budget instead of three, and 0.545 with a 64-column remainder; cnv4 / cnv5 / cnv6: -5 / -4 / -1 %,
    // profiles/r05q_f32_mainrem_ab.md)
    if (c->opt_merge_rem_f32 && li >= 3 && (li <= 5 || c->opt_merge_rem_f32 > 1) && plan.size() == 2 && plan[0].BN == 128 && (plan[1].BN == 32 || plan[1].BN == 64)) {
        ConvParams pm = p, pr = p;
        pm.mtile0 = plan[0].mtile0; pm.ntiles_n = L.npad / 128; pm.tile_order = order_for(plan[0], pm.ntiles_n);
        pr.mtile0 = plan[1].mtile0; pr.ntiles_n = L.npad / plan[1].BN; pr.tile_order = order_for(plan[1], pr.ntiles_n);
        const int n_main = plan[0].mtiles * pm.ntiles_n, n_rem = plan[1].mtiles * pr.ntiles_n;
        if (n_main % 8 == 0 && (L.groups == 1 || n_rem % 8 == 0)) {
            ProfScope ps(c, run.stream, L.label);
            HIP_TRY(c, launch_layer_mainrem(li, plan[1].BN, pm, pr, n_main, n_rem, L.groups, run.stream));
            c->last_plan[li][0] = (plan[0].mtiles + plan[1].mtiles) * 1000 + 128;      // one launch covers the layer
            return DAVO_OK;
        }
    }
    for (size_t i = 0; i < plan.size(); ++i) {
        p.mtile0 = plan[i].mtile0;
        p.ntiles_n = plan[i].BN == 16 ? 1 : L.npad / plan[i].BN;
        dim3 grid(plan[i].mtiles * p.ntiles_n, L.groups);
        p.tile_order = order_for(plan[i], p.ntiles_n);
        const std::string label = i == 0 ? std::string(L.label) : std::string(L.label) + ".rem";
        ProfScope ps(c, run.stream, label.c_str());
        HIP_TRY(c, launch_layer(li, plan[i].BN, p, grid, run.stream));
        c->last_plan[li][i] = plan[i].mtiles * 1000 + plan[i].BN;
    }
    return DAVO_OK;
}

// ---- one conv layer, f16x3 path: x and y are split-fp16 blocked tensors (y float32 when y_f32) -----
int run_conv_layer_h3(davo_ctx* c, const Run& run, int li, const void* x, int x_ch, int Hin, int Win, void* y, int y_ld,
                      bool y_f32, int NB, bool fuse_pose = false, int* pose_bm = nullptr, int* pose_mt = nullptr,
                      int* pose_ntn = nullptr, float* pose_out = nullptr) {
    const ConvLayer& L = c->L[li];
    ConvParamsH p{};
    int Ho, Wo, pt, pl;
    same_pad(Hin, L.KS, L.stride, L.rate, &Ho, &pt);
    same_pad(Win, L.KS, L.stride, L.rate, &Wo, &pl);
    p.x = static_cast<const uint8_t*>(x); p.w = L.d_wh.get(); p.bias = L.d_bh.get(); p.y = static_cast<uint8_t*>(y);
    p.zeros = reinterpret_cast<const uint8_t*>(c->d_zeros.get());
    p.Hin = Hin; p.Win = Win; p.Hout = Ho; p.Wout = Wo;
    p.x_pix_bytes = (long)x_ch * 4; p.x_boff = 0; p.x_pix_log2 = ilog2_exact(x_ch * 4);
    p.cb_log2 = L.cb_log2; p.tpc_log2 = L.tpc_log2; p.cpb = L.cpb; p.nchunks = L.nchunks_h;
    p.w_row_bytes = (long)L.nchunks_h * 128;
    p.y_mode = y_f32 ? 0 : 1; p.y_ld = y_ld; p.y_coff = 0; p.Cout = L.cout;
    p.pad_t = pt; p.pad_l = pl; p.rate = L.rate;
    p.M = NB * Ho * Wo; p.ntaps = L.KS * L.KS; p.mtile0 = 0; p.relu = 1;
    p.Mtot = p.M; p.xs = c->opt_share_taps ? 1 : 0;
    {   // stored activations carry 2^act_shift (exact); cnv7 feeds the float32 pose head unscaled
        const int sin = li == 0 ? 0 : c->act_shift[li - 1], sout = li == 6 ? 0 : c->act_shift[li];
        p.out_scale = ldexpf(1.0f / L.wscale, sout - sin);
        p.bias_scale = ldexpf(L.wscale, sin);
        p.range = run.range ? run.range + li : nullptr;
    }
    if (L.groups == 2) {
        p.g_x_boff = L.cin * 4; p.g_y_coff = L.cout;
        p.g_w = (long)L.npad_h * p.w_row_bytes; p.g_bias = L.npad_h;
    }
    if (const char* e = tuning_env("DAVO_DBG")) p.dbg = atoi(e);       // tuning build only
    // cnv5, cnv6, cnv7 (256 channels per group) and cnv4 (128): conv_igemm_h3s.h is instantiated for them
    const bool allow_208 = (li >= 4 && L.npad_h == 256) || (li == 3 && L.npad_h == 128 && c->opt_tile_208x128);
    // cnv5 / cnv6 with "wave128": the 256x256 tile is conv_igemm_h3w's, 4.7 % faster than the one the planner's table was fitted on
    // (measured across 21 batch sizes with the table scaled: only B = 24 and 256x832 B = 6 change plan, -2.7 / -3.2 %: profiles/r05bn_planner_scale.log)
    const double others_scale = (c->opt_wave128 && (li == 4 || li == 5) && L.npad_h == 256 && L.groups == 1 && !fuse_pose) ? 0.955 : 1.0;
    std::vector<LaunchH> plan = plan_layer_h3(p.M, L.npad_h, L.groups, L.tile_h, allow_208, c->ncu, others_scale);
    if (fuse_pose) {      // one launch, one tile shape no taller than an image, so a tile touches <= 2 images
        const int P = Ho * Wo;
        const int best = plan_single_tile_h3(p.M, L.npad_h, L.groups, P, L.tile_h, allow_208, c->ncu);
        if (best < 0) return fail(c, DAVO_ERR_INVALID, "no tile fits the fused pose head");
        plan = {{0, p.M, best}};
        const TileShape ts = tile_shape(best);
        const int mt = (p.M + ts.bm - 1) / ts.bm, ntn = L.npad_h / ts.bn;
        size_t debug_bytes = 0;
#ifdef DAVO_POSE_DEBUG
        debug_bytes = (size_t)L.groups * mt * ntn * 512 * 20 * sizeof(float);
#endif
        { int rs = slot_scratch(c, run, &c->d_pose_tiles, &c->pose_tiles_floats, (size_t)L.groups * mt * ntn * 6, &p.pose_partial, debug_bytes); if (rs) return rs; }
        p.y_mode = 2; p.pose_w = c->d_wpred.get();
        p.pose_P = P; p.pose_mt = mt;
        if (pose_out) {      // the launch's last workgroup adds the tiles and writes the poses (pose_tail.h)
            p.pose_counter = c->slots[run.slot].d_counters.get(); p.pose_bias = c->d_bpred.get(); p.pose_out = pose_out;
            p.pose_NB = NB; p.pose_bm = ts.bm; p.pose_total = L.groups * mt * ntn; p.pose_sel = run.pairs;
        }
        if (pose_bm) *pose_bm = ts.bm;
        if (pose_mt) *pose_mt = mt;
        if (pose_ntn) *pose_ntn = ntn;
    }
    c->last_plan[li][0] = c->last_plan[li][1] = 0; c->last_split[li] = 1;
    // cnv4 on conv_igemm_h3w128's 256 x 128 tiles, every row in one launch - where the 256-row tiles fill whole rounds of the CUs or
    // nearly so: a round of them takes 24.4 us against 29.2 for the same rows on conv_igemm_h3's tiles (B = 128: 0.385 -> 0.318 ms),
    // which a last round that is three quarters empty gives back (B = 32, 3.25 rounds: 0.0925 -> 0.0938 ms)
    const long t256 = (p.M + 255) / 256;
    const bool rounds_ok = t256 >= c->ncu && (double)((t256 + c->ncu - 1) / c->ncu) * c->ncu <= 1.12 * (double)t256;
    if ((c->opt_wave128 >= 3 || (c->opt_wave128 >= 2 && rounds_ok)) && li == 3 && !fuse_pose && L.groups == 1 && L.npad_h == 128 && L.tile_h < 0 &&
        p.M >= 256 * c->ncu) {
        ConvParamsH pw = p;
        pw.ntiles_n = 1; pw.mtile0 = 0;
        if (layer_h3w128_supported(pw)) {
            {
                ProfScope ps(c, run.stream, L.label);
                HIP_TRY(c, launch_layer_h3w128(pw, run.stream));
            }
            c->last_plan[li][0] = ((p.M + 127) / 128) * 1000 + TILE_256x128;
            return DAVO_OK;
        }
    }
    if (c->opt_merge_cnv4 && c->opt_merge_rem && li == 3 && !fuse_pose && L.npad_h == 128 && L.groups == 1 && c->ncu == 256 && L.tile_h < 0 &&
        plan.size() == 1 && plan[0].tile == TILE_128x128) {
        // cnv4 (N = 128): whole rounds of 256x128 tiles (shared-tap staging, twice the matrix work per staged byte of the
        // 128x128 tile) + the remaining rows on 128x128 tiles, as one grid like cnv5 / cnv6 below
        const int rows1 = (p.M / 256 / c->ncu) * c->ncu * 256;
        const int rem = p.M - rows1, n_rem = (rem + 127) / 128;
        if (rows1 > 0 && rem > 0 && rem % 128 == 0 && n_rem % 64 == 0 && n_rem <= 256)
            plan = {{0, rows1, TILE_256x128}, {rows1, rem, TILE_128x128}};
    }
    const bool merge_256 = plan.size() == 2 && plan[0].tile == TILE_256x256 && plan[1].tile == TILE_128x128 && L.npad_h == 256;
    // the merged grid's 256x128 main tile is instantiated for cnv4 alone (launch_h3.hip): a cnv6 of 128 columns (-cnv6_64) with the same
    // plan keeps its two launches
    const bool merge_128 = li == 3 && plan.size() == 2 && plan[0].tile == TILE_256x128 && plan[1].tile == TILE_128x128 && L.npad_h == 128;
    if (c->opt_merge_rem && !fuse_pose && (merge_256 || merge_128) && L.groups == 1 && c->ncu == 256 && !tuning_env("DAVO_NO_MERGE")) {
        // main + remainder as one grid (conv_igemm_h3_mainrem): same tiles, same arithmetic, de-phased store bursts
        ConvParamsH pm = p, pr = p;
        const int rem_ntn = L.npad_h / 128;                       // N tiles of a 128x128 remainder row block
        pm.ntiles_n = 1; pm.mtile0 = 0; pm.M = plan[0].rows;
        pr.ntiles_n = rem_ntn; pr.mtile0 = plan[1].row0 / 128; pr.M = plan[1].row0 + plan[1].rows;
        const int n_main = plan[0].rows / 256, n_rem = ((plan[1].rows + 127) / 128) * rem_ntn;
        // the shape test comes first: a profiling scope is opened only around a launch that is really issued
        // (an empty event pair under the layer's label would halve its average and advance the stride counter twice)
        // "wave128": the four-wave main tile (conv_igemm_h3w.h) runs as a launch of its own - merged with four-wave remainder tiles it
        // measured 0.262 / 0.497 ms for cnv5 / cnv6 against 0.258 / 0.487 as two launches (profiles/r05bc_w128_ab.log)
        const bool own_launch = c->opt_wave128 && merge_256 && layer_h3w_supported(li, pm);
        if (!own_launch && layer_h3_mainrem_supported(li, pm, n_main, n_rem)) {
            // f16x3: long-first measured 256.8 against 259.9 us on cnv5 with a third more HBM reads (205 -> 272 MB: neighbours no longer
            // run side by side) and no change of the power-capped step: natural order unless "skip_order" is 2
            pm.tile_order = c->opt_skip_order >= 2 ? tile_order_for(c, li, 1, 256, 0, n_main, 1, pm.M, Ho, Wo, Hin, L.stride, pt, L.rate) : nullptr;
            const int order = c->opt_merge_order >= 0 ? c->opt_merge_order : (pm.tile_order ? 2 : 0);
            {
                ProfScope ps(c, run.stream, L.label);
                HIP_TRY(c, launch_layer_h3_mainrem(li, pm, n_main, pr, n_rem, order, run.stream));
            }
            c->last_plan[li][0] = ((plan[0].rows + plan[1].rows + 127) / 128) * 1000 + 7;     // 7: 256x256 + 128x128 in one grid
            return DAVO_OK;
        }
    }
    // Split-K.  A launch of at most half a workgroup per CU (cnv6 at batch 1: 104 tiles of 128x128, each a serial chain of 72
    // chunks at ~0.7 us) leaves half of the chip idle and is as long as its chain: the two halves of the input channels run
    // as two "groups" of the same kernel (the grouped-convolution path cnv7 uses: own channel offset, weight offset and
    // output slot; the second half starts from a zero bias) into float32 partial sums, and splitk_fixup adds the two,
    // applies ReLU and writes the stored form.  Two partial sums instead of one chain change the float32 rounding of the
    // layer's outputs (not their value: ~1e-7 relative), so batch sizes that split and batch sizes that do not agree to
    // rounding, not to the bit ("split_k" 0 restores the single chain).  (With S parts: S groups, S partial sums.)
    if (c->opt_split_k && !fuse_pose && (li == 4 || li == 5) && L.groups == 1 && plan.size() == 1 && p.y_mode == 1 && L.cout % 32 == 0 &&
        !is_208(plan[0].tile)) {
        const TileShape ts = tile_shape(plan[0].tile);
        const int mtiles = (p.M + ts.bm - 1) / ts.bm, ntn = L.npad_h / ts.bn;
        const long tiles = (long)mtiles * ntn;
        // parts: whole channel blocks each, whole filter rows (shared-tap staging walks a row's three taps together).  Four parts
        // where the workgroups then still fit side by side (two per CU on the two-slot ring), else two (one per CU, deep ring)
        auto fits = [&](int S) { return L.nchunks_h % (S * L.cpb) == 0 && ((L.nchunks_h / S) % 3) == 0; };
        const int per_cu = ts.lds * 2 <= 160 * 1024 ? 2 : 1;
        const int S = (fits(4) && tiles * 4 <= (long)per_cu * c->ncu && tiles * 2 <= c->ncu) ? 4 : (fits(2) && tiles * 2 <= c->ncu ? 2 : 1);       // two parts at two per CU (B = 2) measured slower: 54 -> 57 us
        if (S > 1) {
            float* part = nullptr;
            { int rs = slot_scratch(c, run, &c->d_splitk, &c->splitk_floats, (size_t)p.M * S * L.cout, &part); if (rs) return rs; }
            ConvParamsH ps = p;
            ps.nchunks = L.nchunks_h / S;
            ps.g_x_boff = (L.cin / S) * 4; ps.g_w = (long)ps.nchunks * 128; ps.g_bias = L.npad_h; ps.g_y_coff = L.cout;
            ps.y = reinterpret_cast<uint8_t*>(part); ps.y_mode = 0; ps.y_ld = S * L.cout; ps.relu = 0; ps.range = nullptr;
            ps.ntiles_n = ntn; ps.mtile0 = 0;
            dim3 grid(mtiles * ntn, S);
            ps.deep = c->opt_deep_ring && tiles * S <= c->ncu;
            c->last_plan[li][0] = ((p.M + 127) / 128) * 1000 + plan[0].tile; c->last_split[li] = S;
            // The fix-up folded into the launch (pose_tail.h, splitk_tail): with an x extent that is a multiple of 8 the S parts of a
            // tile run on one XCD, so the part that finishes last finds the others' partial sums in its own L2 and writes the stored
            // form itself - no splitk_fixup launch (7 us each at batch 1, two per forward).  Checked once per context on the device.
            bool fold = c->opt_fold_fixup && S <= 4 && grid.x % 8 == 0 && (int)grid.x <= SK_TILE_COUNTERS && c->ncu == c->dev_cus && !c->cu_partition &&
                        !c->user_stream;
            if (fold && c->xcd_rr < 0) {
                int ok = 0;
                HIP_TRY(c, xcd_round_robin_probe(run.stream, &ok));
                c->xcd_rr = ok;
            }
            fold = fold && c->xcd_rr > 0;
            if (fold) {
                ps.sk_counter = c->slots[run.slot].d_counters.get() + 1 + c->max_batch;
                ps.sk_y = p.y; ps.sk_range = p.range; ps.sk_parts = S; ps.sk_relu = 1;
            }
            ProfScope pscope(c, run.stream, L.label);
            HIP_TRY(c, launch_layer_h3(li, plan[0].tile, ps, grid, run.stream));
            if (!fold) HIP_TRY(c, launch_splitk_fixup(part, p.M, L.cout, S, 1, p.y, p.range, run.stream));
            return DAVO_OK;
        }
    }
    for (size_t i = 0; i < plan.size() && i < 2; ++i) {
        const TileShape ts = tile_shape(plan[i].tile);
        p.ntiles_n = L.npad_h / ts.bn;
        p.mtile0 = plan[i].row0 / ts.bm;
        const int full_m = p.M;
        p.M = plan[i].row0 + plan[i].rows;                    // rows past this launch's range are not its job
        const int mtiles = (plan[i].rows + ts.bm - 1) / ts.bm;
        dim3 grid(mtiles * p.ntiles_n, L.groups);
        p.deep = c->opt_deep_ring && plan.size() == 1 && (long)grid.x * grid.y <= c->ncu;       // at most one workgroup per CU
        c->last_plan[li][i] = ((plan[i].rows + 127) / 128) * 1000 + plan[i].tile;
        // no tile order here: cnv4's single launch of 128x128 tiles (two per CU, 6.5 rounds) measured 94.4 us in natural order and
        // 97.4 long-first (profiles/r04e_skip_padding_rows.md); the merged grids above and the float32 launches take one
        const std::string label = i == 0 ? std::string(L.label) : std::string(L.label) + ".rem";
        {
            ProfScope ps(c, run.stream, label.c_str());
            bool done = false;
            if (c->opt_wave128 && L.groups == 1 && !fuse_pose) {
                if (plan[i].tile == TILE_256x256 && layer_h3w_supported(li, p)) {
                    HIP_TRY(c, launch_layer_h3w(li, p, grid, run.stream));
                    done = true;
                } else if (c->opt_wave128 >= 2 && i == 1 && plan.size() == 2 && plan[0].tile == TILE_256x256 && plan[1].tile == TILE_128x128 &&
                           L.npad_h == 256 && plan[1].row0 % 256 == 0 && plan[1].rows % 256 == 0) {
                    // the remainder rows of a layer whose main launch ran on conv_igemm_h3w: 256 x 64 tiles (conv_igemm_h3w64)
                    ConvParamsH pr = p;
                    pr.ntiles_n = 4; pr.mtile0 = plan[1].row0 / 256;
                    const hipError_t e = launch_layer_h3w64(li, pr, run.stream);
                    if (e == hipSuccess) done = true;
                    else if (e != hipErrorNotSupported) HIP_TRY(c, e);
                }
            }
            if (!done) HIP_TRY(c, launch_layer_h3(li, plan[i].tile, p, grid, run.stream));
        }
        p.M = full_m;
    }
    return DAVO_OK;
}

// cnv1 / cnv2 / cnv3 (li 0..2) from an LDS-staged input patch: conv_patch_h3.h (x and y split-fp16 blocked) or, f32, conv_patch_f32.h
// (x and y float32 NHWC).  fused (f16x3 cnv1): the patch is built from the raw inputs (mask + pack fused in); otherwise it is
// copied from x, for cnv1 the packed tensor.
struct PatchLayer { int tw, th, per_cu, plan_id; };       // output tile; workgroups per CU, each walks its tiles; id in last_plan
constexpr PatchLayer PATCH_LAYERS[3] = {
    {cp1::TW, cp1::TH, 3, 99},
    {cp2::TW, cp2::TH, 2, 98},       // f16x3: 120 weight registers per lane; float32: three per CU measured 4 % slower
    {cp3::TW, cp3::TH, 3, 97}};      // its padding, cp3::RATE on every side, is what SAME padding gives a 3x3 at dilation 2

int run_patch_layer(davo_ctx* c, const Run& run, int li, bool f32, const void* x, void* y, int NB, bool fused = false, const Inputs& in = Inputs{}) {
    const ConvLayer& L = c->L[li];
    const PatchLayer& t = PATCH_LAYERS[li];
    const uint8_t* const w_h3[3] = {c->d_w1patch.get(), c->d_w2patch.get(), c->d_w3patch.get()};
    const float* const w_f32[3] = {c->d_w1patch_f32.get(), c->d_w2patch_f32.get(), c->d_w3patch_f32.get()};
    const int Hin[3] = {c->H, c->H1, c->H2}, Win[3] = {c->W, c->W1, c->W2};
    ConvPatchParams p{};
    same_pad(Hin[li], L.KS, L.stride, L.rate, &p.Ho, &p.pad_t);
    same_pad(Win[li], L.KS, L.stride, L.rate, &p.Wo, &p.pad_l);
    p.x = static_cast<const uint8_t*>(x); p.w = f32 ? reinterpret_cast<const uint8_t*>(w_f32[li]) : w_h3[li];
    p.bias = f32 ? L.d_b.get() : L.d_bh.get(); p.y = static_cast<uint8_t*>(y);
    p.zeros = reinterpret_cast<const uint8_t*>(c->d_zeros.get());
    p.H = Hin[li]; p.W = Win[li];
    p.tiles_x = (p.Wo + t.tw - 1) / t.tw; p.tiles_y = (p.Ho + t.th - 1) / t.th;
    p.ntiles = NB * p.tiles_x * p.tiles_y;
    if (!f32) {      // stored activations carry 2^act_shift (exact); cnv1's input carries none
        const int sin = li == 0 ? 0 : c->act_shift[li - 1];
        p.out_scale = ldexpf(1.0f / L.wscale, c->act_shift[li] - sin);
        p.bias_scale = ldexpf(L.wscale, sin);
        p.range = run.range ? run.range + li : nullptr;
        if (const char* e = tuning_env("DAVO_PDBG")) p.dbg = atoi(e);      // tuning build only
        if (li == 0) {
            p.img = static_cast<const uint8_t*>(in.img); p.flow = static_cast<const float*>(in.flow);
            p.seg = in.seg; p.tab = c->slots[run.slot].d_tab.get(); p.v = c->v; p.sel = run.pairs;
        }
    }
    c->last_plan[li][0] = ((NB * p.Ho * p.Wo + 127) / 128) * 1000 + t.plan_id; c->last_plan[li][1] = 0; c->last_split[li] = 1;
    const int nblk = p.ntiles < t.per_cu * c->ncu ? p.ntiles : t.per_cu * c->ncu;
    ProfScope ps(c, run.stream, L.label);
    HIP_TRY(c, launch_patch_layer(li, f32, fused, p, nblk, run.stream, c->label_fmt));
    return DAVO_OK;
}

int run_direct(davo_ctx* c, const Run& run, const char* label, const float* x, int N, int Hin, int Win, int cin, int x_ld,
               int x_coff, const std::string& wname, const std::string& bname, int KS, int cout, int stride,
               int rate, float* y, int y_ld, int y_coff) {
    int Ho, Wo, pt, pl;
    same_pad(Hin, KS, stride, rate, &Ho, &pt);
    same_pad(Win, KS, stride, rate, &Wo, &pl);
    for (const std::string* n : {&wname, &bname}) {            // impl 1 is the only reader of the raw device copies: made on demand
        HostTensor& t = c->weights.at(*n);
        if (!t.dev) { int rc = upload(c, t.data, &t.dev); if (rc) return rc; }
    }
    ProfScope ps(c, run.stream, label);
    HIP_TRY(c, launch_conv_direct(x, N, Hin, Win, cin, x_ld, x_coff, c->weights.at(wname).dev.get(), KS, cout,
                                  c->weights.at(bname).dev.get(), stride, rate, pt, pl, Ho, Wo, 1, y, y_ld, y_coff, run.stream));
    return DAVO_OK;
}

// feature attention (posenn_se.h): cnv5 (x, in the mode's storage) -> the slot's d_se = [x s_r | x s_r s_t], 512 channels of cnv5's geometry
int run_posenn_se(davo_ctx* c, const Run& run, bool h3, const void* x, int NB) {
    static const char* const heads[2] = {"rotation", "translation"};
    static const char* const parts[4] = {"bottleneck_fc/kernel", "bottleneck_fc/bias", "recover_fc/kernel", "recover_fc/bias"};
    const float* w[8];
    for (int h = 0; h < 2; ++h)
        for (int k = 0; k < 4; ++k) {
            const auto it = c->weights.find(std::string("pose_exp_net/pose/") + heads[h] + "/cnv5_se_attention/" + parts[k]);
            if (it == c->weights.end() || !it->second.dev) return fail(c, DAVO_ERR_NOT_READY, "feature-attention weights not loaded");
            w[h * 4 + k] = it->second.dev.get();
        }
    if (!c->slots[run.slot].se) return fail(c, DAVO_ERR_INVALID, "internal: no feature-attention workspace");
    const SeWorkspace& ws = *c->slots[run.slot].se;
    const int P = c->H2 * c->W2;
    {
        ProfScope ps(c, run.stream, "se5_squeeze");
        HIP_TRY(c, launch_se5_squeeze(h3, x, NB, P, ws.d_se_partial.get(), run.stream));
    }
    {
        ProfScope ps(c, run.stream, "se5_excite");
        HIP_TRY(c, launch_se5_excite(ws.d_se_partial.get(), NB, P, h3 ? ldexpf(1.0f, -c->act_shift[4]) : 1.0f, w, ws.d_se_scale.get(), run.stream));
    }
    ProfScope ps(c, run.stream, "se5_scale");
    HIP_TRY(c, launch_se5_scale(h3, x, ws.d_se_scale.get(), NB, P, ws.d_se.get(), (h3 && run.range) ? run.range + RANGE_SE : nullptr, run.stream));
    return DAVO_OK;
}

}  // namespace

int forward_device(davo_ctx* c, const Run& run, int B, const Inputs& in, void* d_pose, RunResult* res) {
    const int sel = run.pairs;
    if (sel != PAIRS_SRC0 && sel != PAIRS_SRC1 && sel != PAIRS_BOTH) return fail(c, DAVO_ERR_INVALID, "internal: pair selection %d", sel);
    if (B < 1 || B > c->max_batch) return fail(c, DAVO_ERR_INVALID, "batch %d outside [1,%d]", B, c->max_batch);
    if (!in.img || !in.flow || !in.seg || !d_pose) return fail(c, DAVO_ERR_INVALID, "null device pointer");
    if (needs_depth(c) && (!in.depth || ((uintptr_t)in.depth & 15)))
        return fail(c, DAVO_ERR_INVALID, "this variant reads depth planes: a 16-byte aligned device pointer is required");
    {
        std::string names;
        if (missing_weights(c, &names)) return fail(c, DAVO_ERR_NOT_READY, "weights not loaded: %s", names.c_str());
    }
    HIP_TRY(c, hipSetDevice(c->device));
    c->forward_seen = true;
    c->last_slot = run.slot;
    if (!c->pred_ready) { int rc = build_pred_weights(c); if (rc) return rc; }
    bool h3 = run.impl == 0 && run.precision == 1, f32_fallback = false;
    if (h3 && !c->packed_h_ready) { int rc = build_packed_weights_h3(c); if (rc) return rc; }
    if (h3 && c->weight_channel_spread_log2 > MAX_WEIGHT_CHANNEL_SPREAD_LOG2) {
        // a consumer's per-input-channel weight norms span more than 2^14: per-layer storage scales cannot keep every channel's fp16
        // pair float32-grade (weights.hip).  The reference's float32 graph has no such limit (nets/posenn.py:205-215): float32 kernels.
        if (!c->opt_auto_range)
            return fail(c, DAVO_ERR_RANGE, "`%s': per-input-channel weight norms span 2^%d (> 2^%d): the f16x3 storage cannot hold every channel "
                        "float32-grade - davo_set_precision(ctx, 0), or leave \"auto_range\" on", c->weight_channel_spread_layer.c_str(),
                        c->weight_channel_spread_log2, MAX_WEIGHT_CHANNEL_SPREAD_LOG2);
        h3 = false;
        f32_fallback = true;                 // counted once per API call by the caller (api.hip)
        char note[256];
        snprintf(note, sizeof note, "float32 kernels: per-input-channel weight norms of `%s' span 2^%d (> 2^%d)",
                 c->weight_channel_spread_layer.c_str(), c->weight_channel_spread_log2, MAX_WEIGHT_CHANNEL_SPREAD_LOG2);
        c->range_report = note;
    }
    if (!h3 && run.impl == 0 && !c->packed_ready) { int rc = build_packed_weights(c); if (rc) return rc; }      // float32 kernels: packed at their first use
    unsigned* const range_reset = (h3 && run.zero_record) ? run.range : nullptr;

    const int H = c->H, W = c->W, HW = H * W, NB = pairs_per_window(sel) * B;
    const Variant& v = c->v;
    const Slot& ws = c->slots[run.slot];
    float *const d_partial = ws.d_partial.get(), *const d_tab = ws.d_tab.get(), *const d_packed = ws.d_packed.get();
    float* const d_se = ws.se ? ws.se->d_se.get() : nullptr;                  // feature attention: cnv6's input (run_posenn_se fills it)
    unsigned* const d_counters = ws.d_counters.get();
    float* a[7];
    for (int i = 0; i < 7; ++i) a[i] = ws.d_act[i].get();
    hipStream_t s = run.stream;
    const uint8_t* const d_img = static_cast<const uint8_t*>(in.img);
    const float* const d_flow = static_cast<const float*>(in.flow);
    const void* const d_seg = in.seg;                          // float32 or bytes: c->label_fmt
    auto wdev = [&](const char* n) -> const float* {
        auto it = c->weights.find(n);
        return it == c->weights.end() ? nullptr : it->second.dev.get();
    };
    // Launches are ~6 us each whatever they do; at batch 1 the path is 11 of them around 0.1 ms of work.  Where a launch can be
    // folded into its neighbour at less than that, small batches do it (measured per batch: profiles/):
    //   the excitation MLP in the squeeze launch's last workgroup (costs two memory-side round trips per workgroup: +2 us at
    //   B = 1, +18 us at B = 32), mask + pack inside cnv1's patch fill (level at B = 32).
    const bool class_table = att_class_table(v.att_source);
    const bool fold_excite = (att_flow_squeeze(v.att_source) || class_table) &&
                             (c->opt_fold_tails >= 1 || (c->opt_fold_tails < 0 && B <= FOLD_EXCITE_MAX_BATCH));
    const bool fold_pose = c->opt_fold_tails == 1;
    const float* se_w1 = wdev(se_weight_name(v.att_source, 0));
    const float* se_b1 = wdev(se_weight_name(v.att_source, 1));
    const float* se_w2 = wdev(se_weight_name(v.att_source, 2));
    const float* se_b2 = wdev(se_weight_name(v.att_source, 3));
    const bool depth_split = v.att_source == ATT_DEPTH_SPLIT;
    const float* far_w[4] = {nullptr, nullptr, nullptr, nullptr};
    float* const d_tab_far = ws.d_tab_far.get();
    if (depth_split) {
        for (int k = 0; k < 4; ++k) far_w[k] = wdev(se_far_weight_name(k));
        if (!d_tab_far || !se_w1 || !se_b1 || !se_w2 || !se_b2 || !far_w[0] || !far_w[1] || !far_w[2] || !far_w[3])
            return fail(c, DAVO_ERR_INVALID, "internal: the depth-split attention's tables or dense tensors are missing");
    }
    if (att_desc_depth(v.att_source)) {
        // depth sources: one float32 sum per depth plane and chunk, then (or, folded, in the same launch) the excitation
        ProfScope ps(c, run.stream, "se_depth_squeeze");
        HIP_TRY(c, launch_se_depth_squeeze(fold_excite, static_cast<const float*>(in.depth), B, HW, v, reinterpret_cast<unsigned*>(d_partial),
                                           d_counters + 1, se_w1, se_b1, se_w2, se_b2, d_tab, range_reset, sel, s));
    } else if (class_table) {
        // segmentation / rgb / seg+flow sources: per-frame histogram, byte or flow sums, then (or, folded, in the same launch) the
        // excitation
        ProfScope ps(c, run.stream, "se_class_squeeze");
        HIP_TRY(c, launch_se_class_squeeze(fold_excite, d_img, d_flow, d_seg, c->label_fmt, B, H, W, v, reinterpret_cast<unsigned*>(d_partial),
                                           d_counters + 1, se_w1, se_b1, se_w2, se_b2, d_tab, range_reset, sel, s));
    } else if (fold_excite && depth_split) {
        // the flagship's squeeze; the triplet's last workgroup evaluates the near tables and the far tables from the same sums
        ProfScope ps(c, run.stream, "se_squeeze_partial");
        const float* near_w[4] = {se_w1, se_b1, se_w2, se_b2};
        HIP_TRY(c, launch_se_squeeze_excite_split(d_flow, B, HW, v, d_partial, d_counters + 1, near_w, far_w, d_tab, d_tab_far, range_reset, sel, s));
    } else if (fold_excite) {
        // squeeze + excitation in one launch: the workgroup that delivers a triplet's last partial sum evaluates its tables
        ProfScope ps(c, run.stream, "se_squeeze_partial");
        HIP_TRY(c, launch_se_squeeze_excite(d_flow, B, HW, v, d_partial, d_counters + 1,
                                            se_w1, se_b1, se_w2, se_b2,
                                            wdev("pose_exp_net/pose_exp_net/seg_channel_weight/weight"), d_tab, range_reset, sel, s));
    } else if (att_flow_squeeze(v.att_source)) {
        ProfScope ps(c, run.stream, "se_squeeze_partial");
        HIP_TRY(c, launch_se_squeeze(d_flow, B, HW, v, d_partial, sel, s));
    }
    if (!fold_excite) {
        ProfScope ps(c, run.stream, "se_excite");
        HIP_TRY(c, launch_se_excite(d_partial, B, HW, v, se_w1, se_b1, se_w2, se_b2,
                                    wdev("pose_exp_net/pose_exp_net/seg_channel_weight/weight"), d_tab, range_reset, sel, s));
    }
    if (!fold_excite && depth_split) {
        // depth-split: the same launch again on the far MLP, reading the same partial sums (a profile entry of its own, so that
        // "se_excite" is one launch per forward in every variant)
        ProfScope ps(c, run.stream, "se_excite_far");
        HIP_TRY(c, launch_se_excite(d_partial, B, HW, v, far_w[0], far_w[1], far_w[2], far_w[3], nullptr, d_tab_far, nullptr, sel, s));
    }
    // f16x3, fuse_pack: cnv1 builds its input patch straight from the raw inputs (mask + pack fused in,
    // the packed tensor never touches HBM).  Measured equal in time to mask_pack + cnv1 (the fused fill is bound
    // by its byte loads), so the two-kernel form stays the default.  Tuning build: DAVO_FUSE_PACK=1 / DAVO_CNV1_PATCH=0.
    const char* fe = tuning_env("DAVO_FUSE_PACK");
    const char* pe = tuning_env("DAVO_CNV1_PATCH");
    const bool fuse_env = (fe && atoi(fe) == 1) || c->opt_fuse_pack == 1 || (c->opt_fuse_pack < 0 && B <= FUSE_PACK_MAX_BATCH);
    const bool patch1 = !(pe && atoi(pe) == 0);
    // (the depth-split attention has no fused fill: its packer is always mask_pack's depth-split form, whatever "fuse_pack" says)
    const bool fused = h3 && patch1 && fuse_env && !depth_split;
    c->packed_valid = !fused;
    c->last_in = in;
    c->packed_ld = run.impl == 0 ? 8 : 10;
    if (!fused) {
        ProfScope ps(c, run.stream, "mask_pack");
        HIP_TRY(c, launch_mask_pack(h3 ? 16 : (run.impl == 0 ? 8 : 10), d_img, d_flow, d_seg, c->label_fmt, d_tab, v, B, H, W, d_packed, sel, s,
                                    static_cast<const float*>(in.depth), d_tab_far, c->depth_thr));
    }
    const int c6 = v.cnv6_out;
    int rc;
    bool pose_fused = false;
    int pose_bm = 0, pose_mt = 0, pose_ntn = 0;
    c->cnv7_valid = true;
    if (h3) {
        if (patch1) { if ((rc = run_patch_layer(c, run, 0, false, d_packed, a[0], NB, fused, in))) return rc; }
        else if ((rc = run_conv_layer_h3(c, run, 0, d_packed, 8, H, W, a[0], 16, false, NB))) return rc;
        const char* p2e = tuning_env("DAVO_CNV2_PATCH");
        if (c->opt_patch_cnv2 && c->L[1].tile_h < 0 && !(p2e && atoi(p2e) == 0)) { if ((rc = run_patch_layer(c, run, 1, false, a[0], a[1], NB))) return rc; }
        else if ((rc = run_conv_layer_h3(c, run, 1, a[0], 16, c->H1, c->W1, a[1], 32, false, NB))) return rc;
        const char* p3e = tuning_env("DAVO_CNV3_PATCH");
        if (c->opt_patch_cnv3 && c->L[2].tile_h < 0 && !(p3e && atoi(p3e) == 0)) { if ((rc = run_patch_layer(c, run, 2, false, a[1], a[2], NB))) return rc; }
        else if ((rc = run_conv_layer_h3(c, run, 2, a[1], 32, c->H2, c->W2, a[2], 64, false, NB))) return rc;
        if ((rc = run_conv_layer_h3(c, run, 3, a[2], 64, c->H2, c->W2, a[3], 128, false, NB))) return rc;
        if ((rc = run_conv_layer_h3(c, run, 4, a[3], 128, c->H2, c->W2, a[4], 256, false, NB))) return rc;
        if (c->posenn_se) {
            if ((rc = run_posenn_se(c, run, true, a[4], NB))) return rc;
            if ((rc = run_conv_layer_h3(c, run, 5, d_se, 512, c->H2, c->W2, a[5], 2 * c6, false, NB))) return rc;
        } else if ((rc = run_conv_layer_h3(c, run, 5, a[4], 256, c->H2, c->W2, a[5], 2 * c6, false, NB))) return rc;
        pose_fused = c->opt_fuse_pose && c->H3 * c->W3 >= 128;
        if ((rc = run_conv_layer_h3(c, run, 6, a[5], 2 * c6, c->H2, c->W2, a[6], 512, true, NB, pose_fused, &pose_bm, &pose_mt, &pose_ntn,
                                    fold_pose ? static_cast<float*>(d_pose) : nullptr))) return rc;
        c->cnv7_valid = !pose_fused;
    } else if (run.impl == 0) {
        if (c->opt_patch_f32 && c->d_w1patch_f32 && c->packed_ld == 8) { if ((rc = run_patch_layer(c, run, 0, true, d_packed, a[0], NB))) return rc; }
        else if ((rc = run_conv_layer(c, run, 0, d_packed, 8, H, W, a[0], 16, NB))) return rc;
        if (c->opt_patch_f32 && c->d_w2patch_f32) { if ((rc = run_patch_layer(c, run, 1, true, a[0], a[1], NB))) return rc; }
        else if ((rc = run_conv_layer(c, run, 1, a[0], 16, c->H1, c->W1, a[1], 32, NB))) return rc;
        if (c->opt_patch_f32 && c->d_w3patch_f32) { if ((rc = run_patch_layer(c, run, 2, true, a[1], a[2], NB))) return rc; }
        else if ((rc = run_conv_layer(c, run, 2, a[1], 32, c->H2, c->W2, a[2], 64, NB))) return rc;
        if ((rc = run_conv_layer(c, run, 3, a[2], 64, c->H2, c->W2, a[3], 128, NB))) return rc;
        if ((rc = run_conv_layer(c, run, 4, a[3], 128, c->H2, c->W2, a[4], 256, NB))) return rc;
        if (c->posenn_se) {
            if ((rc = run_posenn_se(c, run, false, a[4], NB))) return rc;
            if ((rc = run_conv_layer(c, run, 5, d_se, 512, c->H2, c->W2, a[5], 2 * c6, NB))) return rc;
        } else if ((rc = run_conv_layer(c, run, 5, a[4], 256, c->H2, c->W2, a[5], 2 * c6, NB))) return rc;
        // float32 mode, round 4: the pose head in cnv7's epilogue like the f16x3 path's (the 109 MB activation is neither written nor
        // read back, pose_head_partial + pose_finish become pose_from_tiles); tiles of 128 rows must not span more than two images
        pose_fused = c->opt_fuse_pose && c->H3 * c->W3 >= 128 && c->L[6].npad == 256;
        pose_bm = 128; pose_ntn = 8;
        if ((rc = run_conv_layer(c, run, 6, a[5], 2 * c6, c->H2, c->W2, a[6], 512, NB, pose_fused, &pose_mt))) return rc;
        c->cnv7_valid = !pose_fused;
    } else {
        const std::string P = "pose_exp_net/";
        const int c10 = 2 * v.cin_per_frame;
        if (v.cin_per_frame != 5) return fail(c, DAVO_ERR_INVALID, "impl 1 supports the 10-channel (v1) input only");
        if ((rc = run_direct(c, run, "cnv1", d_packed, NB, H, W, c10, 10, 0, P + "cnv1/weights", P + "cnv1/biases", 7, 16, 2, 1, a[0], 16, 0))) return rc;
        if ((rc = run_direct(c, run, "cnv2", a[0], NB, c->H1, c->W1, 16, 16, 0, P + "cnv2/weights", P + "cnv2/biases", 5, 32, 2, 1, a[1], 32, 0))) return rc;
        if ((rc = run_direct(c, run, "cnv3", a[1], NB, c->H2, c->W2, 32, 32, 0, P + "cnv3/weights", P + "cnv3/biases", 3, 64, 1, 2, a[2], 64, 0))) return rc;
        if ((rc = run_direct(c, run, "cnv4", a[2], NB, c->H2, c->W2, 64, 64, 0, P + "cnv4/weights", P + "cnv4/biases", 3, 128, 1, 4, a[3], 128, 0))) return rc;
        if ((rc = run_direct(c, run, "cnv5", a[3], NB, c->H2, c->W2, 128, 128, 0, P + "cnv5/weights", P + "cnv5/biases", 3, 256, 1, 8, a[4], 256, 0))) return rc;
        if (c->posenn_se && (rc = run_posenn_se(c, run, false, a[4], NB))) return rc;      // float32 NHWC like the float32 mode's cnv5
        const char* heads[2] = {"rotation", "translation"};
        for (int h = 0; h < 2; ++h) {
            const std::string hp = P + "pose/" + heads[h] + "/";
            // feature attention: head h reads its half of the scaled tensor
            const float* x6 = c->posenn_se ? d_se : a[4];
            if ((rc = run_direct(c, run, "cnv6", x6, NB, c->H2, c->W2, 256, c->posenn_se ? 512 : 256, c->posenn_se ? h * 256 : 0, hp + "cnv6/weights", hp + "cnv6/biases", 3, c6, 1, 2, a[5], 2 * c6, h * c6))) return rc;
            if ((rc = run_direct(c, run, "cnv7", a[5], NB, c->H2, c->W2, c6, 2 * c6, h * c6, hp + "cnv7/weights", hp + "cnv7/biases", 3, 256, 2, 1, a[6], 512, h * 256))) return rc;
        }
    }
    bool snap_done = false;
    if (!(pose_fused && fold_pose)) {
        ProfScope ps(c, run.stream, "pose_head");
        if (pose_fused) {
            HIP_TRY(c, launch_pose_from_tiles(static_cast<const float*>(c->d_pose_tiles.get()) + (size_t)run.slot * c->pose_tiles_floats, NB, c->H3 * c->W3, pose_bm,
                                              pose_mt, pose_ntn, c->d_bpred.get(), static_cast<float*>(d_pose), h3 ? run.snap : SnapArgs{}, sel, s));
            snap_done = true;
        } else {
            HIP_TRY(c, launch_pose_head(a[6], NB, c->H3 * c->W3, c->d_wpred.get(), c->d_bpred.get(), ws.d_pose_partial.get(), static_cast<float*>(d_pose), sel, s));
        }
    }
    // the range guard's conditional copy of this batch's inputs (api.hip: tickets) rides in pose_from_tiles; other pose heads get a launch
    if (h3 && run.snap.record && !snap_done) HIP_TRY(c, launch_range_guard_snapshot(run.snap, s));
    c->last_B = B;
    c->last_pairs = sel;
    c->last_precision = h3 ? 1 : 0;
    if (res) *res = RunResult{h3, f32_fallback};
    return DAVO_OK;
}

}  // namespace davo

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
// a pair image to its (window, source frame), every layer in between takes the count.
// The three-frame PoseNN (davo_set_posenn_topology; nets/posenn.py:69-131) runs ONE image per window: mask_pack3 (16 channels) ->
// cnv1 (conv_patch_cnv1t_h3, or the implicit GEMM at cin = 16) -> cnv2..cnv7 as above on B images -> the two-pass pose head with six
// pred columns per head (cnv7 stored; the fused epilogue has three columns).
// The coupled network (davo_set_posenn_heads; nets/posenn.py:133-187) runs the pair network up to cnv5, then cnv6 as a one-group GEMM
// of N = cnv6_out, cnv7 as a one-group layer over all of cnv6's channels (256 per pixel) and one head of six columns: f16x3 fuses it
// into cnv7's epilogue like the flagship's (conv_igemm_h3.h, NC = 6; "fuse_pose", maps of at least 128 pixels), float32 and the small
// maps store cnv7 and run the two-pass head.  Host code only: kernels are reached through launch.h.
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

// ---- one conv layer: decided in plan.hip (decide_layer_f32 / decide_layer_h3), issued here ---------------------------------------
PlanOptions plan_options(const davo_ctx* c, int li) {
    PlanOptions o;
    o.wave128 = c->opt_wave128; o.skip_order = c->opt_skip_order; o.merge_order = c->opt_merge_order; o.pad_classes = c->opt_pad_classes;
    o.merge_rem_f32 = c->opt_merge_rem_f32; o.share_taps = c->opt_share_taps; o.merge_rem = c->opt_merge_rem; o.merge_cnv4 = c->opt_merge_cnv4;
    o.tile_208x128 = c->opt_tile_208x128; o.deep_ring = c->opt_deep_ring; o.split_k = c->opt_split_k; o.fold_fixup = c->opt_fold_fixup;
    o.f32_n16 = c->opt_f32_n16; o.f32_n256 = c->opt_f32_n256;
    o.ncu = c->ncu; o.dev_cus = c->dev_cus; o.cu_partition = c->cu_partition; o.user_stream = c->user_stream != nullptr; o.max_batch = c->max_batch;
    o.shift_in = li == 0 ? 0 : c->act_shift[li - 1]; o.shift_out = c->act_shift[li];
    return o;
}

// the profile entry of a step; a launcher's own refusal of a decided step is an internal error, never another kernel in silence
std::string step_label(const ConvLayer& L, bool rem) { return rem ? std::string(L.label) + ".rem" : std::string(L.label); }
int launched(davo_ctx* c, int li, int family, hipError_t e) {
    if (e == hipErrorNotSupported) return fail(c, DAVO_ERR_INVALID, "internal: layer %d was decided for the %s launcher, which refuses it", li, family_name(family));
    HIP_TRY(c, e);
    return DAVO_OK;
}

// FP32-MFMA path.  fuse_pose (cnv7): the pose head runs in the epilogue (conv_igemm.h); *pose_mt receives the layer's M tiles
int run_conv_layer(davo_ctx* c, const Run& run, int li, const float* x, int x_ld, int Hin, int Win, float* y, int y_ld, int NB, bool fuse_pose = false, int* pose_mt = nullptr) {
    const ConvLayer& L = c->L[li];
    const LayerDecision<ConvParams> d = decide_layer_f32(L, LayerCall{li, x_ld, Hin, Win, y_ld, true, NB, fuse_pose, false}, plan_options(c, li));
    if (d.err) return fail(c, d.err, "%s", d.msg);
    float* pose_partial = nullptr;
    if (d.pose_floats) { int rs = slot_scratch(c, run, &c->d_pose_tiles, &c->pose_tiles_floats, d.pose_floats, &pose_partial); if (rs) return rs; }
    if (fuse_pose && pose_mt) *pose_mt = d.pose_mt;
    c->last_plan[li][0] = d.plan_code[0]; c->last_plan[li][1] = d.plan_code[1]; c->last_split[li] = d.split;
    const ConvParams& g = d.steps[0].p[0];
    const PadTables* pc = nullptr;
    if (d.pad_classes) {
        int rc = DAVO_OK;
        pc = pad_tables_for(c, li, NB, g.Hout, g.Wout, Hin, Win, g.pad_t, g.pad_l, L.rate, &rc);
        if (rc) return rc;
    }
    for (int i = 0; i < d.nsteps; ++i) {
        const LaunchStep<ConvParams>& s = d.steps[i];
        ConvParams p[2] = {s.p[0], s.p[1]};
        for (int b = 0; b < s.nblocks; ++b) {
            const OrderRequest& r = s.ord[b];
            p[b].x = x; p[b].w = L.d_w.get(); p[b].bias = L.d_b.get(); p[b].y = y; p[b].zeros = c->d_zeros.get();
            if (fuse_pose) { p[b].pose_w = c->d_wpred.get(); p[b].pose_partial = pose_partial; }
            if (pc) {
                p[b].row_pixel = pc->row_pixel.get(); p[b].tile_taps = pc->tile_taps.get();
                p[b].tile_order = tile_order_pc(c, li, r.mtile0, r.mtiles, r.ntiles_n, g.M, g.Hout, g.Wout, *pc);
            } else if (r.kind == ORDER_LONG_FIRST)
                p[b].tile_order = tile_order_for(c, li, r.key, r.bm, r.mtile0, r.mtiles, r.ntiles_n, g.M, g.Hout, g.Wout, Hin, L.stride, g.pad_t, L.rate);
        }
        const dim3 grid(s.gx, s.gy);
        ProfScope ps(c, run.stream, step_label(L, s.rem_label).c_str());
        const hipError_t e = s.family == FAM_F32_N256      ? launch_layer_n256(li, p[0], grid, run.stream)
                             : s.family == FAM_F32_MAINREM ? launch_layer_mainrem(li, s.tile, p[0], p[1], s.n_main, s.n_rem, L.groups, run.stream)
                                                           : launch_layer(li, s.tile, p[0], grid, run.stream);
        { int rc = launched(c, li, s.family, e); if (rc) return rc; }
    }
    return DAVO_OK;
}

// f16x3 path: x and y are split-fp16 blocked tensors (y float32 when y_f32).  pose_out: the launch's last workgroup writes the poses
int run_conv_layer_h3(davo_ctx* c, const Run& run, int li, const void* x, int x_ch, int Hin, int Win, void* y, int y_ld,
                      bool y_f32, int NB, bool fuse_pose = false, int* pose_bm = nullptr, int* pose_mt = nullptr,
                      int* pose_ntn = nullptr, float* pose_out = nullptr) {
    const ConvLayer& L = c->L[li];
    const bool six = fuse_pose && coupled(c);       // the coupled head's six pred columns: the NC = 6 epilogue, pred as [2][256][3]
    const LayerDecision<ConvParamsH> d = decide_layer_h3(L, LayerCall{li, x_ch, Hin, Win, y_ld, y_f32, NB, fuse_pose, pose_out != nullptr, six}, plan_options(c, li));
    if (d.err) return fail(c, d.err, "%s", d.msg);
    // scratch before the launches that use it (growing it may synchronise every slot), the device probe before any profiling scope
    float *pose_partial = nullptr, *part = nullptr;
    if (d.pose_floats) { int rs = slot_scratch(c, run, &c->d_pose_tiles, &c->pose_tiles_floats, d.pose_floats, &pose_partial, d.pose_debug_bytes); if (rs) return rs; }
    if (d.splitk_floats) { int rs = slot_scratch(c, run, &c->d_splitk, &c->splitk_floats, d.splitk_floats, &part); if (rs) return rs; }
    if (d.fold_if_xcd && c->xcd_rr < 0) {
        int ok = 0;
        HIP_TRY(c, xcd_round_robin_probe(run.stream, &ok));
        c->xcd_rr = ok;
    }
    const bool fold = d.fold_if_xcd && c->xcd_rr > 0;
    if (fuse_pose) {
        if (pose_bm) *pose_bm = d.pose_bm;
        if (pose_mt) *pose_mt = d.pose_mt;
        if (pose_ntn) *pose_ntn = d.pose_ntn;
    }
    c->last_plan[li][0] = d.plan_code[0]; c->last_plan[li][1] = d.plan_code[1]; c->last_split[li] = d.split;
    uint8_t* const y8 = static_cast<uint8_t*>(y);
    unsigned* const range = run.range ? run.range + li : nullptr;
    for (int i = 0; i < d.nsteps; ++i) {
        const LaunchStep<ConvParamsH>& s = d.steps[i];
        ConvParamsH p[2] = {s.p[0], s.p[1]};
        for (int b = 0; b < s.nblocks; ++b) {
            const OrderRequest& r = s.ord[b];
            p[b].x = static_cast<const uint8_t*>(x); p[b].w = L.d_wh.get(); p[b].bias = L.d_bh.get(); p[b].y = y8;
            p[b].zeros = reinterpret_cast<const uint8_t*>(c->d_zeros.get());
            p[b].range = range;
            if (fuse_pose) { p[b].pose_w = six ? c->d_wpred_halves.get() : c->d_wpred.get(); p[b].pose_partial = pose_partial; }
            if (fuse_pose && pose_out) {      // pose_tail.h
                p[b].pose_counter = c->slots[run.slot].d_counters.get(); p[b].pose_bias = c->d_bpred.get(); p[b].pose_out = pose_out;
                p[b].pose_sel = run.pairs;
            }
            if (r.kind == ORDER_LONG_FIRST)
                p[b].tile_order = tile_order_for(c, li, r.key, r.bm, r.mtile0, r.mtiles, r.ntiles_n, p[b].M, p[b].Hout, p[b].Wout, Hin, L.stride, p[b].pad_t, L.rate);
        }
        const dim3 grid(s.gx, s.gy);
        hipError_t e = hipSuccess;
        ProfScope ps(c, run.stream, step_label(L, s.rem_label).c_str());       // split-K: the kernel and its fix-up together
        switch (s.family) {
            case FAM_H3: case FAM_H3S: e = launch_layer_h3(li, s.tile, p[0], grid, run.stream); break;
            case FAM_H3W: e = launch_layer_h3w(li, p[0], grid, run.stream); break;
            case FAM_H3W64: e = launch_layer_h3w64(li, p[0], run.stream); break;
            case FAM_H3W128: e = launch_layer_h3w128(p[0], run.stream); break;
            case FAM_H3_MAINREM:
                e = launch_layer_h3_mainrem(li, p[0], s.n_main, p[1], s.n_rem, s.order >= 0 ? s.order : (p[0].tile_order ? 2 : 0), run.stream);
                break;
            case FAM_H3_SPLITK:
                p[0].y = reinterpret_cast<uint8_t*>(part); p[0].range = nullptr;
                if (fold) {
                    p[0].sk_counter = c->slots[run.slot].d_counters.get() + d.sk_counter0;
                    p[0].sk_y = y8; p[0].sk_range = range; p[0].sk_parts = d.split; p[0].sk_relu = 1;
                }
                e = launch_layer_h3(li, s.tile, p[0], grid, run.stream);
                if (e == hipSuccess && !fold) e = launch_splitk_fixup(part, d.sk_M, d.sk_cout, d.split, 1, y8, range, run.stream);
                break;
            default: e = hipErrorNotSupported;
        }
        { int rc = launched(c, li, s.family, e); if (rc) return rc; }
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
            p.img = static_cast<const uint8_t*>(in.img); p.flow = in.flow;
            p.seg = in.seg; p.tab = c->slots[run.slot].d_tab.get(); p.v = c->v; p.sel = run.pairs;
        }
    }
    c->last_plan[li][0] = ((NB * p.Ho * p.Wo + 127) / 128) * 1000 + t.plan_id; c->last_plan[li][1] = 0; c->last_split[li] = 1;
    const int nblk = p.ntiles < t.per_cu * c->ncu ? p.ntiles : t.per_cu * c->ncu;
    ProfScope ps(c, run.stream, L.label);
    HIP_TRY(c, launch_patch_layer(li, f32, fused, p, nblk, run.stream, c->fmt));
    return DAVO_OK;
}

// cnv1 of the three-frame PoseNN from an LDS-staged patch (conv_patch_cnv1t_h3): x the 16-channel split-fp16 packed tensor
constexpr int PATCH_CNV1T_PLAN_ID = 96;
int run_patch_cnv1t(davo_ctx* c, const Run& run, const void* x, void* y, int NB) {
    const ConvLayer& L = c->L[0];
    ConvPatchParams p{};
    same_pad(c->H, L.KS, L.stride, L.rate, &p.Ho, &p.pad_t);
    same_pad(c->W, L.KS, L.stride, L.rate, &p.Wo, &p.pad_l);
    p.x = static_cast<const uint8_t*>(x); p.w = c->d_w1patch.get(); p.bias = L.d_bh.get(); p.y = static_cast<uint8_t*>(y);
    p.zeros = reinterpret_cast<const uint8_t*>(c->d_zeros.get());
    p.H = c->H; p.W = c->W;
    p.tiles_x = (p.Wo + cp1::TW - 1) / cp1::TW; p.tiles_y = (p.Ho + cp1::TH - 1) / cp1::TH;
    p.ntiles = NB * p.tiles_x * p.tiles_y;
    p.out_scale = ldexpf(1.0f / L.wscale, c->act_shift[0]);       // cnv1's input carries no storage scale
    p.bias_scale = L.wscale;
    p.range = run.range;                                          // word 0 of the record is cnv1's
    if (const char* e = tuning_env("DAVO_PDBG")) p.dbg = atoi(e);      // tuning build only
    c->last_plan[0][0] = ((NB * p.Ho * p.Wo + 127) / 128) * 1000 + PATCH_CNV1T_PLAN_ID; c->last_plan[0][1] = 0; c->last_split[0] = 1;
    const int nblk = p.ntiles < cp1t::PER_CU * c->ncu ? p.ntiles : cp1t::PER_CU * c->ncu;
    ProfScope ps(c, run.stream, L.label);
    HIP_TRY(c, launch_patch_cnv1t(p, nblk, run.stream));
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
    const bool tri = triplet(c);       // the three-frame PoseNN: one image per window, both poses from one pass
    const bool cpl = coupled(c);       // the coupled network: one cnv6, one cnv7 over all of it, one head of six pred columns
    if (cpl && (tri || c->posenn_se || c->L[5].groups != 1 || c->L[6].groups != 1 || c->L[6].cin != c->v.cnv6_out))
        return fail(c, DAVO_ERR_INVALID, "internal: the coupled PoseNN runs on the pair topology with one-group cnv6 and cnv7");
    if (tri && (sel != PAIRS_BOTH || run.impl != 0)) return fail(c, DAVO_ERR_INVALID, "internal: the three-frame PoseNN runs both pairs on the MFMA kernels (pairs %d, impl %d)", sel, run.impl);
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

    const int H = c->H, W = c->W, HW = H * W, NB = batch_images(c, B, sel);
    const Variant& v = c->v;
    const Slot& ws = c->slots[run.slot];
    float *const d_partial = ws.d_partial.get(), *const d_tab = ws.d_tab.get(), *const d_packed = ws.d_packed.get();
    float* const d_se = ws.se ? ws.se->d_se.get() : nullptr;                  // feature attention: cnv6's input (run_posenn_se fills it)
    unsigned* const d_counters = ws.d_counters.get();
    float* a[7];
    for (int i = 0; i < 7; ++i) a[i] = ws.d_act[i].get();
    hipStream_t s = run.stream;
    const uint8_t* const d_img = static_cast<const uint8_t*>(in.img);
    const void* const d_flow = in.flow;                        // float32 or binary16: c->fmt.flow
    const void* const d_seg = in.seg;                          // float32 or bytes: c->fmt.label
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
    const bool pooled = att_pooled(v.att_source);
    if (pooled) {
        // pooled flow attention (se_pool.h): the window sums of the context's pool plan, then the excitation as a launch of its own
        // ("fold_tails" does not apply to these sources)
        if (!ws.d_desc || !se_w1 || !se_b1 || !se_w2 || !se_b2) return fail(c, DAVO_ERR_INVALID, "internal: the pooled attention's descriptor buffer or dense tensors are missing");
        {
            ProfScope ps(c, run.stream, "se_pool_squeeze");
            HIP_TRY(c, launch_se_pool_squeeze(d_flow, c->fmt, B, H, W, v, c->pool, d_partial, sel, s));
        }
        ProfScope ps(c, run.stream, "se_pool_excite");
        HIP_TRY(c, launch_se_pool_excite(d_partial, B, v, c->pool, se_w1, se_b1, se_w2, se_b2, d_tab, ws.d_desc.get(), range_reset, sel, s));
    } else if (att_desc_depth(v.att_source)) {
        // depth sources: one float32 sum per depth plane and chunk, then (or, folded, in the same launch) the excitation
        ProfScope ps(c, run.stream, "se_depth_squeeze");
        HIP_TRY(c, launch_se_depth_squeeze(fold_excite, in.depth, c->fmt, B, HW, v, reinterpret_cast<unsigned*>(d_partial),
                                           d_counters + 1, se_w1, se_b1, se_w2, se_b2, d_tab, range_reset, sel, s));
    } else if (class_table) {
        // segmentation / rgb / seg+flow sources: per-frame histogram, byte or flow sums, then (or, folded, in the same launch) the
        // excitation
        ProfScope ps(c, run.stream, "se_class_squeeze");
        HIP_TRY(c, launch_se_class_squeeze(fold_excite, d_img, d_flow, d_seg, c->fmt, B, H, W, v, reinterpret_cast<unsigned*>(d_partial),
                                           d_counters + 1, se_w1, se_b1, se_w2, se_b2, d_tab, range_reset, sel, s));
    } else if (fold_excite && depth_split) {
        // the flagship's squeeze; the triplet's last workgroup evaluates the near tables and the far tables from the same sums
        ProfScope ps(c, run.stream, "se_squeeze_partial");
        const float* near_w[4] = {se_w1, se_b1, se_w2, se_b2};
        HIP_TRY(c, launch_se_squeeze_excite_split(d_flow, c->fmt, B, HW, v, d_partial, d_counters + 1, near_w, far_w, d_tab, d_tab_far, range_reset, sel, s));
    } else if (fold_excite) {
        // squeeze + excitation in one launch: the workgroup that delivers a triplet's last partial sum evaluates its tables
        ProfScope ps(c, run.stream, "se_squeeze_partial");
        HIP_TRY(c, launch_se_squeeze_excite(d_flow, c->fmt, B, HW, v, d_partial, d_counters + 1,
                                            se_w1, se_b1, se_w2, se_b2,
                                            wdev("pose_exp_net/pose_exp_net/seg_channel_weight/weight"), d_tab, range_reset, sel, s));
    } else if (att_flow_squeeze(v.att_source)) {
        ProfScope ps(c, run.stream, "se_squeeze_partial");
        HIP_TRY(c, launch_se_squeeze(d_flow, c->fmt, B, HW, v, d_partial, sel, s));
    }
    if (!fold_excite && !pooled) {
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
    const bool fused = h3 && patch1 && fuse_env && !depth_split && !tri;
    c->packed_valid = !fused;
    c->last_in = in;
    c->packed_ld = tri ? 16 : (run.impl == 0 ? 8 : 10);
    if (tri) {
        ProfScope ps(c, run.stream, "mask_pack");
        HIP_TRY(c, launch_mask_pack3(h3, d_img, d_flow, d_seg, c->fmt, d_tab, v, B, H, W, d_packed, s));
    } else if (!fused) {
        ProfScope ps(c, run.stream, "mask_pack");
        HIP_TRY(c, launch_mask_pack(h3 ? 16 : (run.impl == 0 ? 8 : 10), d_img, d_flow, d_seg, c->fmt, d_tab, v, B, H, W, d_packed, sel, s,
                                    in.depth, d_tab_far, c->depth_thr));
    }
    const int c6 = v.cnv6_out;
    const int ch6 = cpl ? c6 : 2 * c6, ch7 = cpl ? 256 : 512;      // channels per pixel of the stored cnv6 and cnv7
    int rc;
    bool pose_fused = false;
    int pose_bm = 0, pose_mt = 0, pose_ntn = 0;
    c->cnv7_valid = true;
    if (h3) {
        if (tri) {
            // cnv1 at 16 packed channels: the LDS-patch kernel ("patch_cnv1_t"), else the implicit GEMM at cin = 16
            if (c->opt_patch_cnv1_t && c->L[0].tile_h < 0) { if ((rc = run_patch_cnv1t(c, run, d_packed, a[0], NB))) return rc; }
            else if ((rc = run_conv_layer_h3(c, run, 0, d_packed, 16, H, W, a[0], 16, false, NB))) return rc;
        }
        else if (patch1) { if ((rc = run_patch_layer(c, run, 0, false, d_packed, a[0], NB, fused, in))) return rc; }
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
        } else if ((rc = run_conv_layer_h3(c, run, 5, a[4], 256, c->H2, c->W2, a[5], ch6, false, NB))) return rc;
        // the three-frame PoseNN stores cnv7 (the fused epilogue has three columns per head); the coupled one fuses its six columns (NC = 6)
        pose_fused = c->opt_fuse_pose && c->H3 * c->W3 >= 128 && !tri;
        if ((rc = run_conv_layer_h3(c, run, 6, a[5], ch6, c->H2, c->W2, a[6], ch7, true, NB, pose_fused, &pose_bm, &pose_mt, &pose_ntn,
                                    fold_pose ? static_cast<float*>(d_pose) : nullptr))) return rc;
        c->cnv7_valid = !pose_fused;
    } else if (run.impl == 0) {
        if (c->opt_patch_f32 && c->d_w1patch_f32 && c->packed_ld == 8) { if ((rc = run_patch_layer(c, run, 0, true, d_packed, a[0], NB))) return rc; }
        else if ((rc = run_conv_layer(c, run, 0, d_packed, tri ? 16 : 8, H, W, a[0], 16, NB))) return rc;      // the three-frame PoseNN: conv_igemm_f32 at cin = 16
        if (c->opt_patch_f32 && c->d_w2patch_f32) { if ((rc = run_patch_layer(c, run, 1, true, a[0], a[1], NB))) return rc; }
        else if ((rc = run_conv_layer(c, run, 1, a[0], 16, c->H1, c->W1, a[1], 32, NB))) return rc;
        if (c->opt_patch_f32 && c->d_w3patch_f32) { if ((rc = run_patch_layer(c, run, 2, true, a[1], a[2], NB))) return rc; }
        else if ((rc = run_conv_layer(c, run, 2, a[1], 32, c->H2, c->W2, a[2], 64, NB))) return rc;
        if ((rc = run_conv_layer(c, run, 3, a[2], 64, c->H2, c->W2, a[3], 128, NB))) return rc;
        if ((rc = run_conv_layer(c, run, 4, a[3], 128, c->H2, c->W2, a[4], 256, NB))) return rc;
        if (c->posenn_se) {
            if ((rc = run_posenn_se(c, run, false, a[4], NB))) return rc;
            if ((rc = run_conv_layer(c, run, 5, d_se, 512, c->H2, c->W2, a[5], 2 * c6, NB))) return rc;
        } else if ((rc = run_conv_layer(c, run, 5, a[4], 256, c->H2, c->W2, a[5], ch6, NB))) return rc;
        // float32 mode, round 4: the pose head in cnv7's epilogue like the f16x3 path's (the 109 MB activation is neither written nor
        // read back, pose_head_partial + pose_finish become pose_from_tiles); tiles of 128 rows must not span more than two images
        pose_fused = c->opt_fuse_pose && c->H3 * c->W3 >= 128 && c->L[6].npad == 256 && !tri && !cpl;
        pose_bm = 128; pose_ntn = 8;
        if ((rc = run_conv_layer(c, run, 6, a[5], ch6, c->H2, c->W2, a[6], ch7, NB, pose_fused, &pose_mt))) return rc;
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
        if (cpl) {      // the one head: cnv6 from all of cnv5, cnv7 from all of cnv6
            const std::string hp = P + "pose/";
            if ((rc = run_direct(c, run, "cnv6", a[4], NB, c->H2, c->W2, 256, 256, 0, hp + "cnv6/weights", hp + "cnv6/biases", 3, c6, 1, 2, a[5], c6, 0))) return rc;
            if ((rc = run_direct(c, run, "cnv7", a[5], NB, c->H2, c->W2, c6, c6, 0, hp + "cnv7/weights", hp + "cnv7/biases", 3, 256, 2, 1, a[6], 256, 0))) return rc;
        } else for (int h = 0; h < 2; ++h) {
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
        } else if (cpl) {
            HIP_TRY(c, launch_pose_head_coupled(a[6], NB, c->H3 * c->W3, c->d_wpred.get(), c->d_bpred.get(), ws.d_pose_partial.get(), static_cast<float*>(d_pose), sel, s));
        } else if (tri) {
            HIP_TRY(c, launch_pose_head6(a[6], B, c->H3 * c->W3, c->d_wpred.get(), c->d_bpred.get(), ws.d_pose_partial.get(), static_cast<float*>(d_pose), s));
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

// forward.hip — the forward of the pose path on one context, issued: forward_device validates, ensures the weights of the mode that
// runs, asks plan.hip's decide_forward for the launch sequence (a fixed-size record: front, packer, seven layer records, head) and
// walks it - run_front, run_layers, run_head, which only issue.  Nothing here chooses a kernel or knows the map or channel ladder.
// The sequence:
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

// ---- tile orders ------------------------------------------------------------------------------------
// One cache for every launch's table (davo_ctx::tile_orders): `build' is asked once per key for the order, an empty one meaning
// that no table is needed, and the table is uploaded.  A table that cannot be put on the device is not fatal: natural order.
template <class Build>
const int* cached_tile_order(davo_ctx* c, const std::vector<int>& key, Build build) {
    if (!c->opt.skip_order) return nullptr;
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
    static_cast<LaunchOptions&>(o) = c->opt;
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

// the tiles a fused cnv7 left its pose sums in: tile height, M tiles, N tiles (pose_from_tiles reads them back)
struct PoseTiles { int bm = 0, mt = 0, ntn = 0; };

// FP32-MFMA path.  call.fuse_pose (cnv7): the pose head runs in the epilogue (conv_igemm.h) on tiles of 128 rows x 8 N tiles; *tiles receives them
int run_conv_layer(davo_ctx* c, const Run& run, const LayerCall& call, const float* x, float* y, PoseTiles* tiles) {
    const int li = call.li, Hin = call.Hin, Win = call.Win, NB = call.NB;
    const bool fuse_pose = call.fuse_pose;
    const ConvLayer& L = c->L[li];
    const LayerDecision<ConvParams> d = decide_layer_f32(L, call, plan_options(c, li));
    if (d.err) return fail(c, d.err, "%s", d.msg);
    float* pose_partial = nullptr;
    if (d.pose_floats) { int rs = slot_scratch(c, run, &c->d_pose_tiles, &c->pose_tiles_floats, d.pose_floats, &pose_partial); if (rs) return rs; }
    if (fuse_pose) *tiles = PoseTiles{128, d.pose_mt, 8};
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
int run_conv_layer_h3(davo_ctx* c, const Run& run, const LayerCall& call, const void* x, void* y, PoseTiles* tiles, float* pose_out) {
    const int li = call.li, Hin = call.Hin;
    const bool fuse_pose = call.fuse_pose;
    const ConvLayer& L = c->L[li];
    const bool six = call.pose_six;                 // the coupled head's six pred columns: the NC = 6 epilogue, pred as [2][256][3]
    const LayerDecision<ConvParamsH> d = decide_layer_h3(L, call, plan_options(c, li));
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
    if (fuse_pose) *tiles = PoseTiles{d.pose_bm, d.pose_mt, d.pose_ntn};
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
// (x and y float32 NHWC).  RUN_PATCH_FUSED (f16x3 cnv1): the patch is built from the raw inputs (mask + pack fused in); otherwise it is
// copied from x, for cnv1 the packed tensor - for RUN_PATCH_CNV1T the three-frame PoseNN's 16-channel one (conv_patch_cnv1t_h3).
struct PatchLayer { int tw, th, per_cu; };       // output tile; workgroups per CU, each walks its tiles
constexpr PatchLayer PATCH_LAYERS[3] = {
    {cp1::TW, cp1::TH, 3},
    {cp2::TW, cp2::TH, 2},       // f16x3: 120 weight registers per lane; float32: three per CU measured 4 % slower
    {cp3::TW, cp3::TH, 3}};      // its padding, cp3::RATE on every side, is what SAME padding gives a 3x3 at dilation 2

int run_patch_layer(davo_ctx* c, const Run& run, int li, const LayerPlan& r, bool f32, const void* x, void* y, int NB, const Inputs& in) {
    const ConvLayer& L = c->L[li];
    const PatchLayer& t = PATCH_LAYERS[li];
    const bool fused = r.runner == RUN_PATCH_FUSED, cnv1t = r.runner == RUN_PATCH_CNV1T;
    const int per_cu = cnv1t ? cp1t::PER_CU : t.per_cu;
    const uint8_t* const w_h3[3] = {c->d_w1patch.get(), c->d_w2patch.get(), c->d_w3patch.get()};
    const float* const w_f32[3] = {c->d_w1patch_f32.get(), c->d_w2patch_f32.get(), c->d_w3patch_f32.get()};
    ConvPatchParams p{};
    same_pad(r.Hin, L.KS, L.stride, L.rate, &p.Ho, &p.pad_t);
    same_pad(r.Win, L.KS, L.stride, L.rate, &p.Wo, &p.pad_l);
    p.x = static_cast<const uint8_t*>(x); p.w = f32 ? reinterpret_cast<const uint8_t*>(w_f32[li]) : w_h3[li];
    p.bias = f32 ? L.d_b.get() : L.d_bh.get(); p.y = static_cast<uint8_t*>(y);
    p.zeros = reinterpret_cast<const uint8_t*>(c->d_zeros.get());
    p.H = r.Hin; p.W = r.Win;
    p.tiles_x = (p.Wo + t.tw - 1) / t.tw; p.tiles_y = (p.Ho + t.th - 1) / t.th;
    p.ntiles = NB * p.tiles_x * p.tiles_y;
    if (!f32) {      // stored activations carry 2^act_shift (exact); cnv1's input carries none
        const int sin = li == 0 ? 0 : c->act_shift[li - 1];
        p.out_scale = ldexpf(1.0f / L.wscale, c->act_shift[li] - sin);
        p.bias_scale = ldexpf(L.wscale, sin);
        p.range = run.range ? run.range + li : nullptr;
        if (const char* e = tuning_env("DAVO_PDBG")) p.dbg = atoi(e);      // tuning build only
        if (li == 0 && !cnv1t) {
            p.img = static_cast<const uint8_t*>(in.img); p.flow = in.flow;
            p.seg = in.seg; p.tab = c->slots[run.slot].d_tab.get(); p.v = c->v; p.sel = run.pairs;
        }
    }
    c->last_plan[li][0] = r.plan_code; c->last_plan[li][1] = 0; c->last_split[li] = 1;
    const int nblk = p.ntiles < per_cu * c->ncu ? p.ntiles : per_cu * c->ncu;
    ProfScope ps(c, run.stream, L.label);
    HIP_TRY(c, launch_patch_layer(li, f32, fused, cnv1t, p, nblk, run.stream, c->fmt));
    return DAVO_OK;
}

// impl 1, group g of layer li: the direct convolution on the raw HWIO weights of the reference's scopes
int run_direct(davo_ctx* c, const Run& run, int li, const LayerPlan& r, int g, const float* x, float* y, int NB) {
    static const char* const heads[2] = {"rotation/", "translation/"};
    const ConvLayer& L = c->L[li];
    const std::string scope = li < 5 ? std::string("pose_exp_net/") : std::string("pose_exp_net/pose/") + (coupled(c) ? "" : heads[g]);
    const std::string wname = scope + L.label + "/weights", bname = scope + L.label + "/biases";
    int Ho, Wo, pt, pl;
    same_pad(r.Hin, L.KS, L.stride, L.rate, &Ho, &pt);
    same_pad(r.Win, L.KS, L.stride, L.rate, &Wo, &pl);
    for (const std::string* n : {&wname, &bname}) {            // impl 1 is the only reader of the raw device copies: made on demand
        HostTensor& t = c->weights.at(*n);
        if (!t.dev) { int rc = upload(c, t.data, &t.dev); if (rc) return rc; }
    }
    ProfScope ps(c, run.stream, L.label);
    HIP_TRY(c, launch_conv_direct(x, NB, r.Hin, r.Win, r.cin, r.x_ch, r.x_coff[g], c->weights.at(wname).dev.get(), L.KS, r.cout,
                                  c->weights.at(bname).dev.get(), L.stride, L.rate, pt, pl, Ho, Wo, 1, y, r.y_ld, r.y_coff[g], run.stream));
    return DAVO_OK;
}

// feature attention (posenn_se.h): cnv5 (x, in the mode's storage, P pixels per image) -> the slot's d_se = [x s_r | x s_r s_t], 512 channels of cnv5's geometry
int run_posenn_se(davo_ctx* c, const Run& run, bool h3, const void* x, int NB, int P) {
    SeDense w[2];
    for (int h = 0; h < 2; ++h) {
        const std::string scope = std::string("pose_exp_net/pose/") + (h ? "translation" : "rotation") + "/cnv5_se_attention/";
        const float** const slot[4] = {&w[h].w1, &w[h].b1, &w[h].w2, &w[h].b2};
        const char* const parts[4] = {"bottleneck_fc/kernel", "bottleneck_fc/bias", "recover_fc/kernel", "recover_fc/bias"};
        for (int k = 0; k < 4; ++k) {
            const auto it = c->weights.find(scope + parts[k]);
            if (it == c->weights.end() || !it->second.dev) return fail(c, DAVO_ERR_NOT_READY, "feature-attention weights not loaded");
            *slot[k] = it->second.dev.get();
        }
    }
    if (!c->slots[run.slot].se) return fail(c, DAVO_ERR_INVALID, "internal: no feature-attention workspace");
    const SeWorkspace& ws = *c->slots[run.slot].se;
    {
        ProfScope ps(c, run.stream, "se5_squeeze");
        HIP_TRY(c, launch_se5_squeeze(h3, x, NB, P, ws.d_se_partial.get(), run.stream));
    }
    {
        ProfScope ps(c, run.stream, "se5_excite");
        HIP_TRY(c, launch_se5_excite(ws.d_se_partial.get(), NB, P, h3 ? ldexpf(1.0f, -c->act_shift[4]) : 1.0f, w[0], w[1], ws.d_se_scale.get(), run.stream));
    }
    ProfScope ps(c, run.stream, "se5_scale");
    HIP_TRY(c, launch_se5_scale(h3, x, ws.d_se_scale.get(), NB, P, ws.d_se.get(), (h3 && run.range) ? run.range + RANGE_SE : nullptr, run.stream));
    return DAVO_OK;
}

// ---- the forward: decided in plan.hip (decide_forward), issued here -----------------------------------------------------------------
// the weights of the mode that really runs, on the device: -> MODE_*; f16x3 falls back to float32 on the weight-spread guard
int ensure_weights(davo_ctx* c, const Run& run, int* mode, bool* f32_fallback) {
    if (!c->pred_ready) { int rc = build_pred_weights(c); if (rc) return rc; }
    bool h3 = run.impl == 0 && run.precision == 1;
    *f32_fallback = false;
    if (h3 && !c->packed_h_ready) { int rc = build_packed_weights_h3(c); if (rc) return rc; }
    if (h3 && c->weight_channel_spread_log2 > MAX_WEIGHT_CHANNEL_SPREAD_LOG2) {
        // a consumer's per-input-channel weight norms span more than 2^14: per-layer storage scales cannot keep every channel's fp16
        // pair float32-grade (weights.hip).  The reference's float32 graph has no such limit (nets/posenn.py:205-215): float32 kernels.
        if (!c->opt_auto_range)
            return fail(c, DAVO_ERR_RANGE, "`%s': per-input-channel weight norms span 2^%d (> 2^%d): the f16x3 storage cannot hold every channel "
                        "float32-grade - davo_set_precision(ctx, 0), or leave \"auto_range\" on", c->weight_channel_spread_layer.c_str(),
                        c->weight_channel_spread_log2, MAX_WEIGHT_CHANNEL_SPREAD_LOG2);
        h3 = false;
        *f32_fallback = true;                // counted once per API call by the caller (api.hip)
        char note[256];
        snprintf(note, sizeof note, "float32 kernels: per-input-channel weight norms of `%s' span 2^%d (> 2^%d)",
                 c->weight_channel_spread_layer.c_str(), c->weight_channel_spread_log2, MAX_WEIGHT_CHANNEL_SPREAD_LOG2);
        c->range_report = note;
    }
    if (!h3 && run.impl == 0 && !c->packed_ready) { int rc = build_packed_weights(c); if (rc) return rc; }      // float32 kernels: packed at their first use
    *mode = h3 ? MODE_H3 : run.impl == 0 ? MODE_F32 : MODE_DIRECT;
    return DAVO_OK;
}

// the context's settings and the batch's wishes decide_forward reads; the tuning build's environment is read here
ForwardOptions forward_options(const davo_ctx* c, const Run& run) {
    auto env = [](const char* name) { const char* e = tuning_env(name); return e ? atoi(e) : -1; };
    ForwardOptions o;
    static_cast<LaunchOptions&>(o) = c->opt;
    for (int i = 0; i < 7; ++i) o.forced_tile[i] = c->L[i].tile_h >= 0;
    o.have_patch_f32[0] = (bool)c->d_w1patch_f32; o.have_patch_f32[1] = (bool)c->d_w2patch_f32; o.have_patch_f32[2] = (bool)c->d_w3patch_f32;
    o.npad7 = c->L[6].npad;
    o.zero_record = run.zero_record; o.want_snapshot = run.snap.record != nullptr;
    o.env_fuse_pack = env("DAVO_FUSE_PACK"); o.env_patch[0] = env("DAVO_CNV1_PATCH"); o.env_patch[1] = env("DAVO_CNV2_PATCH"); o.env_patch[2] = env("DAVO_CNV3_PATCH");
    return o;
}

// the attention front and the packer: squeeze, excitation(s), mask + pack
int run_front(davo_ctx* c, const Run& run, const ForwardPlan& p, int B, const Inputs& in) {
    const Slot& ws = c->slots[run.slot];
    const Variant& v = c->v;
    const int H = c->H, W = c->W, HW = H * W, sel = run.pairs, kind = p.front.kind;
    const bool fold = p.front.fold_excite;
    hipStream_t s = run.stream;
    float *const d_partial = ws.d_partial.get(), *const d_tab = ws.d_tab.get(), *const d_tab_far = ws.d_tab_far.get();
    unsigned* const d_counters = ws.d_counters.get() + 1;      // [1 + b]: triplet b's squeeze ticket
    const uint8_t* const d_img = static_cast<const uint8_t*>(in.img);
    auto wdev = [&](const char* n) -> const float* {
        auto it = c->weights.find(n);
        return it == c->weights.end() ? nullptr : it->second.dev.get();
    };
    const int a = v.att_source;
    const SeDense w{wdev(se_weight_name(a, 0)), wdev(se_weight_name(a, 1)), wdev(se_weight_name(a, 2)), wdev(se_weight_name(a, 3))};
    SeDense far;
    if (kind == FRONT_FLOW_SPLIT) {
        far = SeDense{wdev(se_far_weight_name(0)), wdev(se_far_weight_name(1)), wdev(se_far_weight_name(2)), wdev(se_far_weight_name(3))};
        if (!d_tab_far || !w || !far) return fail(c, DAVO_ERR_INVALID, "internal: the depth-split attention's tables or dense tensors are missing");
    }
    if (kind == FRONT_POOLED && (!ws.d_desc || !w)) return fail(c, DAVO_ERR_INVALID, "internal: the pooled attention's descriptor buffer or dense tensors are missing");
    const float* const wstatic = (kind == FRONT_FLOW || p.front.excite) ? wdev("pose_exp_net/pose_exp_net/seg_channel_weight/weight") : nullptr;
    auto reset = [&](int label) -> unsigned* { return p.front.reset_at == label ? run.range : nullptr; };      // the launch that zeroes the record's per-batch word
    if (p.front.squeeze) {
        const int label = p.launch[0];
        ProfScope ps(c, s, forward_label(label));
        if (kind == FRONT_POOLED)             // the window sums of the context's pool plan (se_pool.h)
            HIP_TRY(c, launch_se_pool_squeeze(in.flow, c->fmt, B, H, W, v, c->pool, d_partial, sel, s));
        else if (kind == FRONT_DEPTH)         // one float32 sum per depth plane and chunk
            HIP_TRY(c, launch_se_depth_squeeze(fold, in.depth, c->fmt, B, HW, v, reinterpret_cast<unsigned*>(d_partial), d_counters, w, d_tab, reset(label), sel, s));
        else if (kind == FRONT_CLASS)         // segmentation / rgb / seg+flow sources: per-frame histogram, byte or flow sums
            HIP_TRY(c, launch_se_class_squeeze(fold, d_img, in.flow, in.seg, c->fmt, B, H, W, v, reinterpret_cast<unsigned*>(d_partial), d_counters, w, d_tab, reset(label), sel, s));
        else if (fold && kind == FRONT_FLOW_SPLIT)      // the triplet's last workgroup evaluates the near and the far tables from the same sums
            HIP_TRY(c, launch_se_squeeze_excite_split(in.flow, c->fmt, B, HW, v, d_partial, d_counters, w, far, d_tab, d_tab_far, reset(label), sel, s));
        else if (fold)                        // the workgroup that delivers a triplet's last partial sum evaluates its tables
            HIP_TRY(c, launch_se_squeeze_excite(in.flow, c->fmt, B, HW, v, d_partial, d_counters, w, wstatic, d_tab, reset(label), sel, s));
        else
            HIP_TRY(c, launch_se_squeeze(in.flow, c->fmt, B, HW, v, d_partial, sel, s));
    }
    if (kind == FRONT_POOLED) {
        ProfScope ps(c, s, "se_pool_excite");
        HIP_TRY(c, launch_se_pool_excite(d_partial, B, v, c->pool, w, d_tab, ws.d_desc.get(), reset(LB_SE_POOL_EXCITE), sel, s));
    }
    if (p.front.excite) {
        ProfScope ps(c, s, "se_excite");
        HIP_TRY(c, launch_se_excite(d_partial, B, HW, v, w, wstatic, d_tab, reset(LB_SE_EXCITE), sel, s));
    }
    if (p.front.excite_far) {                 // the same launch again on the far MLP, reading the same partial sums
        ProfScope ps(c, s, "se_excite_far");
        HIP_TRY(c, launch_se_excite(d_partial, B, HW, v, far, nullptr, d_tab_far, nullptr, sel, s));
    }
    if (p.pack.kind == PACK_NONE) return DAVO_OK;
    ProfScope ps(c, s, "mask_pack");
    if (p.pack.kind == PACK_TRIPLET) HIP_TRY(c, launch_mask_pack3(p.mode == MODE_H3, d_img, in.flow, in.seg, c->fmt, d_tab, v, B, H, W, ws.d_packed.get(), s));
    else HIP_TRY(c, launch_mask_pack(p.pack.ld, d_img, in.flow, in.seg, c->fmt, d_tab, v, B, H, W, ws.d_packed.get(), sel, s, in.depth, d_tab_far, c->depth_thr));
    return DAVO_OK;
}

// cnv1..cnv7, each on the runner its record names; impl 1 walks cnv6 and cnv7 once per head
int run_layers(davo_ctx* c, const Run& run, const ForwardPlan& p, const Inputs& in, float* d_pose, PoseTiles* tiles) {
    const Slot& ws = c->slots[run.slot];
    const bool h3 = p.mode == MODE_H3;
    auto buffer = [&](int b) -> float* { return b == BUF_PACKED ? ws.d_packed.get() : b == BUF_SE ? (ws.se ? ws.se->d_se.get() : nullptr) : ws.d_act[b].get(); };
    auto run_layer = [&](int li, int g) {
        const LayerPlan& r = p.layer[li];
        const float* const x = buffer(r.x_buf);
        float* const y = ws.d_act[li].get();
        switch (r.runner) {
            case RUN_IGEMM_H3: return run_conv_layer_h3(c, run, layer_call(p, li), x, y, tiles, r.pose_tail ? d_pose : nullptr);
            case RUN_IGEMM_F32: return run_conv_layer(c, run, layer_call(p, li), x, y, tiles);
            case RUN_DIRECT: return run_direct(c, run, li, r, g, x, y, p.NB);
            default: return run_patch_layer(c, run, li, r, !h3, x, y, p.NB, in);
        }
    };
    int rc;
    for (int li = 0; li < 5; ++li)
        if ((rc = run_layer(li, 0))) return rc;
    if (p.se5 && (rc = run_posenn_se(c, run, h3, ws.d_act[4].get(), p.NB, p.layer[4].Hout * p.layer[4].Wout))) return rc;
    for (int g = 0; g < p.layer[5].ngroups; ++g)
        for (int li = 5; li < 7; ++li)
            if ((rc = run_layer(li, g))) return rc;
    return DAVO_OK;
}

// the poses, unless cnv7's launch wrote them, and the range guard's snapshot where no pose_from_tiles carries it
int run_head(davo_ctx* c, const Run& run, const ForwardPlan& p, const PoseTiles& t, float* d_pose) {
    const Slot& ws = c->slots[run.slot];
    const int P = p.layer[6].Hout * p.layer[6].Wout;
    if (p.head.kind != HEAD_TAIL) {
        ProfScope ps(c, run.stream, "pose_head");
        if (p.head.kind == HEAD_TILES)
            HIP_TRY(c, launch_pose_from_tiles(static_cast<const float*>(c->d_pose_tiles.get()) + (size_t)run.slot * c->pose_tiles_floats, p.NB, P, t.bm, t.mt, t.ntn,
                                              c->d_bpred.get(), d_pose, p.mode == MODE_H3 ? run.snap : SnapArgs{}, run.pairs, run.stream));
        else
            HIP_TRY(c, launch_pose_head(p.head.cols, p.head.heads, ws.d_act[6].get(), p.NB, P, c->d_wpred.get(), c->d_bpred.get(), ws.d_pose_partial.get(), d_pose,
                                        run.pairs, run.stream));
    }
    if (p.head.snapshot_launch) HIP_TRY(c, launch_range_guard_snapshot(run.snap, run.stream));      // api.hip: tickets
    return DAVO_OK;
}

}  // namespace

// validate, ensure weights, decide, issue
int forward_device(davo_ctx* c, const Run& run, int B, const Inputs& in, void* d_pose, RunResult* res) {
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
    int mode = MODE_H3, rc;
    bool f32_fallback = false;
    if ((rc = ensure_weights(c, run, &mode, &f32_fallback))) return rc;
    const ForwardCall call{c->H, c->W, B, run.pairs, mode, c->v, triplet(c), coupled(c), c->posenn_se, c->L[5].groups, c->L[6].groups, c->L[6].cin};
    const ForwardPlan p = decide_forward(call, forward_options(c, run));
    if (p.err) return fail(c, p.err, "%s", p.msg);
    c->packed_valid = p.pack.packed_valid;
    c->last_in = in;
    c->packed_ld = p.pack.packed_ld;
    c->cnv7_valid = true;
    PoseTiles tiles;
    if ((rc = run_front(c, run, p, B, in))) return rc;
    if ((rc = run_layers(c, run, p, in, static_cast<float*>(d_pose), &tiles))) return rc;
    c->cnv7_valid = p.head.cnv7_valid;
    if ((rc = run_head(c, run, p, tiles, static_cast<float*>(d_pose)))) return rc;
    c->last_B = B;
    c->last_pairs = run.pairs;
    c->last_precision = mode == MODE_H3 ? 1 : 0;
    if (res) *res = RunResult{mode == MODE_H3, f32_fallback};
    return DAVO_OK;
}

}  // namespace davo

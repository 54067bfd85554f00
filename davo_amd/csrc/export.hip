// export.hip — what davo_forward_features / davo_forward_heat deliver beside the poses (include/davo_hip.h): the feature and the
// heat export, their workspaces (davo_set_feature_export, davo_set_heat_export) and the two entry points, which are davo_forward
// (entry.hip: forward_entry) with the exports wanted.  The kernels are feature_export.h's, reached through launch.h.
#include <algorithm>
#include <cmath>

#include "ctx.h"
#include "launch.h"

using namespace davo;

// ---- feature export: davo_set_feature_export / davo_forward_features ----------------------------------------------
// What DAVO.inference(sess, mode='feature') fetches beside the poses (davo.py:1553-1569; generate_feature_map.py:183-260 is its
// reader): everything is computed from what a forward leaves on the device - the class tables (d_tab), the staged inputs and cnv6
// in the storage form the forward ran in - by the two kernels of feature_export.h, into one workspace block of the context, and
// copied to the caller's arrays piece by piece.  The block holds fx_cap windows of every export tensor: the largest sub-batch
// davo_forward issues under the host_chunk of the moment the export was switched on; a larger run of windows (a re-issued batch,
// a host_chunk raised since) goes out in pieces of fx_cap.  With the export off nothing here is allocated or launched.
namespace {

struct FxLayout { size_t rot, trans, masked, image, attention, att_19, total; };      // float offsets into d_fx for `cap' windows
FxLayout fx_layout(const davo_ctx* c, int cap) {
    const size_t HW = (size_t)c->H * c->W, n = (size_t)cap, c6 = (size_t)c->v.cnv6_out;
    FxLayout l{};
    l.rot = 0;
    l.trans = l.rot + n * HW * c6;
    l.masked = l.trans + n * HW * c6;
    l.image = l.masked + n * HW * 9;
    l.attention = l.image + n * HW * 9;
    l.att_19 = l.attention + n * HW * 3;              // last: the only section that is no multiple of 16 bytes
    l.total = l.att_19 + n * 3 * NCLS;
    return l;
}

bool fx_wanted(const davo_feature_out* o) {
    return o && (o->att_19 || o->attention || o->masked_image || o->image || o->feat_rot || o->feat_trans);
}

// Windows [w0, w0 + nw) of the last forward - `in' are that forward's device inputs, window 0 - go to windows
// [b0, b0 + nw) of the caller's arrays of B windows.  Reads d_tab, the inputs and d_act[5] as that forward left them, in the
// precision it ran (last_precision) and under the storage scale it stored cnv6 with.  Returns with the copies done.
int export_features(davo_ctx* c, const Inputs& in, int w0, int nw, int b0, int B, const davo_feature_out& out) {
    if (!c->fx || c->fx->cap < 1) return fail(c, DAVO_ERR_INVALID, "internal: no feature export workspace");
    float* const d_fx = c->fx->d.get();
    const int fx_cap = c->fx->cap;
    if (c->last_pairs != PAIRS_BOTH || w0 < 0 || w0 + nw > c->last_B) return fail(c, DAVO_ERR_INVALID, "internal: feature export of windows the last forward did not run");
    const size_t HW = (size_t)c->H * c->W, c6 = (size_t)c->v.cnv6_out;
    const bool h3 = c->last_precision == 1;
    const FxLayout l = fx_layout(c, fx_cap);
    const Slot& ws = last_workspace(c);
    hipStream_t s = last_stream(c);
    for (int p0 = 0; p0 < nw; p0 += fx_cap) {
        const int np = std::min(fx_cap, nw - p0);
        const Inputs win = from_window(c, in, w0 + p0);
        float* const w_att19 = out.att_19 ? d_fx + l.att_19 : nullptr;
        float* const w_att = out.attention ? d_fx + l.attention : nullptr;
        float* const w_masked = out.masked_image ? d_fx + l.masked : nullptr;
        float* const w_image = out.image ? d_fx + l.image : nullptr;
        float* const w_rot = out.feat_rot ? d_fx + l.rot : nullptr;
        float* const w_trans = out.feat_trans ? d_fx + l.trans : nullptr;
        if (w_att19 || w_att || w_masked || w_image) {
            ProfScope ps(c, s, "feature_maps");
            HIP_TRY(c, launch_feature_maps(static_cast<const uint8_t*>(win.img), win.seg, c->fmt,
                                           ws.d_tab.get() + (size_t)(w0 + p0) * 3 * NCLS, c->v, np, c->H, c->W, w_att19, w_att, w_masked, w_image, s,
                                           win.depth, ws.d_tab_far ? ws.d_tab_far.get() + (size_t)(w0 + p0) * 3 * NCLS : nullptr, c->depth_thr));
        }
        if (w_rot || w_trans) {
            ProfScope ps(c, s, "feature_resize_cnv6");
            HIP_TRY(c, launch_feature_resize_cnv6(h3, ws.d_act[5].get(), w0 + p0, np, c->H2, c->W2, (int)c6, h3 ? ldexpf(1.0f, -c->act_shift[5]) : 1.0f,
                                                  w_rot, w_trans, s));
        }
        // the caller's per-frame arrays are [3][B][...], the workspace's [3][np][...]: one copy per frame
        const size_t first = (size_t)(b0 + p0);
        auto frames = [&](float* host, const float* dev, size_t per_window) -> int {
            if (!host) return DAVO_OK;
            for (int f = 0; f < 3; ++f)
                HIP_TRY(c, hipMemcpyAsync(host + ((size_t)f * B + first) * per_window, dev + (size_t)f * np * per_window,
                                          (size_t)np * per_window * sizeof(float), hipMemcpyDeviceToHost, s));
            return DAVO_OK;
        };
        { int rc = frames(out.att_19, w_att19, NCLS); if (rc) return rc; }
        { int rc = frames(out.attention, w_att, HW); if (rc) return rc; }
        { int rc = frames(out.masked_image, w_masked, HW * 3); if (rc) return rc; }
        { int rc = frames(out.image, w_image, HW * 3); if (rc) return rc; }
        if (w_rot) HIP_TRY(c, hipMemcpyAsync(out.feat_rot + first * HW * c6, w_rot, (size_t)np * HW * c6 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (w_trans) HIP_TRY(c, hipMemcpyAsync(out.feat_trans + first * HW * c6, w_trans, (size_t)np * HW * c6 * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));              // the next piece reuses the workspace
    }
    return DAVO_OK;
}

// ---- heat export: davo_set_heat_export / davo_forward_heat ------------------------------------------------------
// What generate_feature_map.py:204-265 keeps of the two feature maps: per head and window the channel sum of the resized cnv6 and
// the block's maximum, reduced where cnv6 lies (feature_export.h: feature_heat_cnv6, feature_resize_plane) into a block of the
// context's own - 2 (H/4 W/4 + H W + 1) floats per window - and copied out piece by piece like the full export.
struct HeatLayout { size_t plane, sum, max, total; };      // float offsets into the block for `cap' windows; head h at + h * cap * per-window
HeatLayout heat_layout(const davo_ctx* c, int cap) {
    const size_t HW = (size_t)c->H * c->W, HW2 = (size_t)c->H2 * c->W2, n = (size_t)cap;
    HeatLayout l{};
    l.plane = 0;                                       // first: written as float4, H W is a multiple of 16
    l.sum = l.plane + 2 * n * HW;
    l.max = l.sum + 2 * n * HW2;
    l.total = l.max + 2 * n;
    return l;
}

bool heat_wanted(const davo_heat_out* o) { return o && (o->rot_sum || o->trans_sum || o->rot_max || o->trans_max); }

// export_features' contract for the heat members: windows [w0, w0 + nw) of the last forward -> windows [b0, b0 + nw) of the caller's
int export_heat(davo_ctx* c, int w0, int nw, int b0, const davo_heat_out& out) {
    if (!c->heat || c->heat->cap < 1) return fail(c, DAVO_ERR_INVALID, "internal: no heat export workspace");
    float* const d = c->heat->d.get();
    const int cap = c->heat->cap;
    if (c->last_pairs != PAIRS_BOTH || w0 < 0 || w0 + nw > c->last_B) return fail(c, DAVO_ERR_INVALID, "internal: heat export of windows the last forward did not run");
    const size_t HW = (size_t)c->H * c->W, HW2 = (size_t)c->H2 * c->W2;
    const bool h3 = c->last_precision == 1;
    const HeatLayout l = heat_layout(c, cap);
    const Slot& ws = last_workspace(c);
    hipStream_t s = last_stream(c);
    const bool rot = out.rot_sum || out.rot_max, trans = out.trans_sum || out.trans_max;
    for (int p0 = 0; p0 < nw; p0 += cap) {
        const int np = std::min(cap, nw - p0);
        float* const w_plane[2] = {out.rot_sum ? d + l.plane : nullptr, out.trans_sum ? d + l.plane + (size_t)cap * HW : nullptr};
        float* const w_sum[2] = {rot ? d + l.sum : nullptr, trans ? d + l.sum + (size_t)cap * HW2 : nullptr};
        float* const w_max[2] = {rot ? d + l.max : nullptr, trans ? d + l.max + cap : nullptr};
        {
            ProfScope ps(c, s, "feature_heat_cnv6");
            HIP_TRY(c, launch_feature_heat(h3, ws.d_act[5].get(), w0 + p0, np, c->H2, c->W2, c->v.cnv6_out, h3 ? ldexpf(1.0f, -c->act_shift[5]) : 1.0f,
                                           w_sum[0], w_sum[1], w_max[0], w_max[1], w_plane[0], w_plane[1], s));
        }
        c->heat->last_np = np;
        const size_t first = (size_t)(b0 + p0);
        if (out.rot_sum) HIP_TRY(c, hipMemcpyAsync(out.rot_sum + first * HW, w_plane[0], (size_t)np * HW * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.trans_sum) HIP_TRY(c, hipMemcpyAsync(out.trans_sum + first * HW, w_plane[1], (size_t)np * HW * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.rot_max) HIP_TRY(c, hipMemcpyAsync(out.rot_max + first, w_max[0], (size_t)np * sizeof(float), hipMemcpyDeviceToHost, s));
        if (out.trans_max) HIP_TRY(c, hipMemcpyAsync(out.trans_max + first, w_max[1], (size_t)np * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));              // the next piece reuses the workspace
    }
    return DAVO_OK;
}

// The depth-split flow attention applies two tables per frame, chosen per pixel: there is no 19-row table an `att_19' member could
// hold (the reference sets no att_19s for the branch either, davo.py:1470).  Refused before anything runs; the context stays usable.
int refuse_att_19(davo_ctx* c, const char* fn, const davo_feature_out* out) {
    if (c->v.att_source != ATT_DEPTH_SPLIT || !out || !out->att_19) return DAVO_OK;
    return fail(c, DAVO_ERR_INVALID, "%s: `att_19' does not exist for the depth-split flow attention (att_source %d): every source pixel takes its "
                "weight from the near or the far table by its depth, no single 19-row table was applied - pass att_19 = NULL", fn, ATT_DEPTH_SPLIT);
}

// windows an export workspace is built for: the largest sub-batch davo_forward issues under the host_chunk of the moment
int export_cap(const davo_ctx* c) { return c->host_chunk > 0 ? std::min(c->max_batch, 2 * c->host_chunk - 1) : c->max_batch; }

}  // namespace

int davo::export_all(davo_ctx* c, const Exports& ex, const Inputs& in, int w0, int nw, int b0, int B) {
    if (ex.fx) { int rc = export_features(c, in, w0, nw, b0, B, *ex.fx); if (rc) return rc; }
    if (ex.heat) { int rc = export_heat(c, w0, nw, b0, *ex.heat); if (rc) return rc; }
    return DAVO_OK;
}

extern "C" {

int davo_set_feature_export(davo_ctx* c, int on) {
    if (!c) return DAVO_ERR_INVALID;
    { int rc = refuse_while_tracking(c, "davo_set_feature_export"); if (rc) return rc; }      // exports under tracking are not built
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = sync_all_slots(c); if (rc) return rc; }
    if (!on) { c->fx.reset(); c->fx_on = false; return DAVO_OK; }
    if (triplet(c)) return fail(c, DAVO_ERR_INVALID, "the feature export has no three-frame PoseNN form yet (davo_set_posenn_topology): its maps and cnv6 windows are per pair image");
    if (coupled(c)) return fail(c, DAVO_ERR_INVALID, "the feature export has no coupled PoseNN form yet (davo_set_posenn_heads): its feature maps are one cnv6 per head");
    if (!c->fx) {
        FxBlock fx;
        fx.cap = export_cap(c);
        HIP_TRY(c, dev_alloc(&fx.d, fx_layout(c, fx.cap).total));
        c->fx = std::move(fx);
    }
    c->fx_on = true;
    return DAVO_OK;
}

int davo_forward_features(davo_ctx* c, int B, const uint8_t* img, const float* flow, const float* seg, const float* depth, float* pose_out,
                          const davo_feature_out* out) {
    if (!c) return DAVO_ERR_INVALID;
    if (!c->fx_on) return fail(c, DAVO_ERR_NOT_READY, "davo_forward_features: the feature export is off - call davo_set_feature_export(ctx, 1) first");
    if (c->pairs != PAIRS_BOTH)
        return fail(c, DAVO_ERR_INVALID, "davo_forward_features runs both pairs of every window, the reference's semantics (davo.py:1456-1457): "
                    "davo_set_pairs(ctx, DAVO_PAIRS_BOTH) first (the selection is %d)", c->pairs);
    { int rc = refuse_att_19(c, "davo_forward_features", out); if (rc) return rc; }
    return forward_entry(c, B, window_batch("davo_forward", false, true, img, flow, seg, depth), pose_out, Exports{fx_wanted(out) ? out : nullptr, nullptr});
}

int davo_set_heat_export(davo_ctx* c, int on) {
    if (!c) return DAVO_ERR_INVALID;
    { int rc = refuse_while_tracking(c, "davo_set_heat_export"); if (rc) return rc; }      // exports under tracking are not built
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = sync_all_slots(c); if (rc) return rc; }
    if (!on) { c->heat.reset(); return DAVO_OK; }
    if (triplet(c)) return fail(c, DAVO_ERR_INVALID, "the heat export has no three-frame PoseNN form yet (davo_set_posenn_topology): its cnv6 windows are per pair image");
    if (coupled(c)) return fail(c, DAVO_ERR_INVALID, "the heat export has no coupled PoseNN form yet (davo_set_posenn_heads): its heat maps are one cnv6 per head");
    if (!c->heat) {
        HeatBlock h;
        h.cap = export_cap(c);
        HIP_TRY(c, dev_alloc(&h.d, heat_layout(c, h.cap).total));
        c->heat = std::move(h);
    }
    return DAVO_OK;
}

int davo_forward_heat(davo_ctx* c, int B, const uint8_t* img, const float* flow, const float* seg, const float* depth, float* pose_out,
                      const davo_feature_out* out, const davo_heat_out* heat) {
    if (!c) return DAVO_ERR_INVALID;
    const bool want_fx = fx_wanted(out), want_heat = heat_wanted(heat);
    if (want_fx && !c->fx_on) return fail(c, DAVO_ERR_NOT_READY, "davo_forward_heat: a member of `out' is wanted and the feature export is off - call davo_set_feature_export(ctx, 1) first");
    if (want_heat && !c->heat) return fail(c, DAVO_ERR_NOT_READY, "davo_forward_heat: a member of `heat' is wanted and the heat export is off - call davo_set_heat_export(ctx, 1) first");
    if (c->pairs != PAIRS_BOTH)
        return fail(c, DAVO_ERR_INVALID, "davo_forward_heat runs both pairs of every window, the reference's semantics (davo.py:1456-1457): "
                    "davo_set_pairs(ctx, DAVO_PAIRS_BOTH) first (the selection is %d)", c->pairs);
    { int rc = refuse_att_19(c, "davo_forward_heat", out); if (rc) return rc; }
    return forward_entry(c, B, window_batch("davo_forward", false, true, img, flow, seg, depth), pose_out, Exports{want_fx ? out : nullptr, want_heat ? heat : nullptr});
}

}  // extern "C"

// hooks.hip — the measurement and test hooks of libdavo_hip.so (include/davo_hip.h): page-locked and device memory for the
// callers' buffers, the profile calls, what the last forward planned, the planner's and the padding classes' host logic, one
// tensor of the last forward (davo_debug_read) and one convolution through the kernels (davo_conv2d_same).  No forward calls these.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ctx.h"
#include "launch.h"
#include "pad_classes.h"
#include "plan.h"

using namespace davo;

// the seven layers as a context of these settings holds them (api.hip: davo_create and the davo_set_posenn_* calls, "force_tile")
static void hook_layers(ConvLayer (&L)[7], int cnv6_out, bool posenn_se, bool tri, bool cpl, int force_tile) {
    init_posenn_layers(L, cnv6_out);
    if (tri) init_layer(L[0], "cnv1", 7, 2, 1, 16, 16, 1);
    if (posenn_se) init_layer(L[5], "cnv6", 3, 1, 2, 256, cnv6_out, 2);          // davo_set_posenn_se: one group per head
    if (cpl) init_coupled_head(L, cnv6_out);
    for (ConvLayer& l : L) l.tile_h = forced_tile_h(force_tile, l.cout);
}

// davo_decide_layer's options are the option table's first rows (options.h) and twelve values that are no options, davo_decide_forward's
// the rows behind those and three more: a row added to the table without the header's counts does not compile
constexpr int LAYER_ROWS = DAVO_DECIDE_OPTIONS - 12, FORWARD_ROWS = DAVO_FORWARD_OPTIONS - 3;
static_assert(NUM_OPTIONS == LAYER_ROWS + FORWARD_ROWS, "options.h: OPTION_TABLE and include/davo_hip.h: DAVO_DECIDE_OPTIONS, DAVO_FORWARD_OPTIONS");

extern "C" {

int davo_host_alloc(int device, size_t bytes, void** out) {
    if (!out || bytes == 0) return DAVO_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return DAVO_ERR_HIP;
    return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? DAVO_OK : DAVO_ERR_HIP;
}
int davo_host_free(void* p) { return hipHostFree(p) == hipSuccess ? DAVO_OK : DAVO_ERR_HIP; }
int davo_host_register(int device, void* p, size_t bytes) {
    if (!p || bytes == 0) return DAVO_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return DAVO_ERR_HIP;
    return hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess ? DAVO_OK : DAVO_ERR_HIP;
}
int davo_host_unregister(void* p) { return hipHostUnregister(p) == hipSuccess ? DAVO_OK : DAVO_ERR_HIP; }

int davo_device_malloc(davo_ctx* c, size_t bytes, void** out) {
    if (!c || !out) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMalloc(out, bytes));
    return DAVO_OK;
}
int davo_device_free(davo_ctx* c, void* p) {
    if (!c) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipFree(p));
    return DAVO_OK;
}
int davo_memcpy_h2d(davo_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, last_stream(c)));
    HIP_TRY(c, hipStreamSynchronize(last_stream(c)));
    return DAVO_OK;
}
int davo_memcpy_d2h(davo_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, last_stream(c)));
    HIP_TRY(c, hipStreamSynchronize(last_stream(c)));
    return DAVO_OK;
}

int davo_profile_enable(davo_ctx* c, int on) {
    if (!c) return DAVO_ERR_INVALID;
    if (!on && c->prof) { int rc = prof_collect(c); if (rc) return rc; }
    c->prof = on != 0;
    c->prof_dominant_only = on == 2;
    return DAVO_OK;
}
int davo_profile_reset(davo_ctx* c) {
    if (!c) return DAVO_ERR_INVALID;
    int rc = prof_collect(c);
    if (rc) return rc;
    for (auto& pe : c->prof_entries) { pe.launches = 0; pe.total_ms = 0.0; pe.dur_ms.clear(); pe.period_ms.clear(); }
    return DAVO_OK;
}
int davo_profile_samples(davo_ctx* c, const char* name, int which, float* out, int cap) {
    if (!c || !name || which < 0 || which > 1 || cap < 0 || (cap > 0 && !out)) return DAVO_ERR_INVALID;
    int rc = prof_collect(c);
    if (rc) return rc;
    for (const auto& pe : c->prof_entries)
        if (pe.name == name) {
            const std::vector<float>& v = which == 0 ? pe.dur_ms : pe.period_ms;
            const int n = (int)std::min(v.size(), (size_t)cap);
            for (int i = 0; i < n; ++i) out[i] = v[i];
            return (int)v.size();
        }
    return 0;
}
int davo_profile_entry(davo_ctx* c, int i, char* name, int name_len, int* launches, double* total_ms) {
    if (!c) return DAVO_ERR_INVALID;
    int rc = prof_collect(c);
    if (rc) return rc;
    if (i < 0 || i >= (int)c->prof_entries.size()) return DAVO_ERR_INVALID;
    const ProfEntry& pe = c->prof_entries[i];
    if (name && name_len > 0) { strncpy(name, pe.name.c_str(), name_len - 1); name[name_len - 1] = 0; }
    if (launches) *launches = pe.launches;
    if (total_ms) *total_ms = pe.total_ms;
    return DAVO_OK;
}

int davo_last_plan(davo_ctx* c, int layer, int launch, int* mtiles, int* bn) {
    if (!c || layer < 0 || layer > 6 || launch < 0 || launch > 1) return DAVO_ERR_INVALID;
    const int v = c->last_plan[layer][launch];
    if (mtiles) *mtiles = v / 1000;
    if (bn) *bn = v % 1000;
    return DAVO_OK;
}

int davo_last_split(davo_ctx* c, int layer, int* parts) {
    if (!c || layer < 0 || layer > 6) return DAVO_ERR_INVALID;
    if (parts) *parts = c->last_split[layer];
    return DAVO_OK;
}

int davo_debug_read(davo_ctx* c, const char* tensor, float* host_out, size_t n_floats) {
    if (!c || !tensor || !host_out) return DAVO_ERR_INVALID;
    if (c->last_B < 1) return fail(c, DAVO_ERR_NOT_READY, "no forward has run yet");
    const size_t NB = (size_t)batch_images(c, c->last_B, c->last_pairs);      // pair images of the last forward (three-frame PoseNN: one image per window)
    const float* src = nullptr;
    size_t n = 0;
    const std::string t = tensor;
    const Slot& ws = last_workspace(c);
    if (t == "att_table") { src = ws.d_tab.get(); n = (size_t)c->last_B * 3 * NCLS; }       // att_source 13: the near MLP's tables
    else if (t == "att_table_far") {                         // ... and the far MLP's; the target's rows are ones in both
        if (!ws.d_tab_far) return fail(c, DAVO_ERR_INVALID, "`att_table_far' exists for the depth-split flow attention only (att_source %d, got %d)", ATT_DEPTH_SPLIT, c->v.att_source);
        src = ws.d_tab_far.get(); n = (size_t)c->last_B * 3 * NCLS;
    }
    else if (t == "se_desc") {                               // pooled flow attention (se_pool.h): the SE descriptors [B][2][D] of the source frames
        if (!ws.d_desc) return fail(c, DAVO_ERR_INVALID, "`se_desc' exists for the pooled flow-attention variants only (att_source %d..%d, got %d)", ATT_POOL_GP2X2, ATT_POOL_SPP864, c->v.att_source);
        src = ws.d_desc.get(); n = (size_t)c->last_B * 2 * att_se_in(c->v.att_source);
    }
    else if (t == "cnv5_se_scale" || t == "cnv5_se") {      // feature attention (posenn_se.h): [2B][2][256] s_r | s_r s_t; [2B][H2][W2][512] rotation | translation input of cnv6
        if (!c->posenn_se || !ws.se) return fail(c, DAVO_ERR_NOT_READY, "`%s' exists in the feature-attention variant only (davo_set_posenn_se)", tensor);
        if (t == "cnv5_se") { src = ws.se->d_se.get(); n = NB * c->H2 * c->W2 * 512; }
        else { src = ws.se->d_se_scale.get(); n = NB * 2 * 256; }
    }
    else if (t == "packed") {
        if (!c->packed_valid) {          // fused path: materialise the packed tensor on demand from the last inputs
            HIP_TRY(c, launch_mask_pack(16, static_cast<const uint8_t*>(c->last_in.img), c->last_in.flow, c->last_in.seg,
                                        c->fmt, ws.d_tab.get(), c->v, c->last_B, c->H, c->W, ws.d_packed.get(), c->last_pairs, last_stream(c),
                                        nullptr, nullptr, 0.f));      // (the depth-split variant never takes the fused path)
            c->packed_valid = true;
        }
        src = ws.d_packed.get(); n = NB * c->H * c->W * c->packed_ld;
    }
    else {
        const char* names[7] = {"cnv1", "cnv2", "cnv3", "cnv4", "cnv5", "cnv6", "cnv7"};
        for (int i = 0; i < 7; ++i)
            if (t == names[i]) { src = ws.d_act[i].get(); n = NB * c->act_floats_per_img[i]; }
    }
    if (t == "heat_sum") {            // the heat export's channel sums of the piece it exported last: [2][np][H2][W2], rotation | translation
        if (!c->heat || c->heat->last_np < 1) return fail(c, DAVO_ERR_NOT_READY, "`heat_sum' exists after a davo_forward_heat with the heat export on");
        const size_t per = (size_t)c->H2 * c->W2, np = (size_t)c->heat->last_np;
        if (n_floats != 2 * np * per) return fail(c, DAVO_ERR_INVALID, "`heat_sum' holds %zu floats, caller asked for %zu", 2 * np * per, n_floats);
        const size_t at = (size_t)2 * c->heat->cap * c->H * c->W;
        for (int h = 0; h < 2; ++h) {
            int rc = davo_memcpy_d2h(c, host_out + h * np * per, c->heat->d.get() + at + (size_t)h * c->heat->cap * per, np * per * sizeof(float));
            if (rc) return rc;
        }
        return DAVO_OK;
    }
    if (t == "pose_tiles") {          // the fused pose head's per-tile partial sums of the last batch (slot 0's region)
        if (c->cnv7_valid || !c->d_pose_tiles.get()) return fail(c, DAVO_ERR_NOT_READY, "the pose head did not run fused");
#ifndef DAVO_POSE_DEBUG
        if (n_floats > c->pose_tiles_floats) return fail(c, DAVO_ERR_INVALID, "pose_tiles holds %zu floats", c->pose_tiles_floats);
#endif
        return davo_memcpy_d2h(c, host_out, c->d_pose_tiles.get(), n_floats * sizeof(float));
    }
    if (t == "cnv7" && !c->cnv7_valid)
        return fail(c, DAVO_ERR_NOT_READY, "cnv7 was not materialised: the pose head ran fused (davo_set_option(ctx, \"fuse_pose\", 0))");
    if (!src) return fail(c, DAVO_ERR_INVALID, "unknown tensor `%s'", tensor);
    if (n != n_floats) return fail(c, DAVO_ERR_INVALID, "`%s' holds %zu floats, caller asked for %zu", tensor, n, n_floats);
    int rc = davo_memcpy_d2h(c, host_out, src, n * sizeof(float));
    if (rc) return rc;
    const bool split = c->last_precision == 1 && t != "att_table" && t != "att_table_far" && t != "se_desc" && t != "cnv7" && t != "cnv5_se_scale";
    if (split) {       // split-fp16 blocked -> plain float32 NHWC
        int ch = triplet(c) ? 16 : 8;                // "packed"
        const char* names[6] = {"cnv1", "cnv2", "cnv3", "cnv4", "cnv5", "cnv6"};
        for (int i = 0; i < 6; ++i) if (t == names[i]) ch = c->act_ch[i];
        if (t == "cnv5_se") ch = 512;                // cnv5's storage ...
        const int cb = ch < 32 ? ch : 32;
        int shift = t == "cnv5_se" ? c->act_shift[4] : 0;       // ... and its scale
        for (int i = 0; i < 6; ++i) if (t == names[i]) shift = c->act_shift[i];
        std::vector<float> tmp(ch);
        const size_t npix = n / ch;
        for (size_t px = 0; px < npix; ++px) {
            const _Float16* raw = reinterpret_cast<const _Float16*>(host_out + px * ch);
            for (int k = 0; k < ch; ++k) {
                const _Float16* blk = raw + (size_t)(k / cb) * cb * 2;
                tmp[k] = ldexpf((float)blk[k % cb] + (float)blk[cb + k % cb], -shift);
            }
            memcpy(host_out + px * ch, tmp.data(), ch * sizeof(float));
        }
    }
    return DAVO_OK;
}

int davo_tile_filter_rows(int m0, int m1, int Hout, int Wout, int Hin, int stride, int pad_t, int rate,
                          int* ky0, int* nky, int nblocks, int* chunk_map) {
    if (!ky0 || !nky || Hout < 1 || Wout < 1 || Hin < 1 || stride < 1 || rate < 1 || m0 < 0 || nblocks < 0) return DAVO_ERR_INVALID;
    const FilterRows fr = valid_filter_rows(m0, m1, Hout, Wout, Hin, stride, pad_t, rate);
    *ky0 = fr.ky0;
    *nky = fr.nky;
    if (chunk_map)
        for (int v = 0; v < 3 * fr.nky * nblocks; ++v) chunk_map[v] = h3_real_chunk(v, fr.ky0, fr.nky);
    return DAVO_OK;
}

int davo_pad_class_tables(int NB, int Hout, int Wout, int Hin, int Win, int pad_t, int pad_l, int rate, int* row_pixel, unsigned short* tile_taps) {
    if (!row_pixel || !tile_taps || NB < 1 || Hout < 1 || Wout < 1 || Hin < 1 || Win < 1 || rate < 1 || (long)NB * Hout * Wout > 0x7fffff00L) return DAVO_ERR_INVALID;
    std::vector<int32_t> rows;
    std::vector<uint16_t> taps;
    const bool sorted = pad_class_tables(NB, Hout, Wout, Hin, Win, pad_t, pad_l, rate, BM, &rows, &taps);
    memcpy(row_pixel, rows.data(), rows.size() * sizeof(int32_t));
    memcpy(tile_taps, taps.data(), taps.size() * sizeof(uint16_t));
    return sorted ? 1 : 0;
}

int davo_pad_class_tile_order(const unsigned short* tile_taps, int mtile0, int mtiles, int ntiles_n, int* order) {
    if (!tile_taps || !order || mtile0 < 0 || mtiles < 1 || ntiles_n < 1) return DAVO_ERR_INVALID;
    std::vector<int> o;
    pad_class_tile_order(tile_taps, mtile0, mtiles, ntiles_n, &o);
    memcpy(order, o.data(), o.size() * sizeof(int));
    return DAVO_OK;
}

int davo_plan_layer_f32(int mtiles, int npad, int groups, int ncu, int* mtile0, int* launch_mtiles, int* tile_bn) {
    if (mtiles < 1 || npad < 32 || npad % 32 || groups < 1 || ncu < 1 || !mtile0 || !launch_mtiles || !tile_bn) return DAVO_ERR_INVALID;
    const std::vector<Launch> plan = plan_layer(mtiles, npad, groups, ncu);
    if (plan.empty() || plan.size() > 2) return DAVO_ERR_INVALID;
    for (size_t i = 0; i < plan.size(); ++i) { mtile0[i] = plan[i].mtile0; launch_mtiles[i] = plan[i].mtiles; tile_bn[i] = plan[i].BN; }
    return (int)plan.size();
}

int davo_plan_layer(int M, int npad, int groups, int* rows, int* tile_bm, int* tile_bn) {
    if (M < 1 || npad < 32 || npad % 32 || groups < 1 || !rows || !tile_bm || !tile_bn) return DAVO_ERR_INVALID;
    const std::vector<LaunchH> plan = plan_layer_h3(M, npad, groups, -1, npad == 256);
    if (plan.empty() || plan.size() > 2) return DAVO_ERR_INVALID;
    for (size_t i = 0; i < plan.size(); ++i) {
        const TileShape ts = tile_shape(plan[i].tile);
        rows[i] = plan[i].rows; tile_bm[i] = ts.bm; tile_bn[i] = ts.bn;
    }
    return (int)plan.size();
}

int davo_decide_layer(int precision, int layer, int H, int W, int NB, int cnv6_out, int fuse_pose, const int* options, int n_options,
                      int* out, int out_cap) {
    if (precision < 0 || precision > 1 || layer < 0 || layer > 6 || H < 1 || W < 1 || NB < 1 || cnv6_out < 1 || !out || (n_options > 0 && !options) ||
        n_options < 0 || n_options > DAVO_DECIDE_OPTIONS)
        return DAVO_ERR_INVALID;
    PlanOptions o;
    int cu_partition = 0, user_stream = 0, force_tile = -1, pose_tail = 0, posenn_se = 0, tri = 0, cpl = 0;
    int* const tail[DAVO_DECIDE_OPTIONS - LAYER_ROWS] = {&o.ncu, &o.dev_cus, &cu_partition, &user_stream, &o.max_batch, &o.shift_in, &o.shift_out,
                                                         &force_tile, &pose_tail, &posenn_se, &tri, &cpl};
    for (int i = 0; i < n_options; ++i) *(i < LAYER_ROWS ? &(o.*OPTION_TABLE[i].field) : tail[i - LAYER_ROWS]) = options[i];
    o.cu_partition = cu_partition != 0; o.user_stream = user_stream != 0;
    if (o.ncu < 1 || o.dev_cus < 1 || o.max_batch < 1 || force_tile < -1 || force_tile >= NUM_TILES) return DAVO_ERR_INVALID;
    // the layer's input and output as decide_forward lays a forward of NB images out (one pair, or the three-frame PoseNN's NB windows)
    ConvLayer L[7];
    hook_layers(L, cnv6_out, posenn_se != 0, tri != 0, cpl != 0, force_tile);
    Variant v{};
    v.cin_per_frame = 5; v.cnv6_out = cnv6_out;
    const ForwardPlan fp = decide_forward(ForwardCall{H, W, NB, tri ? PAIRS_BOTH : PAIRS_SRC1, precision == 1 ? MODE_H3 : MODE_F32, v, tri != 0, cpl != 0, posenn_se,
                                                      L[5].groups, L[6].groups, L[6].cin}, ForwardOptions{});
    if (fp.err) return fp.err;
    LayerCall call = layer_call(fp, layer);
    call.fuse_pose = fuse_pose != 0; call.pose_tail = pose_tail != 0; call.pose_six = fuse_pose && cpl && precision == 1;
    int n = 0;
    auto put = [&](long v) { if (n < out_cap) out[n] = (int)v; ++n; };
    // m_end: one past the step's last output row; deep, family_ok: f16x3 only (the family's own predicate on the step's own block)
    auto record = [&](const auto& d, auto m_end, auto deep, auto family_ok) {
        if (d.err) return d.err;
        put(d.nsteps);
        for (int i = 0; i < d.nsteps; ++i) {
            const auto& s = d.steps[i];
            const auto &p = s.p[0], &r = s.p[s.nblocks - 1];
            for (long v : {(long)s.family, (long)s.tile, (long)s.row0, (long)m_end(s), (long)p.mtile0, (long)p.ntiles_n, (long)s.gx, (long)s.gy,
                           (long)s.n_main, (long)s.n_rem, (long)s.order, (long)deep(s), (long)s.rem_label, (long)(s.nblocks > 1 ? r.mtile0 : 0),
                           (long)(s.nblocks > 1 ? r.ntiles_n : 0), (long)s.ord[0].kind, (long)family_ok(s), (long)p.nchunks})
                put(v);
        }
        for (long v : {(long)d.plan_code[0], (long)d.plan_code[1], (long)d.split, (long)d.fold_if_xcd, (long)d.pad_classes, (long)d.pose_bm, (long)d.pose_mt,
                       (long)d.pose_ntn, (long)d.pose_floats, (long)d.splitk_floats, (long)L[layer].nchunks_h, (long)L[layer].cpb})
            put(v);
        return n;
    };
    if (precision == 0) {
        typedef LaunchStep<ConvParams> S;
        return record(decide_layer_f32(L[layer], call, o), [](const S& s) { return s.m_end; }, [](const S&) { return 0; }, [](const S&) { return 1; });
    }
    typedef LaunchStep<ConvParamsH> S;
    return record(decide_layer_h3(L[layer], call, o), [](const S& s) { return s.p[s.nblocks - 1].M; }, [](const S& s) { return s.p[0].deep; },
                  [&](const S& s) {
                      const ConvParamsH& p = s.p[0];
                      return s.family == FAM_H3W          ? layer_h3w_supported(layer, p)
                             : s.family == FAM_H3W64      ? layer_h3w64_supported(layer, p)
                             : s.family == FAM_H3W128     ? layer_h3w128_supported(p)
                             : s.family == FAM_H3_MAINREM ? layer_h3_mainrem_supported(layer, p, s.n_main, s.n_rem)
                             : s.family == FAM_H3S        ? is_208(s.tile)
                                                          : !is_208(s.tile);
                  });
}

int davo_decide_forward(const int* call, const int* options, int n_options, int* out, int out_cap) {
    if (!call || !out || (n_options > 0 && !options) || n_options < 0 || n_options > DAVO_FORWARD_OPTIONS) return DAVO_ERR_INVALID;
    const int H = call[0], W = call[1], B = call[2], mode = call[4], cnv6_out = call[6], topology = call[8], heads = call[9], posenn_se = call[10];
    if (H < 1 || W < 1 || B < 1 || mode < MODE_H3 || mode > MODE_DIRECT || call[5] < 0 || call[5] > ATT_MAX || cnv6_out < 1 ||
        (topology != DAVO_POSENN_PAIRS && topology != DAVO_POSENN_TRIPLET) || (heads != DAVO_POSENN_HEADS_DECOUPLED && heads != DAVO_POSENN_HEADS_COUPLED))
        return DAVO_ERR_INVALID;
    ForwardOptions o;
    int force_tile = -1, zero_record = 0, want_snapshot = 0;
    int* const tail[DAVO_FORWARD_OPTIONS - FORWARD_ROWS] = {&force_tile, &zero_record, &want_snapshot};
    for (int i = 0; i < n_options; ++i) *(i < FORWARD_ROWS ? &(o.*OPTION_TABLE[LAYER_ROWS + i].field) : tail[i - FORWARD_ROWS]) = options[i];
    if (force_tile < -1 || force_tile >= NUM_TILES) return DAVO_ERR_INVALID;
    o.zero_record = zero_record != 0; o.want_snapshot = want_snapshot != 0;
    const bool tri = topology == DAVO_POSENN_TRIPLET, cpl = heads == DAVO_POSENN_HEADS_COUPLED;
    ConvLayer L[7];
    hook_layers(L, cnv6_out, posenn_se != 0 && !cpl, tri, cpl, force_tile);
    for (int i = 0; i < 7; ++i) o.forced_tile[i] = L[i].tile_h >= 0;
    o.have_patch_f32[0] = !tri;                                // weights.hip: the three-frame cnv1 has no float32 patch weights
    o.npad7 = L[6].npad;
    Variant v{};
    v.att_source = call[5]; v.cnv6_out = cnv6_out; v.cin_per_frame = call[7];
    const ForwardPlan p = decide_forward(ForwardCall{H, W, B, call[3], mode, v, tri, cpl, posenn_se, L[5].groups, L[6].groups, L[6].cin}, o);
    if (p.err) return p.err;
    int n = 0;
    auto put = [&](int x) { if (n < out_cap) out[n] = x; ++n; };
    for (int x : {p.NB, p.front.kind, (int)p.front.squeeze, (int)p.front.fold_excite, (int)p.front.excite, (int)p.front.excite_far, p.front.reset_at, p.pack.kind,
                  p.pack.ld, p.pack.packed_ld, (int)p.pack.packed_valid, (int)p.se5, p.head.kind, p.head.cols, p.head.heads, (int)p.head.snapshot_launch,
                  (int)p.head.cnv7_valid})
        put(x);
    for (const LayerPlan& r : p.layer)
        for (int x : {r.runner, r.label, r.x_buf, r.x_ch, r.Hin, r.Win, r.y_ld, r.Hout, r.Wout, (int)r.y_f32, (int)r.fuse_pose, (int)r.pose_tail, (int)r.pose_six,
                      r.plan_code, r.ngroups, r.cin, r.cout, r.x_coff[0], r.x_coff[1], r.y_coff[0], r.y_coff[1]})
            put(x);
    put(p.nlaunch);
    for (int i = 0; i < p.nlaunch; ++i) put(p.launch[i]);
    return n;
}

int davo_conv2d_same(int device, const float* x, int N, int H, int W, int Cin, const float* w, int k, int Cout,
                     const float* bias, int stride, int rate, int relu, int precision, float* y, char* err, int err_len) {
    auto bad = [&](const char* m, int code) {
        if (err && err_len > 0) { strncpy(err, m, err_len - 1); err[err_len - 1] = 0; }
        return code;
    };
    const int cl = ilog2_exact(Cin);
    if (!x || !w || !bias || !y) return bad("null pointer", DAVO_ERR_INVALID);
    if (cl < 2) return bad("Cin must be a power of two >= 4", DAVO_ERR_INVALID);
    if (precision == 1 && cl < 3) return bad("f16x3 needs Cin >= 8", DAVO_ERR_INVALID);
    if (!(k == 1 || k == 3 || k == 5 || k == 7) || !(stride == 1 || stride == 2) || rate < 1)
        return bad("k in {1,3,5,7}, stride in {1,2}, rate >= 1", DAVO_ERR_INVALID);
    if (hipSetDevice(device) != hipSuccess) return bad("hipSetDevice failed", DAVO_ERR_HIP);
    ConvLayer L;
    init_layer(L, "conv", k, stride, rate, Cin, Cout, 1);
    int Ho, Wo, pt, pl;
    same_pad(H, k, stride, rate, &Ho, &pt);
    same_pad(W, k, stride, rate, &Wo, &pl);
    const size_t nx = (size_t)N * H * W * Cin, ny = (size_t)N * Ho * Wo * Cout;
    std::vector<float> bp(precision == 1 ? L.npad_h : L.npad, 0.f);
    memcpy(bp.data(), bias, Cout * sizeof(float));
    std::vector<float> wp;
    std::vector<_Float16> wph, xh;
    const void *hx = x, *hw = nullptr;
    size_t wbytes = 0;
    if (precision == 1) {
        wph.assign((size_t)L.npad_h * L.nchunks_h * 64, (_Float16)0.0f);
        L.wscale = weight_prescale(w, (size_t)k * k * Cin * Cout);
        pack_conv_weights_h3(w, k, Cin, Cout, nullptr, Cin, L.cb_log2, L.tpc_log2, L.cpb, L.nchunks_h, L.wscale, wph.data());
        hw = wph.data(); wbytes = wph.size() * sizeof(_Float16);
        const int cb = 1 << L.cb_log2;                       // float32 NHWC -> split-fp16 blocked
        xh.resize(nx * 2);
        for (size_t px = 0; px < nx / Cin; ++px)
            for (int ch = 0; ch < Cin; ++ch) {
                _Float16* blk = xh.data() + px * Cin * 2 + (size_t)(ch / cb) * cb * 2;
                split_f16(x[px * Cin + ch], blk + ch % cb, blk + cb + ch % cb);
            }
        hx = xh.data();
    } else {
        wp.assign((size_t)L.npad * L.kpad, 0.f);
        pack_conv_weights(w, k, Cin, Cout, nullptr, Cin, L.npad, L.kpad, wp.data());
        hw = wp.data(); wbytes = wp.size() * sizeof(float);
    }
    DevMem<void> dx, dw, db, dy, dz;
    hipError_t e = hipSuccess;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    chk(dev_alloc(&dx, nx * 4)); chk(dev_alloc(&dw, wbytes));
    chk(dev_alloc(&db, bp.size() * 4)); chk(dev_alloc(&dy, ny * 4));
    chk(dev_alloc(&dz, 256));
    if (e == hipSuccess) {
        chk(hipMemset(dz.get(), 0, 256));
        chk(hipMemcpy(dx.get(), hx, nx * 4, hipMemcpyHostToDevice));
        chk(hipMemcpy(dw.get(), hw, wbytes, hipMemcpyHostToDevice));
        chk(hipMemcpy(db.get(), bp.data(), bp.size() * 4, hipMemcpyHostToDevice));
        if (precision == 1) {
            const int tile = Cout <= 32 ? TILE_128x32 : Cout <= 64 ? TILE_256x64 : Cout <= 128 ? TILE_256x128 : TILE_128x256;
            const TileShape ts = tile_shape(tile);
            // float32 output, no shared-tap staging (the generic instantiations have none), unscaled storage
            ConvParamsH p = fill_params_h3(L, LayerCall{0, Cin, H, W, Cout, true, N, false, false}, false, 0, 0);
            p.x = static_cast<const uint8_t*>(dx.get()); p.w = static_cast<const uint8_t*>(dw.get());
            p.bias = static_cast<const float*>(db.get()); p.y = static_cast<uint8_t*>(dy.get());
            p.zeros = static_cast<const uint8_t*>(dz.get());
            p.x_pix_log2 = -1; p.ntiles_n = L.npad_h / ts.bn; p.relu = relu;
            dim3 grid((p.M + ts.bm - 1) / ts.bm * p.ntiles_n, 1);
            const hipError_t le = launch_h3_generic(k, stride, tile, p, grid, nullptr);
            chk(le);
        } else {
            ConvParams p = fill_params_f32(L, LayerCall{0, Cin, H, W, Cout, true, N, false, false});
            p.x = static_cast<const float*>(dx.get()); p.w = static_cast<const float*>(dw.get());
            p.bias = static_cast<const float*>(db.get()); p.y = static_cast<float*>(dy.get());
            p.zeros = static_cast<const float*>(dz.get());
            p.relu = relu;
            dim3 grid((p.M + BM - 1) / BM * p.ntiles_n, 1);
            chk(launch_conv(k, stride, L.BN, p, grid, nullptr));
        }
        chk(hipDeviceSynchronize());
        chk(hipMemcpy(y, dy.get(), ny * 4, hipMemcpyDeviceToHost));
    }
    if (e != hipSuccess) return bad(hipGetErrorString(e), DAVO_ERR_HIP);
    return DAVO_OK;
}

}  // extern "C"

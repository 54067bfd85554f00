// api.hip — the context of libdavo_hip.so (include/davo_hip.h): its life cycle, weight loading, the settings (label format,
// posenn_se, precision, pairs, impl, stream, in-flight slots, the option table), the range-state calls and davo_synchronize.
// The calls that take a batch are entry.hip (davo_forward_features / davo_forward_heat: export.hip), the test hooks hooks.hip;
// the forward plan itself is forward.hip; the f16x3 range guard around it is range_guard.hip (bookkeeping: range_book.h);
// the RCCL communicator is comm.hip.
#include <cstring>

#include "ctx.h"
#include "plan.h"
#include "pool_plan.h"

using namespace davo;

namespace davo {

// hipMemset runs on the null stream and may return before the fill has run; the context's streams are non-blocking, so nothing
// orders them behind it.  (Found as one wrong batch in twenty streamed runs: the zero fill of a slot's new staging set landed on
// top of the first batch's freshly copied flow planes, profiles/r05f_stream_flake.log.)  Returns when the bytes ARE zero.
int zero_now(davo_ctx* c, void* p, size_t bytes) {
    HIP_TRY(c, hipMemset(p, 0, bytes));
    HIP_TRY(c, hipStreamSynchronize(nullptr));
    return DAVO_OK;
}

// Room for max_batch windows of every plane the variant reads.  zero_unread: the flow and label planes start out zero - what the path
// never reads (flow planes 2,3; the target frame's label map) is never copied into a davo_submit staging set: defined contents all the same
int alloc_input_set(davo_ctx* c, InputSet* out, bool zero_unread) {
    const PlaneBytes nb = plane_bytes(c);
    const size_t n = (size_t)c->max_batch;
    InputSet s;
    HIP_TRY(c, dev_alloc(&s.img, nb.img * n));
    HIP_TRY(c, dev_alloc(&s.flow, nb.flow * n));
    HIP_TRY(c, dev_alloc(&s.seg, nb.seg * n));
    if (needs_depth(c)) HIP_TRY(c, dev_alloc(&s.depth, nb.depth * n));      // always copied whole
    if (zero_unread) {
        { int rc = zero_now(c, s.flow.get(), nb.flow * n); if (rc) return rc; }
        { int rc = zero_now(c, s.seg.get(), nb.seg * n); if (rc) return rc; }
    }
    *out = std::move(s);
    return DAVO_OK;
}

}  // namespace davo

namespace {

// the feature-attention variant's room in one slot (posenn_se.h): the 512-channel scaled tensor of cnv5's geometry (2,048 bytes per
// pixel in either arithmetic mode), the scale table and the squeeze's partial sums.  Nothing of it exists with the mode off.
int alloc_se_workspace(davo_ctx* c, Slot* s) {
    const size_t NB = 2 * (size_t)c->max_batch;
    s->se.reset();
    SeWorkspace w;
    HIP_TRY(c, dev_alloc(&w.d_se, NB * c->H2 * c->W2 * 512));
    HIP_TRY(c, dev_alloc(&w.d_se_scale, NB * 2 * 256));
    HIP_TRY(c, dev_alloc(&w.d_se_partial, NB * SE5_CHUNKS * 256));
    s->se = std::move(w);
    return DAVO_OK;
}

// att_source 14..17: the pool plan of the context's image size, once, on the device (pool_plan.h)
int build_pool_plan(davo_ctx* c) {
    const PoolPlan p = pool_plan(c->H, c->W, c->v.att_source);
    if (p.cells.empty() || p.items.empty() || 2 * (int)p.cells.size() != att_se_in(c->v.att_source))
        return fail(c, DAVO_ERR_INVALID, "internal: pool plan of %dx%d, att_source %d has %zu cells, %zu work items", c->H, c->W, c->v.att_source,
                    p.cells.size(), p.items.size());
    std::vector<int> items;
    std::vector<float> inv;
    for (const PoolItem& it : p.items) { items.push_back(it.y0); items.push_back(it.y1); items.push_back(it.x0); items.push_back(it.x1); }
    for (const PoolCell& cell : p.cells) inv.push_back(cell.inv_div);
    c->d_pool_items = upload_table(items);
    c->d_pool_cell_first = upload_table(p.cell_first);
    c->d_pool_inv_div = upload_table(inv);
    if (!c->d_pool_items || !c->d_pool_cell_first || !c->d_pool_inv_div) HIP_TRY(c, hipErrorOutOfMemory);
    c->pool = PoolDev{c->d_pool_items.get(), c->d_pool_cell_first.get(), c->d_pool_inv_div.get(), (int)p.items.size(), (int)p.cells.size()};
    return DAVO_OK;
}

// one more in-flight slot (stream + activation workspace for max_batch triplets): appended once it is complete
int add_slot(davo_ctx* c) {
    const size_t NB = 2 * (size_t)c->max_batch;
    Slot s;
    HIP_TRY(c, stream_create(&s.stream));
    for (int i = 0; i < 7; ++i) HIP_TRY(c, dev_alloc(&s.d_act[i], NB * c->slot_floats_per_img[i]));      // the decoupled widths, whatever the heads are now
    HIP_TRY(c, dev_alloc(&s.d_packed, NB * (size_t)c->H * c->W * 10));
    // squeeze partials: se_flow [B][2 sources][SQ_CHUNKS][2] floats, the class-table sources [B][3 frames][SQ_CHUNKS][SQ_REC] words
    // (the pooled flow-attention variants: [B][2 sources][work items][2] floats)
    const size_t partial_floats = att_pooled(c->v.att_source) ? (size_t)c->max_batch * 2 * c->pool.n_items * 2
                                                              : (size_t)c->max_batch * SQ_CHUNKS * (att_class_table(c->v.att_source) ? 3 * SQ_REC : 2 * 2);
    HIP_TRY(c, dev_alloc(&s.d_partial, partial_floats));
    HIP_TRY(c, dev_alloc(&s.d_tab, (size_t)c->max_batch * 3 * NCLS));
    if (c->v.att_source == ATT_DEPTH_SPLIT) HIP_TRY(c, dev_alloc(&s.d_tab_far, (size_t)c->max_batch * 3 * NCLS));      // the far MLP's tables: this source only
    HIP_TRY(c, dev_alloc(&s.d_pose_partial, NB * 2 * PH_SPLIT * 3));
    { int rc = zero_now(c, s.d_partial.get(), partial_floats * sizeof(float)); if (rc) return rc; }
    if (att_pooled(c->v.att_source)) {      // the descriptors [B][2][D]: this family only; zero, so that a one-pair batch leaves the other source's row defined
        const size_t desc_floats = (size_t)c->max_batch * 2 * 2 * c->pool.n_cells;
        HIP_TRY(c, dev_alloc(&s.d_desc, desc_floats));
        { int rc = zero_now(c, s.d_desc.get(), desc_floats * sizeof(float)); if (rc) return rc; }
    }
    const size_t counters = (size_t)c->max_batch + 1 + SK_TILE_COUNTERS;
    HIP_TRY(c, dev_alloc(&s.d_counters, counters));
    { int rc = zero_now(c, s.d_counters.get(), counters * sizeof(unsigned)); if (rc) return rc; }
    if (c->posenn_se) { int rc = alloc_se_workspace(c, &s); if (rc) return rc; }
    c->slots.push_back(std::move(s));
    return DAVO_OK;
}

}  // namespace

// ============================================================================================
extern "C" {

int davo_create(davo_ctx** out, int device, int H, int W, int max_batch, const davo_variant* v) {
    if (!out || !v) return DAVO_ERR_INVALID;
    *out = nullptr;
    davo_ctx* c = new davo_ctx();
    *out = c;                                   // returned even on failure so the message is readable
    c->device = device; c->H = H; c->W = W; c->max_batch = max_batch;
    c->v = Variant{v->cin_per_frame, v->cnv6_out, v->se_act, v->norm_flow, v->abs_mode, v->att_source,
                   v->mask_rgb, v->mask_info};
    if (H < 16 || W < 16 || H % 4 || W % 4) return fail(c, DAVO_ERR_INVALID, "H and W must be multiples of 4 and >= 16 (got %dx%d)", H, W);
    if (max_batch < 1) return fail(c, DAVO_ERR_INVALID, "max_batch must be >= 1");
    if (v->cin_per_frame != 5 && v->cin_per_frame != 3) return fail(c, DAVO_ERR_INVALID, "cin_per_frame must be 3 or 5");
    if (ilog2_exact(v->cnv6_out) < 5 || v->cnv6_out > 256) return fail(c, DAVO_ERR_INVALID, "cnv6_out must be 32, 64, 128 or 256");
    if (v->se_act < 0 || v->se_act > 2 || v->abs_mode < 0 || v->abs_mode > 3 || v->att_source < 0 || v->att_source > ATT_MAX)
        return fail(c, DAVO_ERR_INVALID, "variant field out of range");
    int ndev = 0;
    HIP_TRY(c, hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(c, DAVO_ERR_INVALID, "device %d not present (%d visible)", device, ndev);
    HIP_TRY(c, hipSetDevice(device));
    {   // the launch planner sizes whole rounds for the CUs this device really has (a partitioned MI355X exposes fewer than 256)
        hipDeviceProp_t prop;
        HIP_TRY(c, hipGetDeviceProperties(&prop, device));
        c->dev_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        c->ncu = c->dev_cus;
    }
    c->needed = needed_names(c->v);

    c->H1 = (H + 1) / 2; c->W1 = (W + 1) / 2;
    c->H2 = (c->H1 + 1) / 2; c->W2 = (c->W1 + 1) / 2;
    c->H3 = (c->H2 + 1) / 2; c->W3 = (c->W2 + 1) / 2;
    const int c6 = c->v.cnv6_out;
    init_posenn_layers(c->L, c6);

    const int ch[7] = {16, 32, 64, 128, 256, 2 * c6, 512};
    const size_t px[7] = {(size_t)c->H1 * c->W1, (size_t)c->H2 * c->W2, (size_t)c->H2 * c->W2, (size_t)c->H2 * c->W2,
                          (size_t)c->H2 * c->W2, (size_t)c->H2 * c->W2, (size_t)c->H3 * c->W3};
    for (int i = 0; i < 7; ++i) {
        c->act_ch[i] = ch[i];
        c->act_floats_per_img[i] = px[i] * ch[i];
        c->slot_floats_per_img[i] = px[i] * ch[i];
    }
    if (att_pooled(c->v.att_source)) { int rc = build_pool_plan(c); if (rc) return rc; }      // the slots' squeeze partials are sized by it
    { int rc = add_slot(c); if (rc) return rc; }
    HIP_TRY(c, dev_alloc(&c->d_zeros, 256 / sizeof(float)));
    { int rc = zero_now(c, c->d_zeros.get(), 256); if (rc) return rc; }
    HIP_TRY(c, dev_alloc(&c->d_range_base, (1 + RANGE_RING) * RANGE_WORDS));
    { int rc = zero_now(c, c->d_range_base.get(), (1 + RANGE_RING) * RANGE_WORDS * sizeof(unsigned)); if (rc) return rc; }
    return DAVO_OK;
}

int davo_set_posenn_se(davo_ctx* c, int mode) {
    if (!c) return DAVO_ERR_INVALID;
    if (mode != 0 && mode != 1) return fail(c, DAVO_ERR_INVALID, "posenn_se mode must be 0 (none) or 1 (insert)");
    if (!c->weights.empty() || c->forward_seen)
        return fail(c, DAVO_ERR_INVALID, "davo_set_posenn_se must be called before the first davo_load_weight and the first forward "
                    "(it changes the variant's variables and cnv6's layout)");
    if (mode && c->v.att_source != 0)
        return fail(c, DAVO_ERR_INVALID, "the feature-attention PoseNN (`-se_insert') runs with att_source 0 (`-no_segmask') only, got %d", c->v.att_source);
    if (mode && triplet(c)) return fail(c, DAVO_ERR_INVALID, "the three-frame PoseNN (davo_set_posenn_topology) has no feature-attention form");
    if (mode && coupled(c)) return fail(c, DAVO_ERR_INVALID, "the coupled PoseNN (davo_set_posenn_heads) has no feature-attention form");
    HIP_TRY(c, hipSetDevice(c->device));
    c->posenn_se = mode;
    // the heads read different inputs now: cnv6 becomes one group per head, the grouped path cnv7 runs on (forward.hip)
    const int c6 = c->v.cnv6_out;
    if (mode) init_layer(c->L[5], "cnv6", 3, 1, 2, 256, c6, 2);
    else if (coupled(c)) init_coupled_head(c->L, c6);      // mode 0 on a coupled context: its own one-group cnv6
    else init_layer(c->L[5], "cnv6", 3, 1, 2, 256, 2 * c6, 1);
    c->needed = needed_names(c->v, mode, coupled(c));
    for (Slot& s : c->slots) {
        if (mode) { int rc = alloc_se_workspace(c, &s); if (rc) return rc; }
        else s.se.reset();
    }
    c->last_slot = 0;
    return DAVO_OK;
}

int davo_set_posenn_topology(davo_ctx* c, int topology) {
    if (!c) return DAVO_ERR_INVALID;
    if (topology != DAVO_POSENN_PAIRS && topology != DAVO_POSENN_TRIPLET)
        return fail(c, DAVO_ERR_INVALID, "topology must be DAVO_POSENN_PAIRS (0) or DAVO_POSENN_TRIPLET (1), got %d", topology);
    if (!c->weights.empty() || c->forward_seen)
        return fail(c, DAVO_ERR_INVALID, "davo_set_posenn_topology must be called before the first davo_load_weight and the first forward "
                    "(it changes the shapes of cnv1 and pred and cnv1's layout)");
    if (topology == DAVO_POSENN_TRIPLET) {
        if (att_reads_depth(c->v.att_source))
            return fail(c, DAVO_ERR_INVALID, "the three-frame PoseNN has no form of the depth sources (att_source 11..13, got %d)", c->v.att_source);
        if (c->posenn_se)
            return fail(c, DAVO_ERR_INVALID, "the three-frame PoseNN has no feature-attention form: davo_set_posenn_se(ctx, 1) is set");
        if (c->pairs != PAIRS_BOTH)
            return fail(c, DAVO_ERR_INVALID, "the three-frame PoseNN yields both poses from one pass: davo_set_pairs must be DAVO_PAIRS_BOTH, is %d", c->pairs);
        if (c->impl != 0) return fail(c, DAVO_ERR_INVALID, "the three-frame PoseNN has no direct-convolution form: davo_set_impl(ctx, 1) is set");
        if (c->fx_on || c->heat)
            return fail(c, DAVO_ERR_INVALID, "the three-frame PoseNN has no feature or heat export: switch the exports off first");
        if (coupled(c))
            return fail(c, DAVO_ERR_INVALID, "the three-frame coupled PoseNN (couple_net_v0_dilation) is not built: davo_set_posenn_heads(ctx, DAVO_POSENN_HEADS_COUPLED) is set");
    }
    c->topology = topology;
    // cnv1 reads 16 packed channels (prologue.h, mask_pack3) instead of 8; every other layer is the same, on B images instead of 2 B
    init_layer(c->L[0], "cnv1", 7, 2, 1, topology == DAVO_POSENN_TRIPLET ? 16 : 8, 16, 1);
    c->last_slot = 0;
    return DAVO_OK;
}

int davo_set_posenn_heads(davo_ctx* c, int heads) {
    if (!c) return DAVO_ERR_INVALID;
    if (heads != DAVO_POSENN_HEADS_DECOUPLED && heads != DAVO_POSENN_HEADS_COUPLED)
        return fail(c, DAVO_ERR_INVALID, "heads must be DAVO_POSENN_HEADS_DECOUPLED (0) or DAVO_POSENN_HEADS_COUPLED (1), got %d", heads);
    if (!c->weights.empty() || c->forward_seen)
        return fail(c, DAVO_ERR_INVALID, "davo_set_posenn_heads must be called before the first davo_load_weight and the first forward "
                    "(it changes the head's variables and the layout of cnv6, cnv7 and pred)");
    if (heads == DAVO_POSENN_HEADS_COUPLED) {
        if (triplet(c))
            return fail(c, DAVO_ERR_INVALID, "the three-frame coupled PoseNN (couple_net_v0_dilation) is not built: davo_set_posenn_topology(ctx, DAVO_POSENN_TRIPLET) is set");
        if (c->posenn_se)
            return fail(c, DAVO_ERR_INVALID, "the coupled PoseNN has no feature-attention form: davo_set_posenn_se(ctx, 1) is set");
        if (c->fx_on || c->heat)
            return fail(c, DAVO_ERR_INVALID, "the coupled PoseNN has no feature or heat export: switch the exports off first");
    }
    c->heads = heads;
    const int c6 = c->v.cnv6_out;
    // coupled: cnv6 one GEMM of c6 columns, cnv7 one group over all of them; the activations are [images][H2][W2][c6] and
    // [images][H3][W3][256].  The slots' buffers were sized for the decoupled widths (2 c6 and 512 channels) and the pose head's partial
    // sums for two heads of three columns: the coupled tensors must fit them
    if (heads == DAVO_POSENN_HEADS_COUPLED) init_coupled_head(c->L, c6);
    else {
        init_layer(c->L[5], "cnv6", 3, 1, 2, 256, c->posenn_se ? c6 : 2 * c6, c->posenn_se ? 2 : 1);
        init_layer(c->L[6], "cnv7", 3, 2, 1, c6, 256, 2);
    }
    const int ch5 = heads == DAVO_POSENN_HEADS_COUPLED ? c6 : 2 * c6, ch7 = heads == DAVO_POSENN_HEADS_COUPLED ? 256 : 512;
    const size_t px5 = (size_t)c->H2 * c->W2, px7 = (size_t)c->H3 * c->W3;
    static_assert(PH_SPLIT * 6 <= 2 * PH_SPLIT * 3, "the slots' pose partials [images][2][PH_SPLIT][3] hold the coupled head's [images][PH_SPLIT][6]");
    if (px5 * ch5 > c->slot_floats_per_img[5] || px7 * ch7 > c->slot_floats_per_img[6])      // what add_slot allocates, for every slot built before or after this call
        return fail(c, DAVO_ERR_INVALID, "internal: cnv6 / cnv7 of %d / %d channels do not fit the slots' buffers (%zu / %zu floats per image)", ch5, ch7,
                    c->slot_floats_per_img[5], c->slot_floats_per_img[6]);
    c->act_ch[5] = ch5; c->act_floats_per_img[5] = px5 * ch5;
    c->act_ch[6] = ch7; c->act_floats_per_img[6] = px7 * ch7;
    c->needed = needed_names(c->v, c->posenn_se, coupled(c));
    c->last_slot = 0;
    return DAVO_OK;
}

// The three format setters' one body.  kind: "label" | "flow" | "depth" (the setter is davo_set_<kind>_format); field: its member of
// the context's InputFormat; name0 / name1: the header's names of the values 0 and 1.
static int set_input_format(davo_ctx* c, const char* kind, int InputFormat::*field, int fmt, const char* name0, const char* name1) {
    if (!c) return DAVO_ERR_INVALID;
    InputFormat next = c->fmt;
    next.*field = fmt;
    if (!valid(next)) return fail(c, DAVO_ERR_INVALID, "%s format must be %s (0) or %s (1), got %d", kind, name0, name1, fmt);
    // everything sized by plane_bytes() follows the format: it is fixed once inputs were taken or a set of them was allocated
    bool sets = static_cast<bool>(c->host) || static_cast<bool>(c->snaps) || static_cast<bool>(c->track);
    for (const InputSet& s : c->stream_sets) sets = sets || s.built();
    for (const FrameSet& s : c->frame_sets) sets = sets || s.built();
    if (c->inputs_seen || c->forward_seen || sets)
        return fail(c, DAVO_ERR_INVALID, "davo_set_%s_format must be called before the first call that takes inputs "
                    "(the staging sets, the range guard's snapshots and every copy are sized by it)", kind);
    c->fmt = next;
    return DAVO_OK;
}

int davo_set_label_format(davo_ctx* c, int fmt) { return set_input_format(c, "label", &InputFormat::label, fmt, "DAVO_LABELS_F32", "DAVO_LABELS_U8"); }
int davo_set_flow_format(davo_ctx* c, int fmt) { return set_input_format(c, "flow", &InputFormat::flow, fmt, "DAVO_FLOW_F32", "DAVO_FLOW_F16"); }
int davo_set_depth_format(davo_ctx* c, int fmt) { return set_input_format(c, "depth", &InputFormat::depth, fmt, "DAVO_DEPTH_F32", "DAVO_DEPTH_F16"); }
int davo_get_label_format(const davo_ctx* c) { return c ? c->fmt.label : DAVO_ERR_INVALID; }
int davo_get_flow_format(const davo_ctx* c) { return c ? c->fmt.flow : DAVO_ERR_INVALID; }
int davo_get_depth_format(const davo_ctx* c) { return c ? c->fmt.depth : DAVO_ERR_INVALID; }

int davo_load_weight(davo_ctx* c, const char* tf_name, const float* data, const int64_t* shape, int ndim) {
    // ndim 0: a scalar variable (the depth threshold); shape may then be null
    if (!c || !tf_name || !data || ndim < 0 || ndim > 4 || (!shape && ndim > 0)) return fail(c, DAVO_ERR_INVALID, "bad argument to davo_load_weight");
    std::vector<int64_t> want;
    if (!expected_shape(c, tf_name, &want)) return fail(c, DAVO_ERR_INVALID, "unknown variable `%s'", tf_name);
    bool listed = false;
    for (auto& n : c->needed) listed |= (n == tf_name);
    if (!listed) return fail(c, DAVO_ERR_INVALID, "variable `%s' is not part of this variant", tf_name);
    std::vector<int64_t> got;
    if (ndim > 0) got.assign(shape, shape + ndim);
    if (got != want) {
        std::string g, w;
        for (auto d : got) g += std::to_string(d) + ",";
        for (auto d : want) w += std::to_string(d) + ",";
        return fail(c, DAVO_ERR_INVALID, "`%s': shape [%s] does not match expected [%s]", tf_name, g.c_str(), w.c_str());
    }
    size_t n = 1;
    for (auto d : got) n *= (size_t)d;
    HostTensor& t = c->weights[tf_name];
    t.shape = got;
    t.data.assign(data, data + n);
    if (strcmp(tf_name, DEPTH_THRESHOLD_NAME) == 0) c->depth_thr = data[0];      // the kernels take it as an argument from this host copy
    HIP_TRY(c, hipSetDevice(c->device));
    // the kernels read the small dense tensors (SE fully-connected layers, static channel weights) in the reference's own layout;
    // the convolution tensors are re-laid-out at the first forward (weights.hip) and their raw device copy is only the test hook's
    // (impl 1: uploaded on demand, forward.hip) - 20 hipMalloc + copies less in front of a rank's first batch
    const std::string nm = tf_name;
    const bool dense = is_dense_weight(nm);
    t.dev.reset();
    if (dense) { int rc = upload(c, t.data, &t.dev); if (rc) return rc; }
    c->packed_ready = false;
    c->packed_h_ready = false;
    c->pred_ready = false;
    return DAVO_OK;
}

int davo_weights_missing(davo_ctx* c) {
    if (!c) return DAVO_ERR_INVALID;
    std::string names;
    const int n = missing_weights(c, &names);
    if (n) c->err = "weights not loaded: " + names;
    return n;
}

int davo_range_stats(davo_ctx* c, long long* recalibrations, long long* f32_batches, long long* reissued) {
    if (!c) return DAVO_ERR_INVALID;
    if (recalibrations) *recalibrations = c->n_recalibrations;
    if (f32_batches) *f32_batches = c->n_f32_batches;
    if (reissued) *reissued = c->n_reissued;
    return DAVO_OK;
}

int davo_activation_range(davo_ctx* c, float* max_abs, int* shifts, int reset) {
    if (!c) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = judge_all(c); if (rc && rc != DAVO_ERR_RANGE) return rc; }      // every issued batch's record is in range_seen now
    for (int i = 0; i < 6; ++i) {
        if (max_abs) max_abs[i] = c->range_seen[i];
        if (shifts) shifts[i] = c->act_shift[i];
    }
    if (reset) for (int i = 0; i < 6; ++i) c->range_seen[i] = 0.f;
    return DAVO_OK;
}

const char* davo_range_report(const davo_ctx* c) { return c ? c->range_report.c_str() : ""; }

int davo_set_activation_shifts(davo_ctx* c, const int* shifts) {
    if (!c) return DAVO_ERR_INVALID;
    { int rc = judge_all(c); if (rc) return rc; }             // batches issued under the old scales get their verdict first
    { int rc = freeze_pending_and_reset_ring(c); if (rc) return rc; }      // maxima stored under the old scales say nothing about the new
    c->book.host_record_stale();                                             // ... the host path's record included: its next call starts afresh
    for (int i = 0; i < 6; ++i) {
        const int s = shifts ? shifts[i] : 0;
        if (s < -60 || s > 60) return fail(c, DAVO_ERR_INVALID, "activation shift %d outside [-60,60]", s);
        c->act_shift[i] = s;
    }
    return DAVO_OK;
}

int davo_reset_range_state(davo_ctx* c) {
    if (!c) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    // batches issued so far get their verdict - and their recovery - under the scales they ran with; with "auto_range" 0 a failed
    // verdict is this call's result, after the state has been reset all the same
    const int verdict = judge_all(c);
    if (verdict && verdict != DAVO_ERR_RANGE) return verdict;
    const std::string verdict_err = c->err;
    { int rc = freeze_pending_and_reset_ring(c); if (rc) return rc; }       // no ticket is pending: this zeroes the ring's records
    { int rc = zero_now(c, c->d_range_base.get(), RANGE_WORDS * sizeof(unsigned)); if (rc) return rc; }
    for (int i = 0; i < 7; ++i) c->act_shift[i] = 0;
    for (int i = 0; i < 6; ++i) c->range_seen[i] = 0.f;
    c->book.reset();                                                         // the counters' and the cursor's initial values, no deferred verdict
    c->range_report.clear();
    if (verdict) { c->err = verdict_err; return verdict; }
    return DAVO_OK;
}

// the body of davo_calibrate / davo_calibrate_depth: a window batch on the device, no poses wanted
static int calibrate_entry(davo_ctx* c, int B, Batch b, int* shifts_out) {
    { int rc = check_batch(c, &b, B, true); if (rc) return rc; }
    { int rc = refuse_while_tracking(c, "davo_calibrate"); if (rc) return rc; }
    c->inputs_seen = true;
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = judge_all(c); if (rc) return rc; }             // batches issued under the old scales get their verdict first
    { int rc = freeze_pending_and_reset_ring(c); if (rc) return rc; }
    DevMem<float> d_pose;
    HIP_TRY(c, dev_alloc(&d_pose, (size_t)B * 12));
    Inputs in = b.win;
    if (c->flip) { int rc = mirror_device_batch(c, b.win, B, &in); if (rc) return rc; }      // the caller's buffers are only read
    const int rc = calibrate_on(c, B, in, d_pose.get(), PAIRS_BOTH);
    if (rc == DAVO_OK && shifts_out) for (int i = 0; i < 6; ++i) shifts_out[i] = c->act_shift[i];
    return rc;
}

int davo_calibrate(davo_ctx* c, int B, const void* d_img, const void* d_flow, const void* d_seg, int* shifts_out) {
    return calibrate_entry(c, B, window_batch("davo_calibrate", true, false, d_img, d_flow, d_seg, nullptr), shifts_out);
}

int davo_calibrate_depth(davo_ctx* c, int B, const void* d_img, const void* d_flow, const void* d_seg, const void* d_depth, int* shifts_out) {
    return calibrate_entry(c, B, window_batch("davo_calibrate", true, true, d_img, d_flow, d_seg, d_depth), shifts_out);
}

const char* davo_last_error(const davo_ctx* c) { return c ? c->err.c_str() : "null context"; }

// Every member of the context frees what it owns (owned.h), in any order: the streams are drained first so that nothing on the
// device still reads what goes.
void davo_destroy(davo_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    drain_own_streams(c);
    comm_release(c);
    delete c;
}

int davo_synchronize(davo_ctx* c) {
    if (!c) return DAVO_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    // f16x3: the batches davo_forward_device issued since the last synchronize are judged here (the asynchronous
    // entry point cannot know its own result).  A failed verdict re-issues that batch (recover_batch); with "auto_range" 0
    // it is returned as DAVO_ERR_RANGE = some layer left the fp16-pair storage range.  davo_submit batches are delivered first.
    { int rc = deliver_all(c); if (rc) return rc; }
    return judge_all(c);
}
int davo_set_stream(davo_ctx* c, void* hip_stream) {
    if (!c) return DAVO_ERR_INVALID;
    if (hip_stream && c->inflight > 1) return fail(c, DAVO_ERR_INVALID, "a caller-owned stream needs davo_set_inflight(ctx, 1)");
    // batches issued on the stream the context is about to leave get their verdict (and any re-issue) while that stream is still
    // the one the context synchronises; the caller may destroy it afterwards
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = deliver_all(c); if (rc) return rc; }
    { int rc = judge_all(c); if (rc) return rc; }
    c->user_stream = static_cast<hipStream_t>(hip_stream);
    c->last_slot = 0;
    return DAVO_OK;
}

// (Re)create the slots' streams.  With cu_partition on, slot i of n gets the CUs [i*32/n, (i+1)*32/n) of EVERY XCD
// (hipExtStreamCreateWithCUMask; mask bit b = CU b/8 of XCD b%8, and a mask must leave no XCD empty — probed with
// tools/exp/cumask_probe.hip), so batches in different slots run side by side on disjoint CUs and the write bursts of
// one overlap the matrix phases of the other.  The launch planner then sizes rounds for 256/n CUs.
static int rebuild_slot_streams(davo_ctx* c, int n) {
    for (int i = 0; i < (int)c->slots.size(); ++i) {
        Slot& s = c->slots[i];
        StreamOwner fresh;                                                     // the slot keeps a live stream whatever fails here
        if (c->cu_partition && n > 1 && i < n && c->dev_cus == 256) {          // the mask layout below is the 8 XCD x 32 CU part's
            uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const int lo = i * 32 / n, hi = (i + 1) * 32 / n;                 // CU indices inside an XCD
            for (int b = 0; b < 256; ++b)
                if (b / 8 >= lo && b / 8 < hi) mask[b / 32] |= 1u << (b % 32);
            HIP_TRY(c, stream_create(&fresh, 8, mask));
        } else {
            HIP_TRY(c, stream_create(&fresh));
        }
        std::swap(s.stream, fresh);
        if (fresh) HIP_TRY(c, hipStreamDestroy(fresh.release()));              // the old one: a failure is reported
    }
    c->ncu = (c->cu_partition && n > 1 && c->dev_cus == 256) ? 256 / n : c->dev_cus;
    c->last_slot = 0;
    return DAVO_OK;
}

int davo_set_inflight(davo_ctx* c, int n) {
    if (!c || n < 1 || n > MAX_INFLIGHT) return fail(c, DAVO_ERR_INVALID, "inflight must be 1..4");
    if (n > 1 && c->user_stream) return fail(c, DAVO_ERR_INVALID, "in-flight slots use the context's own streams: clear davo_set_stream first");
    { int rc = refuse_while_tracking(c, "davo_set_inflight"); if (rc) return rc; }      // the session's ring is sized by the slots it began with
    HIP_TRY(c, hipSetDevice(c->device));
    { int rc = deliver_all(c); if (rc) return rc; }
    { int rc = sync_all_slots(c); if (rc) return rc; }
    while ((int)c->slots.size() < n) { int rc = add_slot(c); if (rc) return rc; }      // a slot that could not be built whole is not appended
    c->inflight = n;
    c->next_slot = 0;
    if (c->cu_partition || c->ncu != c->dev_cus) { int rc = rebuild_slot_streams(c, n); if (rc) return rc; }
    return DAVO_OK;
}

int davo_set_option(davo_ctx* c, const char* key, int value) {
    if (!c || !key) return DAVO_ERR_INVALID;
    const std::string k = key;
    if (const OptionRow* r = find_option(key)) {                 // a launch option: stored as its table row says (options.h)
        int stored;
        if (!option_store(*r, value, &stored)) return fail(c, DAVO_ERR_INVALID, "pad_classes must be 0, 1 or 8 + a layer mask (8..15), got %d", value);
        c->opt.*r->field = stored;
    }
    else if (k == "auto_range") { int rc = judge_all(c); if (rc) return rc; c->opt_auto_range = value != 0; }
    else if (k == "stable_inputs") { int rc = judge_all(c); if (rc) return rc; c->opt_stable_inputs = value != 0; }
    else if (k == "force_tile") {
        // test hook: every f16x3 layer the tile fits runs as ONE launch of that tile shape (plan.h tile ids; -1 = planner)
        if (value < -1 || value >= NUM_TILES) return fail(c, DAVO_ERR_INVALID, "force_tile must be -1..%d", NUM_TILES - 1);
        for (auto& L : c->L) L.tile_h = forced_tile_h(value, L.cout);
    }
    else if (k == "cu_partition") {
        if (c->user_stream) return fail(c, DAVO_ERR_INVALID, "cu_partition uses the context's own streams: clear davo_set_stream first");
        HIP_TRY(c, hipSetDevice(c->device));
        { int rc = sync_all_slots(c); if (rc) return rc; }
        c->cu_partition = value != 0;
        int rc = rebuild_slot_streams(c, c->inflight);
        if (rc) return rc;
    }
    else if (k == "profile_stride") { if (value < 1) return fail(c, DAVO_ERR_INVALID, "profile_stride must be >= 1"); c->prof_stride = value; c->prof_tick = 0; }
    else if (k == "host_chunk") { if (value < 0) return fail(c, DAVO_ERR_INVALID, "host_chunk must be >= 0"); c->host_chunk = value; }
    else return fail(c, DAVO_ERR_INVALID, "unknown option `%s'", key);
    return DAVO_OK;
}

int davo_get_option(const davo_ctx* c, const char* key, int* value) {
    if (!c || !key || !value) return DAVO_ERR_INVALID;
    const std::string k = key;
    if (const OptionRow* r = find_option(key)) *value = c->opt.*r->field;
    else if (k == "auto_range") *value = c->opt_auto_range;
    else if (k == "stable_inputs") *value = c->opt_stable_inputs;
    else if (k == "cu_partition") *value = c->cu_partition;
    else if (k == "profile_stride") *value = c->prof_stride;
    else if (k == "host_chunk") *value = c->host_chunk;
    else return DAVO_ERR_INVALID;                                  // unknown, or "force_tile": a value per layer
    return DAVO_OK;
}

int davo_option_info(int i, const char** name, int* stored_default) {
    if (i < 0 || i >= NUM_OPTIONS) return DAVO_ERR_INVALID;
    if (name) *name = OPTION_TABLE[i].name;
    if (stored_default) *stored_default = LaunchOptions{}.*OPTION_TABLE[i].field;
    return DAVO_OK;
}

int davo_option_store(const char* key, int value, int* stored) {
    const OptionRow* r = key && stored ? find_option(key) : nullptr;
    return r && option_store(*r, value, stored) ? DAVO_OK : DAVO_ERR_INVALID;
}

int davo_set_precision(davo_ctx* c, int precision) {
    if (!c || (precision != 0 && precision != 1)) return fail(c, DAVO_ERR_INVALID, "precision must be 0 (f32) or 1 (f16x3)");
    c->precision = precision;
    return DAVO_OK;
}

int davo_set_pairs(davo_ctx* c, int pairs) {
    if (!c) return DAVO_ERR_INVALID;
    if (pairs != DAVO_PAIRS_SRC0 && pairs != DAVO_PAIRS_SRC1 && pairs != DAVO_PAIRS_BOTH)
        return fail(c, DAVO_ERR_INVALID, "pairs must be DAVO_PAIRS_SRC0 (1), DAVO_PAIRS_SRC1 (2) or DAVO_PAIRS_BOTH (3), got %d", pairs);
    if (triplet(c) && pairs != DAVO_PAIRS_BOTH)
        return fail(c, DAVO_ERR_INVALID, "the three-frame PoseNN yields both poses from one pass: pairs must be DAVO_PAIRS_BOTH (3), got %d", pairs);
    c->pairs = pairs;              // batches in flight and their re-issues keep theirs (Ticket::pairs)
    return DAVO_OK;
}

int davo_get_pairs(const davo_ctx* c) { return c ? c->pairs : DAVO_ERR_INVALID; }

int davo_set_flip(davo_ctx* c, int on) {
    if (!c) return DAVO_ERR_INVALID;
    if (on != 0 && on != 1) return fail(c, DAVO_ERR_INVALID, "flip must be 0 (off) or 1 (on), got %d", on);
    c->flip = on != 0;             // batches in flight are staged already; their re-issues read the mirrored copy (entry.hip: Stager)
    return DAVO_OK;
}

int davo_get_flip(const davo_ctx* c) { return c ? (c->flip ? 1 : 0) : DAVO_ERR_INVALID; }

int davo_set_impl(davo_ctx* c, int impl) {
    if (!c || (impl != 0 && impl != 1)) return fail(c, DAVO_ERR_INVALID, "impl must be 0 (mfma) or 1 (direct)");
    if (impl && triplet(c)) return fail(c, DAVO_ERR_INVALID, "impl 1 (direct convolutions) has no three-frame PoseNN form");
    c->impl = impl;
    return DAVO_OK;
}

}  // extern "C"

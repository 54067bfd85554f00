"""Version-string parser for the DAVO pose-inference path.

The reference has no config object: ``DAVO(version)`` is configured by substring
tests on the ``--version`` flag, and the order of the ``if/elif`` chains matters
(reference ``davo.py:1010-1017`` se mode, ``:1027-1049`` PoseNN type, ``:1052``
cnv6 width, ``:1057-1073`` extra inputs, ``:1077-1085`` SE activation,
``:1089-1102`` SE input transform, ``:1117-1400`` attention source,
``:1417-1450`` masking).  ``parse_version`` walks the same chains in the same
order and returns a :class:`VariantConfig` for the variants this build runs on
the GPU; everything else the reference recognises is rejected with a
``NameError`` subclass, the exception type the reference itself raises for an
unknown network (``davo.py:1035-1037``, ``nets/attention_module.py:88``).
"""
import re
from dataclasses import dataclass

FLAGSHIP_VERSION = ("v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-segmask_all"
                    "-se_flow-abs_flow-fc_tanh")       # doc/arch-variants.md:8

NUM_SEG_CLASSES = 19            # utils/seg_utils/labels.py:64-101 (train ids 0..18)

# enums shared with include/davo_hip.h (davo_variant)
SE_ACT = {"relu": 0, "tanh": 1, "lrelu": 2}
ABS_MODE = {"none": 0, "h": 1, "v": 2, "all": 3}
ATT_SOURCE = {"ones": 0, "se_flow": 1, "static_src": 2, "static_all": 3,
              # class-table SE sources (davo.py:1274-1292, 1304-1310, 1341-1374): sigmoid table of 19 classes per frame
              "se_seg_wo_tgt": 4, "se_rgb_wo_tgt_to_seg": 5, "se_rgb_to_seg": 6,
              "se_SegFlow_to_seg_wo_tgt": 7, "se_SegFlow_to_seg": 8,
              "se_SegFlow_to_seg_8_wo_tgt": 9, "se_SegFlow_to_seg_8": 10,
              # depth-source class tables (davo.py:1211-1227): the descriptor is the mean of depth_frame + depth_tgt
              "se_depth_wo_tgt_to_seg": 11, "se_depth_to_seg": 12,
              # the flow-driven attention evaluated by two SE MLPs, selected per pixel by depth < depth_threshold (davo.py:1136-1155)
              "se_flow_depthseg_sep": 13}
# pooled flow attention (davo.py:1181-1186, 1193-1210): se_flow whose descriptor is a grid of window means (gp2x2 | SPP levels).  They
# continue davo_variant.att_source's numbering in a table of their own: ATT_SOURCE's extent, 0..13, is pinned by
# tests/test_depthseg_attention.py.  att_source_id() resolves a name of either table.
POOLED_ATT_SOURCE = {"se_gp2x2_flow_nobottle": 14, "se_spp21_flow": 15, "se_spp2_flow": 16, "se_spp864_flow": 17}
MASK_INFO = {"none": 0, "att": 1}


def att_source_id(name):
    """davo_variant.att_source of an attention source's name (ATT_SOURCE or POOLED_ATT_SOURCE)."""
    return ATT_SOURCE[name] if name in ATT_SOURCE else POOLED_ATT_SOURCE[name]


class UnsupportedVariantError(NameError):
    """A version substring the reference knows but this build does not run."""


@dataclass(frozen=True)
class VariantConfig:
    version: str
    major: str               # "v0" | "v1" (regex ^(v[0-9.]+), davo.py:1056-1057)
    use_flow_info: bool      # v1: concat raw flow as 2 extra channels per frame
    cnv6_out: int            # -cnv6_(\d+), default 128 (davo.py:1052-1053)
    se_act: str              # relu | tanh | lrelu  (davo.py:1077-1085)
    norm_flow: bool          # (f-0.32140523)/15.384229 before abs (davo.py:1089-1091)
    abs_mode: str            # none | h | v | all  (davo.py:1094-1102)
    att_source: str          # a key of ATT_SOURCE or POOLED_ATT_SOURCE
    mask_rgb: bool           # rgb_k *= att_k          (davo.py:1419-1423 / 1447-1450)
    mask_info: bool          # flow_k *= att_k         (davo.py:1430-1434)
    posenn_se: str = "none"  # none | insert: se_block on cnv5 ahead of each head's cnv6 (davo.py:1010-1011, nets/posenn.py:225-228);
                             # not a davo_variant field: Engine hands it to davo_set_posenn_se
    depth_thres_init: float = 15.0   # -se_flow_on_depthseg_.*layers_([0-9.]+): initialiser of se_flow/depth_threshold (davo.py:1136-1141);
                                     # inference uses the loaded value, so this only reaches synth.make_weights
    posenn: str = "pairs"    # pairs | triplet: decouple_sharednet_v0_dilation on two (tgt, src) images per window, or
                             # decouple_net_v0_dilation on one (tgt, src0, src1) image (davo.py:1038-1040, nets/posenn.py:69-131);
                             # not a davo_variant field: Engine hands it to davo_set_posenn_topology
    heads: str = "decoupled"  # decoupled | coupled: a rotation and a translation head (cnv6, cnv7, pred of three columns each), or the one head of
                              # couple_sharednet_v0_dilation (`-sharedNN-dilatedCouplePoseNN', davo.py:1031-1033, nets/posenn.py:133-187): one
                              # cnv6, one cnv7 that reads all of it, one pred of six columns; not a davo_variant field: Engine hands it to
                              # davo_set_posenn_heads

    @property
    def cin_per_frame(self):
        return 5 if self.use_flow_info else 3

    @property
    def tgt_attended(self):
        """The target frame's rgb is masked by its own class table, looked up through its own label map."""
        return self.att_source in _TGT_ATTENDED

    @property
    def needs_depth(self):
        """The attention source consumes the depth planes (a fourth input beside img, flow, seg)."""
        return self.att_source in _DEPTH_SOURCES

    @property
    def se_scope(self):
        """TF variable scope of the SE dense layers under pose_exp_net/, None without them."""
        return _SE_SCOPE.get(self.att_source)

    def as_c_ints(self):
        """Field order of ``davo_variant`` in include/davo_hip.h."""
        return (self.cin_per_frame, self.cnv6_out, SE_ACT[self.se_act],
                int(self.norm_flow), ABS_MODE[self.abs_mode],
                att_source_id(self.att_source), int(self.mask_rgb), int(self.mask_info))


# attention branches of davo.py:1117-1384 that come BEFORE "-se_flow" in the elif
# chain: if one of these matches, the reference never reaches the se_flow branch.
_BEFORE_SE_FLOW = ("-se_flow_on_depthseg_sharedlayers", "-se_flow_on_depthseg_seplayers",
                   "-se_flow_on_depthseg", "-se_mixDepthFlow", "-se_mixDispFlow")
# the one of them that runs: se_flow_near / se_flow_far tables selected per pixel by depth < depth_threshold (davo.py:1136-1155)
_DEPTHSEG_SEP = "-se_flow_on_depthseg_seplayers"
# branches AFTER "-se_flow" and before "-no_segmask", in the reference's order; the ones in _CLASS_TABLE_SOURCES run here,
# so do the pooled flow sources of _POOLED_FLOW_SOURCES; the rest need disparity, the 8-unit gp2x2 / `-se_spp_flow' strings (pinned as
# rejected) or an se_block / se_spp_block whose map is not a class table
_AFTER_SE_FLOW = ("-se_gp2x2_flow_nobottle", "-se_gp2x2_flow", "-se_spp21_flow", "-se_spp2_flow",
                  "-se_spp_flow", "-se_spp864_flow", "-se_depth_wo_tgt_to_seg", "-se_depth_to_seg",
                  "-se_depth_wo_tgt", "-se_depth", "-se_disp_wo_tgt_to_seg", "-se_disp_to_seg",
                  "-se_disp_wo_tgt", "-se_disp", "-se_rgb_wo_tgt_to_seg", "-se_rgb_to_seg",
                  "-se_rgb_wo_tgt", "-se_rgb", "-se_seg_wo_tgt", "-se_seg", "-se_gp2x2_seg",
                  "-se_spp21_seg", "-se_spp_seg_21", "-se_spp2_seg", "-se_spp_seg", "-se_spp864_seg",
                  "-se_SegFlow_to_seg_8_wo_tgt", "-se_SegFlow_to_seg_8", "-se_SegFlow_to_seg_wo_tgt",
                  "-se_SegFlow_to_seg", "-se_mixSegFlow", "-se_spp21_mixSegFlow")
# (substring, att_source) of the attention branches that run: a global-average-pooled descriptor, two dense layers and a
# 19-class sigmoid table looked up per pixel through the label map.  None of them creates the se_flow scope, so the second
# pair's target map is the target map (davo.py:1404-1414): ones for `_wo_tgt', the frame's own table otherwise.
_CLASS_TABLE_SOURCES = {"-se_seg_wo_tgt": "se_seg_wo_tgt",                          # davo.py:1304-1310, se_block ratio 1
                        "-se_rgb_wo_tgt_to_seg": "se_rgb_wo_tgt_to_seg",            # :1274-1283
                        "-se_rgb_to_seg": "se_rgb_to_seg",                          # :1284-1292
                        "-se_SegFlow_to_seg_8_wo_tgt": "se_SegFlow_to_seg_8_wo_tgt",  # :1341-1349
                        "-se_SegFlow_to_seg_8": "se_SegFlow_to_seg_8",              # :1350-1356
                        "-se_SegFlow_to_seg_wo_tgt": "se_SegFlow_to_seg_wo_tgt",    # :1358-1366
                        "-se_SegFlow_to_seg": "se_SegFlow_to_seg",                  # :1367-1374
                        "-se_depth_wo_tgt_to_seg": "se_depth_wo_tgt_to_seg",        # :1211-1219
                        "-se_depth_to_seg": "se_depth_to_seg"}                      # :1220-1227
# (substring, att_source) of the pooled flow-attention branches that run (davo.py:1181-1186, 1193-1210): se(se_input_flows[i], "se_flow",
# ..., mode='gp2x2' | 'spp').  `-se_gp2x2_flow_nobottle' stands before the bare `-se_gp2x2_flow' in _AFTER_SE_FLOW, as in the reference;
# `-se_spp864_flow' is the reference's own alias of `-se_spp_flow''s graph (davo.py:1205).  The bare `-se_gp2x2_flow' and `-se_spp_flow' stay
# rejected.  The scope is se_flow, so use_se_flow holds and both target maps are ones (davo.py:1404-1412).
_POOLED_FLOW_SOURCES = {"-se_gp2x2_flow_nobottle": "se_gp2x2_flow_nobottle", "-se_spp21_flow": "se_spp21_flow",
                        "-se_spp2_flow": "se_spp2_flow", "-se_spp864_flow": "se_spp864_flow"}
_TGT_ATTENDED = ("static_all", "se_rgb_to_seg", "se_SegFlow_to_seg", "se_SegFlow_to_seg_8", "se_depth_to_seg")
_DEPTH_SOURCES = ("se_depth_wo_tgt_to_seg", "se_depth_to_seg", "se_flow_depthseg_sep")
_SE_SCOPE = {"se_flow": "se_flow", "se_seg_wo_tgt": "se_seg", "se_rgb_wo_tgt_to_seg": "se_rgb", "se_rgb_to_seg": "se_rgb",
             "se_SegFlow_to_seg_wo_tgt": "se_segflow", "se_SegFlow_to_seg": "se_segflow",
             "se_SegFlow_to_seg_8_wo_tgt": "se_segflow", "se_SegFlow_to_seg_8": "se_segflow",
             "se_depth_wo_tgt_to_seg": "se_depth", "se_depth_to_seg": "se_depth",
             "se_gp2x2_flow_nobottle": "se_flow", "se_spp21_flow": "se_flow", "se_spp2_flow": "se_flow", "se_spp864_flow": "se_flow"}
# SE dense layer widths (in, hidden); the recovery layer always has the 19 classes
_SE_WIDTHS = {"se_flow": (2, 8), "se_seg_wo_tgt": (NUM_SEG_CLASSES, NUM_SEG_CLASSES), "se_rgb_wo_tgt_to_seg": (3, 8),
              "se_rgb_to_seg": (3, 8), "se_SegFlow_to_seg_wo_tgt": (NUM_SEG_CLASSES + 2, NUM_SEG_CLASSES),
              "se_SegFlow_to_seg": (NUM_SEG_CLASSES + 2, NUM_SEG_CLASSES),
              "se_SegFlow_to_seg_8_wo_tgt": (NUM_SEG_CLASSES + 2, 8), "se_SegFlow_to_seg_8": (NUM_SEG_CLASSES + 2, 8),
              "se_depth_wo_tgt_to_seg": (1, 8), "se_depth_to_seg": (1, 8),
              # pooled flow attention: D = 2 values per cell (4 | 4 + 1 | 4 | 64 + 36 + 16 cells); `_nobottle' is layer_channels [19, 19]
              "se_gp2x2_flow_nobottle": (8, NUM_SEG_CLASSES), "se_spp21_flow": (10, 8), "se_spp2_flow": (8, 8), "se_spp864_flow": (232, 8)}


def parse_version(version):
    """Return the :class:`VariantConfig` the reference graph builder would build.

    Follows ``DAVO.build_pose_test_graph_davo`` (reference ``davo.py:955-1458``).
    """
    assert version is not None                          # davo.py:959
    v = version

    # -- davo.py:960: depth files are read when the version contains `depth' or `disp'; only the two depth class-table
    #    sources (davo.py:1211-1227) consume them here
    if "disp" in v:
        # test_kitti_pose.py:91 reads depth files only for `depth'; for `disp' it hands the label maps in as depth (:61-64)
        raise UnsupportedVariantError("version `%s': disparity sources are not supported (the reference's driver feeds "
                                      "them the label maps, test_kitti_pose.py:61-64,91)." % v)
    if "-norm_depth" in v:
        raise UnsupportedVariantError("version `%s': `-norm_depth' is not supported (davo.py:1110-1111 iterates over "
                                      "what davo.py:1109 made a tensor)." % v)
    if "depth" in re.sub("-se_depth_wo_tgt_to_seg|-se_depth_to_seg|" + _DEPTHSEG_SEP, "", v):
        raise UnsupportedVariantError("version `%s': the only depth sources supported are `-se_depth_wo_tgt_to_seg', "
                                      "`-se_depth_to_seg' and `%s'." % (v, _DEPTHSEG_SEP))

    # -- davo.py:1010-1017: se_block inside the PoseNN (if / elif: `-se_insert' wins).  `-se_insert' runs where the attention
    #    source resolves to `ones' (checked below, once the source is known); the other two modes do not run
    posenn_se = "insert" if "-se_insert" in v else "none"
    for s in ("-se_skipadd", "-se_replace"):
        if s in v:
            raise UnsupportedVariantError("version `%s': `%s' PoseNN mode is not supported." % (v, s))

    # -- davo.py:1027-1049: PoseNN type
    heads = "decoupled"
    if "-sharedNN" in v:
        if "-dilatedPoseNN" in v:
            pass                                        # decouple_sharednet_v0_dilation
        elif "-dilatedCouplePoseNN" in v:
            heads = "coupled"                           # couple_sharednet_v0_dilation: the trunk of the above, one six-column head
        elif "-couplePoseNN" in v:
            raise NameError("not support `-sharedNN-couplePoseNN' mode.")      # davo.py:1035
        else:
            raise NameError("unknown PoseNN type.")                            # davo.py:1037
        posenn = "pairs"
    elif "-dilatedPoseNN" in v:
        posenn = "triplet"                              # decouple_net_v0_dilation: one (tgt, src0, src1) image per window
    elif "-dilatedCouplePoseNN" in v:
        raise UnsupportedVariantError("version `%s': couple_net_v0_dilation is not supported (without `-sharedNN' only "
                                      "`-dilatedPoseNN', decouple_net_v0_dilation, runs)." % v)
    elif "-couplePoseNN" in v:
        raise UnsupportedVariantError("version `%s': couple_net_v0 is not supported (without `-sharedNN' only "
                                      "`-dilatedPoseNN', decouple_net_v0_dilation, runs)." % v)
    else:
        raise UnsupportedVariantError("version `%s': decouple_net_v0 (no PoseNN substring) is not supported: only the "
                                      "`-sharedNN-dilatedPoseNN' and `-dilatedPoseNN' networks are." % v)

    for s in ("-batch_norm", "-dropout", "-seglabelid"):
        if s in v:
            raise UnsupportedVariantError("version `%s': `%s' is not supported." % (v, s))

    # -- davo.py:1052-1053
    m = re.search("-cnv6_([0-9]+)", v)
    cnv6_out = 128 if m is None else int(m.group(1))
    if cnv6_out not in (32, 64, 128, 256):          # the cnv7 k-order needs a power-of-two Cin
        raise UnsupportedVariantError("version `%s': cnv6 width %d is not supported." % (v, cnv6_out))

    # -- davo.py:1056-1065
    m = re.search("^(v[0-9.]+)", v)
    major = "v0" if m is None else m.group(1)
    use_flow_info = False
    if "v0" in major:
        pass
    elif "v1" in major:
        use_flow_info = True
    if ".555" in major:
        raise UnsupportedVariantError("version `%s': the `.555' masking variant is not supported." % v)

    # -- davo.py:1077-1085
    if "-fc_tanh" in v:
        se_act = "tanh"
    elif "-fc_lrelu" in v:
        se_act = "lrelu"
    else:
        se_act = "relu"

    # -- davo.py:1088-1102 (note -abs_flow_h / _v are tested before -abs_flow)
    norm_flow = "-norm_flow" in v
    if "-abs_flow_h" in v:
        abs_mode = "h"
    elif "-abs_flow_v" in v:
        abs_mode = "v"
    elif "-abs_flow" in v:
        abs_mode = "all"
    else:
        abs_mode = "none"

    # -- davo.py:1117-1400 attention source, same elif order
    before = next((s for s in _BEFORE_SE_FLOW if s in v), None)   # the first branch of the chain that matches
    if before is not None and before != _DEPTHSEG_SEP:
        raise UnsupportedVariantError("version `%s': `%s' attention is not supported." % (v, before))
    after = next((s for s in _AFTER_SE_FLOW if s in v), None)     # likewise, behind `-se_flow'
    depth_thres_init = 15.0
    if before == _DEPTHSEG_SEP:
        att_source = "se_flow_depthseg_sep"
        m = re.search("-se_flow_on_depthseg_.*layers_([0-9.]+)", v)   # davo.py:1136-1141
        if m is not None:
            try:
                depth_thres_init = float(m.group(1))                   # (the reference's float() raises on `1.2.3' or `.')
            except ValueError:
                raise UnsupportedVariantError("version `%s': `%s' behind `%s' is not a number." % (v, m.group(1), _DEPTHSEG_SEP)) from None
    elif "-se_flow" in v:
        att_source = "se_flow"
    elif after in _POOLED_FLOW_SOURCES:
        att_source = _POOLED_FLOW_SOURCES[after]
    elif after in _CLASS_TABLE_SOURCES:
        att_source = _CLASS_TABLE_SOURCES[after]
    elif after is not None:
        raise UnsupportedVariantError("version `%s': `%s' attention is not supported." % (v, after))
    else:
        if "-no_segmask" in v:
            att_source = "ones"
        elif "-segmask_" in v and "-static" in v:
            att_source = "static_src"          # davo.py:1390-1395: tgt map := ones
        else:
            att_source = "static_all"          # davo.py:1396-1400: tgt masked as well

    if posenn_se == "insert" and att_source != "ones":
        # "Ours w/ feature attention" is published with `-no_segmask' alone (doc/arch-variants.md); beside an input-attention
        # source the block is not built
        raise UnsupportedVariantError("version `%s': `-se_insert' PoseNN mode is supported with `-no_segmask' only "
                                      "(attention source `%s')." % (v, att_source))

    # -- davo.py:1415-1450 masking
    if use_flow_info:
        mask_rgb = "-segmask_" in v
        mask_info = mask_rgb and "-segmask_all" in v
    else:
        mask_rgb = "-segmask" in v
        mask_info = False

    if posenn == "triplet":
        # the three-frame network (davo.py:1460): every source that ends in the [B,3,19] class table the packer reads runs; the depth
        # planes and the feature-attention block have no three-frame form here
        if att_source in _DEPTH_SOURCES:
            raise UnsupportedVariantError("version `%s': the depth sources (`%s') are not supported with the three-frame "
                                          "`-dilatedPoseNN' network (decouple_net_v0_dilation)." % (v, att_source))
        if posenn_se != "none":
            raise UnsupportedVariantError("version `%s': `-se_insert' is not supported with the three-frame `-dilatedPoseNN' "
                                          "network (decouple_net_v0_dilation)." % v)
        if att_source != "ones" and not mask_rgb:
            # the precedent of `-se_insert' beside an attention source: a graph whose attention nothing applies is not built
            raise UnsupportedVariantError("version `%s': attention source `%s' without `-segmask' would be built and never read; "
                                          "the three-frame network runs an attention source only where it is applied." % (v, att_source))

    if heads == "coupled":
        # the coupled pair network (nets/posenn.py:133-187): every attention source of the pair network runs in front of it; the
        # feature-attention block has no coupled form here
        if posenn_se != "none":
            raise UnsupportedVariantError("version `%s': `-se_insert' is not supported with the coupled `-sharedNN-dilatedCouplePoseNN' "
                                          "network (couple_sharednet_v0_dilation)." % v)
        if att_source != "ones" and not mask_rgb:
            # the three-frame network's rule, in its words: a graph whose attention nothing applies is not built.  It is also what keeps
            # `v1-sharedNN-dilatedCouplePoseNN-se_flow' (no `-segmask'), pinned as rejected by tests/test_version.py, raising
            raise UnsupportedVariantError("version `%s': attention source `%s' without `-segmask' would be built and never read; "
                                          "the coupled network runs an attention source only where it is applied." % (v, att_source))

    return VariantConfig(version=v, major=major, use_flow_info=use_flow_info, cnv6_out=cnv6_out,
                         se_act=se_act, norm_flow=norm_flow, abs_mode=abs_mode,
                         att_source=att_source, mask_rgb=mask_rgb, mask_info=mask_info, posenn_se=posenn_se,
                         depth_thres_init=depth_thres_init, posenn=posenn, heads=heads)


def weight_shapes(cfg):
    """TF checkpoint names -> shapes for a variant (SURVEY table W; scopes from
    nets/posenn.py:203,221-223,240, nets/attention_module.py:63,94,101,
    nets/posenn.py:386-388)."""
    triplet = cfg.posenn == "triplet"
    # cnv1 reads concat(tgt, src) - or concat(tgt, src0, src1) in the three-frame network, whose pred has 3 * num_source outputs
    # (nets/posenn.py:78,120)
    c10 = (3 if triplet else 2) * cfg.cin_per_frame
    npred = 6 if triplet else 3
    c6 = cfg.cnv6_out
    sh = {
        "pose_exp_net/cnv1/weights": (7, 7, c10, 16), "pose_exp_net/cnv1/biases": (16,),
        "pose_exp_net/cnv2/weights": (5, 5, 16, 32), "pose_exp_net/cnv2/biases": (32,),
        "pose_exp_net/cnv3/weights": (3, 3, 32, 64), "pose_exp_net/cnv3/biases": (64,),
        "pose_exp_net/cnv4/weights": (3, 3, 64, 128), "pose_exp_net/cnv4/biases": (128,),
        "pose_exp_net/cnv5/weights": (3, 3, 128, 256), "pose_exp_net/cnv5/biases": (256,),
    }
    # the head scopes: rotation/ and translation/ with three (three-frame: six) pred columns each, or - coupled - pose/ itself with
    # six (nets/posenn.py:166-176: no rotation/ or translation/ scope)
    if cfg.heads == "coupled":
        head_scopes, npred = ["pose_exp_net/pose/"], 6
    else:
        head_scopes = ["pose_exp_net/pose/%s/" % head for head in ("rotation", "translation")]
    for p in head_scopes:
        sh[p + "cnv6/weights"] = (3, 3, 256, c6)
        sh[p + "cnv6/biases"] = (c6,)
        sh[p + "cnv7/weights"] = (3, 3, c6, 256)
        sh[p + "cnv7/biases"] = (256,)
        sh[p + "pred/weights"] = (1, 1, 256, npred)
        sh[p + "pred/biases"] = (npred,)
        if cfg.posenn_se == "insert":               # se_block(cnv5, 'cnv5_se_attention', ratio=8): nets/attention_module.py:37-49
            q = p + "cnv5_se_attention/"
            sh[q + "bottleneck_fc/kernel"] = (256, 256 // 8)
            sh[q + "bottleneck_fc/bias"] = (256 // 8,)
            sh[q + "recover_fc/kernel"] = (256 // 8, 256)
            sh[q + "recover_fc/bias"] = (256,)
    if cfg.se_scope is not None:
        nin, nh = _SE_WIDTHS[cfg.att_source]
        p = "pose_exp_net/%s/" % cfg.se_scope
        sh[p + "bottleneck_fc/kernel"] = (nin, nh)
        sh[p + "bottleneck_fc/bias"] = (nh,)
        sh[p + "recover_fc/kernel"] = (nh, NUM_SEG_CLASSES)
        sh[p + "recover_fc/bias"] = (NUM_SEG_CLASSES,)
    elif cfg.att_source == "se_flow_depthseg_sep":      # two se_flow MLPs and the trained threshold (davo.py:1136-1155)
        for scope in ("se_flow_near", "se_flow_far"):
            p = "pose_exp_net/%s/" % scope
            sh[p + "bottleneck_fc/kernel"] = (2, 8)
            sh[p + "bottleneck_fc/bias"] = (8,)
            sh[p + "recover_fc/kernel"] = (8, NUM_SEG_CLASSES)
            sh[p + "recover_fc/bias"] = (NUM_SEG_CLASSES,)
        sh["pose_exp_net/se_flow/depth_threshold"] = ()
    elif cfg.att_source in ("static_src", "static_all"):
        sh["pose_exp_net/pose_exp_net/seg_channel_weight/weight"] = (NUM_SEG_CLASSES,)
    return sh
